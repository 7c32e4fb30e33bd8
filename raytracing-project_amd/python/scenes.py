"""Scene inputs: the BASELINE.json configs and torture scenes.

Configs (BASELINE.json "configs"):
  1  examples/penguin.json unchanged, 1200x900 (CPU reference path)
  2  640x480 synthetic: 3 spheres + 1 halfSpace, 3 lights, recursion 1
  3  1920x1080 examples/pokeballs.json, 5 lights, recursion 3
  4  3840x2160 examples/snorlax.json (deep CSG), 5 lights, recursion 4
  5  7680x4320 synthetic 64 spheres + floor, 8 lights, recursion 6, --paper

Resize rule: dpi = W/4, dimensions = [4, H/dpi], screen
re-centred on the original screen centre.  Every function returns JSON text
in the reference schema (raytracer/src/json_loader.cpp).
"""
from __future__ import annotations

import copy
import json
import math
import os
from typing import NamedTuple

_HERE = os.path.dirname(os.path.abspath(__file__))
SCENE_DIR = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "tests", "golden", "scenes")

PENGUIN_LIGHTS = [
    {"position": [5, 6, 8], "intensity": [20, 20, 20]},
    {"position": [-5, 6, 8], "intensity": [15, 15, 15]},
    {"position": [0, 3, 7], "intensity": [12, 12, 12]},
]


def load_example(name: str) -> dict:
    with open(os.path.join(SCENE_DIR, f"{name}.json")) as f:
        return json.load(f)


def resize(scene: dict, width: int, height: int) -> dict:
    """Apply the resize rule: dpi = W/4, dims = [4, H/dpi], same screen centre."""
    s = copy.deepcopy(scene)
    scr = s["screen"]
    dims = scr.get("dimensions", [1, 1])
    P = scr["position"]
    cx, cy = P[0] + dims[0] / 2.0, P[1] + dims[1] / 2.0
    dpi = width // 4
    Ly = height / dpi
    scr["dpi"] = dpi
    scr["dimensions"] = [4, Ly]
    scr["position"] = [cx - 2.0, cy - Ly / 2.0, P[2]]
    return s


def with_dpi(scene: dict, dpi: int) -> dict:
    """Same screen, different dpi (used to make small parity cases)."""
    s = copy.deepcopy(scene)
    s["screen"]["dpi"] = dpi
    return s


def with_size(scene: dict, width: int, height: int, dpi: int = 16) -> dict:
    """Same scene and screen centre, a width x height frame at `dpi` (sizes
    that are no multiple of a wave's tile, odd widths)."""
    s = copy.deepcopy(scene)
    scr = s["screen"]
    dims = scr.get("dimensions", [1, 1])
    cx, cy = scr["position"][0] + dims[0] / 2, scr["position"][1] + dims[1] / 2
    scr["dpi"] = dpi
    scr["dimensions"] = [width / dpi, height / dpi]
    scr["position"] = [cx - width / dpi / 2, cy - height / dpi / 2, scr["position"][2]]
    return s


def cfg2_scene() -> dict:
    return {
        "screen": {"dpi": 160, "dimensions": [4, 3], "position": [-2, -1.5, 0], "observer": [0, 0, 5]},
        "medium": {"ambient": [0.1, 0.1, 0.1], "index": 1.0, "recursion": 1},
        "background": [0.2, 0.3, 0.5],
        "sources": copy.deepcopy(PENGUIN_LIGHTS),
        "objects": [
            {"halfSpace": {"position": [0, -1, 0], "normal": [0, 1, 0],
                           "color": {"diffuse": [0.6, 0.6, 0.6], "specular": [0.1, 0.1, 0.1], "shininess": 8}}},
            {"sphere": {"position": [-1.2, 0, -2], "radius": 0.8,
                        "color": {"diffuse": [0.9, 0.1, 0.1], "specular": [0.5, 0.5, 0.5], "shininess": 32}}},
            {"sphere": {"position": [0, 0, -3], "radius": 1.0,
                        "color": {"diffuse": [0.1, 0.8, 0.2], "reflected": [0.5, 0.5, 0.5], "shininess": 64}}},
            {"sphere": {"position": [1.2, 0, -2], "radius": 0.8, "index": 1.5,
                        "color": {"diffuse": [0.1, 0.2, 0.9], "refracted": [0.5, 0.5, 0.5], "shininess": 16}}},
        ],
    }


def cfg3_scene() -> dict:
    s = resize(load_example("pokeballs"), 1920, 1080)
    s["medium"]["recursion"] = 3
    return s


def cfg4_scene() -> dict:
    s = resize(load_example("snorlax"), 3840, 2160)
    s["sources"] = s["sources"] + [
        {"position": [0, 8, 2], "intensity": [20, 20, 20]},
        {"position": [3, -1, 6], "intensity": [15, 15, 15]},
    ]
    s["medium"]["recursion"] = 4
    return s


def cfg5_scene() -> dict:
    objs = [{"halfSpace": {"position": [0, -1.6, 0], "normal": [0, 1, 0],
                           "color": {"diffuse": [0.6, 0.6, 0.6], "specular": [0.1, 0.1, 0.1], "shininess": 8}}}]
    for k in range(64):
        i, j = k % 8, k // 8
        col = {"diffuse": [(i + 1) / 9.0, (j + 1) / 9.0, 0.5], "specular": [0.3, 0.3, 0.3],
               "shininess": 16 + 8 * (k % 4)}
        sph = {"position": [-3.5 + i, -1.2 + 0.35 * j, -2.0 - j], "radius": 0.3 + 0.05 * ((i + j) % 3), "color": col}
        if k % 3 == 0:
            col["reflected"] = [0.3, 0.3, 0.3]
        if k % 5 == 0:
            col["refracted"] = [0.4, 0.4, 0.4]
            sph["index"] = 1.5
        objs.append({"sphere": sph})
    lights = [{"position": [6 * math.cos(2 * math.pi * l / 8), 6, 2 + 6 * math.sin(2 * math.pi * l / 8)],
               "intensity": [20, 20, 20]} for l in range(8)]
    return {
        "screen": {"dpi": 1920, "dimensions": [4, 2.25], "position": [-2, -1.125, 0], "observer": [0, 0, 5]},
        "medium": {"ambient": [0.1, 0.1, 0.1], "index": 1.0, "recursion": 6},
        "background": [0.2, 0.3, 0.5],
        "sources": lights,
        "objects": objs,
    }


def bvh_scenes(dpi: int = 16) -> dict[str, dict]:
    """Scenes of more than kWaveBvhMin = 256 objects (no eager programs), for the wave BVH
    (CompiledScene::wobjs; tests/test_gpu_bvh.py):
      grid  576 spheres on a 24 x 24 lattice over a floor (every 5th
            reflective, every 7th refractive), 4 lights;
      ties  exact closest-hit ties between objects of both acceptance rules:
            pairs of coincident spheres, some wrapped in a CSG union with a
            tiny far sphere (its first hit t is the same double as the bare
            sphere's, its bound centre lies far away, so Morton order and the
            reference's order disagree about which of a pair comes first):
            sphere vs union (the sphere wins), union vs union (the earlier
            wins), sphere vs sphere (the later wins), in both orders and
            different colours;
      ties_mirror  ties with medium.recursion 3 and every 7th pair's visible
            spheres reflective: a wave BVH, reflection and CSG objects at once
            (k_std_secw<C, 2, false>, which neither grid - plain - nor ties -
            no mirrors - picks);
      nested / nested_mirror  the lattice of ties / ties_mirror without a
            tie: the second sphere of each pair has the same centre and a
            radius 0.05 smaller, so it lies inside the first and no two
            surfaces coincide.  For the FP32 kernels, which cannot keep the
            exact FP64 equality of t that decides a tie (a ray that sees the
            inner sphere's colour has lost the outer one)."""
    def mat(k):
        m = _mat([(k % 7) / 7.0, (k % 5) / 5.0, (k % 3) / 3.0], shininess=8 + 4 * (k % 5))
        if k % 5 == 0:
            m["reflected"] = [0.4, 0.4, 0.4]
        elif k % 7 == 0:
            m["refracted"] = [0.5, 0.5, 0.5]
        return m

    lights = [{"position": [4, 6, 3], "intensity": [30, 30, 30]}, {"position": [-5, 5, 2], "intensity": [20, 20, 20]},
              {"position": [0, 8, -4], "intensity": [15, 15, 15]}, {"position": [2, 1, 4], "intensity": [10, 10, 10]}]
    grid = [{"halfSpace": {"position": [0, -1.4, 0], "normal": [0, 1, 0], "color": _mat([0.6, 0.6, 0.6])}}]
    for k in range(576):
        i, j = k % 24, k // 24
        grid.append({"sphere": {"position": [-3.45 + 0.3 * i, -1.2 + 0.05 * (i % 3), -1.5 - 0.3 * j],
                                "radius": 0.1 + 0.03 * ((i + j) % 3), "color": mat(k), "index": 1.5}})
    ties = [{"halfSpace": {"position": [0, -1.4, 0], "normal": [0, 1, 0], "color": _mat([0.5, 0.5, 0.5])}}]
    for k in range(150):
        i, j = k % 15, k // 15
        c = [-3.5 + 0.5 * i, -1.0 + 0.3 * j, -2.5 - 0.5 * j]
        r = 0.18 + 0.04 * (k % 3)

        def bare(col):
            return {"sphere": {"position": list(c), "radius": r, "color": _mat(col)}}

        def wrapped(col, side):
            far = {"sphere": {"position": [c[0] + 40.0 * side, c[1] + 30.0, c[2] - 60.0], "radius": 0.01,
                              "color": _mat([0.5, 0.5, 0.5])}}
            return {"union": [{"sphere": {"position": list(c), "radius": r, "color": _mat(col)}}, far]}

        if k % 3 == 0:     # sphere vs union: the sphere wins either way
            pair = [bare([1.0, 0.1, 0.1]), wrapped([0.1, 1.0, 0.1], 1)]
        elif k % 3 == 1:   # union vs union: the earlier one wins
            pair = [wrapped([0.1, 1.0, 0.1], 1), wrapped([0.1, 0.1, 1.0], -1)]
        else:              # sphere vs sphere: the later one wins
            pair = [bare([1.0, 0.1, 0.1]), bare([1.0, 1.0, 0.1])]
        ties += pair if (k // 3) % 2 == 0 else pair[::-1]
    def mirror(o):   # (a pair member: a bare sphere, or a union whose first operand is the visible one)
        if "union" in o:
            mirror(o["union"][0])
        else:
            o["sphere"]["color"]["reflected"] = [0.4, 0.4, 0.4]

    ties_mirror = copy.deepcopy(ties)
    for k in range(0, 150, 7):
        mirror(ties_mirror[1 + 2 * k])
        mirror(ties_mirror[2 + 2 * k])
    nested = [copy.deepcopy(ties[0])]
    for k in range(150):
        i, j = k % 15, k // 15
        c = [-3.5 + 0.5 * i, -1.0 + 0.3 * j, -2.5 - 0.5 * j]
        r = 0.18 + 0.04 * (k % 3)
        outer = {"sphere": {"position": list(c), "radius": r, "color": _mat([1.0, 0.1 + 0.3 * (k % 3), 0.1])}}
        inner = {"sphere": {"position": list(c), "radius": r - 0.05, "color": _mat([0.1, 0.1, 1.0])}}
        nested += [outer, inner] if (k // 3) % 2 == 0 else [inner, outer]
    nested_mirror = copy.deepcopy(nested)
    for k in range(0, 150, 7):
        mirror(nested_mirror[1 + 2 * k])
        mirror(nested_mirror[2 + 2 * k])
    return {"nested": _base(nested, recursion=2, dpi=dpi, lights=lights[:2]),
            "nested_mirror": _base(nested_mirror, recursion=3, dpi=dpi, lights=lights[:2]),
            "grid": _base(grid, recursion=3, dpi=dpi, lights=lights),
            "ties": _base(ties, recursion=2, dpi=dpi, lights=lights[:2]),
            "ties_mirror": _base(ties_mirror, recursion=3, dpi=dpi, lights=lights[:2])}


def bvh_perf_scene(n: int = 4096, seed: int = 7, dpi: int = 480) -> dict:
    """n random spheres (seeded) over a floor, 4 lights, recursion 1, at
    dpi 480 (1920x1080): the wave BVH's perf case (tools/bvh_perf.py)."""
    import random
    rnd = random.Random(seed)
    objs = [{"halfSpace": {"position": [0, -1.4, 0], "normal": [0, 1, 0], "color": _mat([0.6, 0.6, 0.6])}}]
    for _ in range(n):
        objs.append({"sphere": {"position": [rnd.uniform(-6, 6), rnd.uniform(-1.3, 2.5), rnd.uniform(-14, -1.5)],
                                "radius": rnd.uniform(0.03, 0.12),
                                "color": _mat([rnd.random(), rnd.random(), rnd.random()], shininess=rnd.choice([8, 16, 32]))}})
    lights = [{"position": [4, 6, 3], "intensity": [30, 30, 30]}, {"position": [-5, 5, 2], "intensity": [20, 20, 20]},
              {"position": [0, 8, -4], "intensity": [15, 15, 15]}, {"position": [2, 1, 4], "intensity": [10, 10, 10]}]
    return _base(objs, recursion=1, dpi=dpi, lights=lights)


CONFIGS = {
    1: ("penguin 1200x900 (config 1)", lambda: load_example("penguin"), 0),
    2: ("synthetic 640x480 3 spheres + halfSpace, 3 lights, rec 1 (config 2)", cfg2_scene, 0),
    3: ("pokeballs 1920x1080, 5 lights, rec 3 (config 3)", cfg3_scene, 0),
    4: ("snorlax 3840x2160, 5 lights, rec 4 (config 4)", cfg4_scene, 0),
    5: ("synthetic 7680x4320 64 spheres, 8 lights, rec 6, paper (config 5)", cfg5_scene, 1),
    # not a BASELINE config: config 5's scene in STANDARD mode at 3840x2160, the
    # reflection / refraction recursion (tracer.cpp:22-73) at scale
    6: ("config-5 scene, standard mode 3840x2160, 8 lights, rec 6 (recursion row)",
        lambda: with_dpi(cfg5_scene(), 960), 0),
}


def config_json(n: int, dpi: int | None = None) -> tuple[str, int]:
    """(json_text, mode) for config n, optionally at a reduced dpi."""
    _, fn, mode = CONFIGS[n]
    s = fn()
    if dpi is not None:
        s = with_dpi(s, dpi)
    return json.dumps(s), mode


# ------------------------------------------------------------- torture scenes
def _mat(d, **kw):
    m = {"diffuse": list(d), "ambient": [0.05, 0.05, 0.05], "specular": [0.4, 0.4, 0.4], "shininess": 24}
    m.update(kw)
    return m


def _base(objects, recursion=3, dpi=24, lights=None):
    return {
        "screen": {"dpi": dpi, "dimensions": [4, 3], "position": [-2, -1.5, 0], "observer": [0, 0.3, 5]},
        "medium": {"ambient": [0.2, 0.2, 0.2], "index": 1.0, "recursion": recursion},
        "background": [0.3, 0.4, 0.6],
        "sources": lights or copy.deepcopy(PENGUIN_LIGHTS),
        "objects": objects,
    }


def torture_scenes(dpi: int = 24) -> dict[str, dict]:
    """Scenes covering every node kind, the CSG/transform quirks and recursion."""
    floor = {"halfSpace": {"position": [0, -1.2, 0], "normal": [0, 1, 0], "color": _mat([0.5, 0.6, 0.5])}}
    sc = {}
    sc["rotation_scaling"] = _base([
        floor,
        {"rotation": {"angle": 30, "direction": 1, "subject": {
            "scaling": {"factors": [1.5, 0.6, 1.0], "subject": {
                "sphere": {"position": [0, 0, 0], "radius": 0.8, "color": _mat([0.8, 0.3, 0.2])}}}}}},
        {"rotation": {"angle": -45, "direction": 2, "subject": {
            "translation": {"factors": [1.6, 0.2, -1.0], "subject": {
                "sphere": {"position": [0, 0, 0], "radius": 0.5, "color": _mat([0.2, 0.3, 0.9])}}}}}},
        {"rotation": {"angle": 60, "direction": 0, "subject": {
            "sphere": {"position": [-1.6, 0.3, -1.5], "radius": 0.6, "color": _mat([0.9, 0.9, 0.2])}}}},
    ], dpi=dpi)
    sc["csg_ops"] = _base([
        floor,
        {"intersection": [
            {"sphere": {"position": [-1.5, 0, -1], "radius": 0.9, "color": _mat([0.9, 0.2, 0.2])}},
            {"sphere": {"position": [-1.0, 0, -1], "radius": 0.9, "color": _mat([0.2, 0.9, 0.2])}}]},
        {"difference": [
            {"sphere": {"position": [0.3, 0.2, -1.5], "radius": 1.0, "color": _mat([0.9, 0.8, 0.2])}},
            {"sphere": {"position": [0.3, 0.2, -0.6], "radius": 0.6, "color": _mat([0.2, 0.2, 0.9])}},
            {"sphere": {"position": [0.9, 0.8, -1.0], "radius": 0.4, "color": _mat([0.7, 0.2, 0.7])}}]},
        {"csg": {"operator": "union",
                 "left": {"sphere": {"position": [1.8, -0.4, -1], "radius": 0.5, "color": _mat([0.3, 0.7, 0.9])}},
                 "right": {"union": [
                     {"sphere": {"position": [1.8, 0.3, -1], "radius": 0.35, "color": _mat([0.9, 0.5, 0.1])}},
                     {"sphere": {"position": [2.2, 0.0, -1], "radius": 0.3, "color": _mat([0.5, 0.9, 0.1])}}]}}},
    ], dpi=dpi)
    sc["halfspace_in_csg"] = _base([
        {"intersection": [
            {"sphere": {"position": [0, 0, -1.5], "radius": 1.2, "color": _mat([0.8, 0.4, 0.3])}},
            {"halfSpace": {"position": [0, 0.2, 0], "normal": [0.3, -1, 0.2], "color": _mat([0.3, 0.8, 0.4])}}]},
        {"difference": [
            {"sphere": {"position": [1.7, 0.3, -1.0], "radius": 0.7, "color": _mat([0.4, 0.4, 0.9])}},
            {"halfSpace": {"position": [1.7, 0.3, -1.0], "normal": [1, 1, 0], "color": _mat([0.9, 0.9, 0.9])}}]},
        {"union": [
            {"sphere": {"position": [-1.8, 0.0, -1.0], "radius": 0.5, "color": _mat([0.9, 0.9, 0.3])}},
            {"halfSpace": {"position": [0, -1.3, 0], "normal": [0, 1, 0], "color": _mat([0.4, 0.5, 0.4])}}]},
        {"translation": {"factors": [0.0, -0.2, 0.0], "subject": {
            "halfSpace": {"position": [0, -1.0, -6], "normal": [0, 0, 1], "color": _mat([0.5, 0.5, 0.7])}}}},
    ], dpi=dpi)
    sc["pokeball_csg"] = _base([
        floor,
        {"pokeball": {"position": [-1.2, 0, -1], "radius": 0.8, "button_dir": [0.2, 0.1, 1.0]}},
        {"difference": [
            {"pokeball": {"position": [1.2, 0, -1], "radius": 0.8, "button_dir": [-0.3, 0.2, 1.0],
                          "belt_half": 0.1, "button_outer": 0.35, "ring_width": 0.08}},
            {"sphere": {"position": [1.6, 0.5, -0.4], "radius": 0.4, "color": _mat([0.2, 0.2, 0.2])}}]},
        {"scaling": {"factors": [0.5, 0.5, 0.5], "subject": {
            "pokeball": {"position": [0, -1.6, -1], "radius": 0.8}}}},
    ], dpi=dpi)
    sc["reflect_refract"] = _base([
        floor,
        {"sphere": {"position": [-1.2, 0, -1.5], "radius": 0.7,
                    "color": _mat([0.2, 0.2, 0.2], reflected=[0.8, 0.8, 0.8])}},
        {"sphere": {"position": [0.3, -0.1, -0.8], "radius": 0.6, "index": 1.5,
                    "color": _mat([0.1, 0.1, 0.1], refracted=[0.9, 0.9, 0.9], reflected=[0.1, 0.1, 0.1])}},
        {"sphere": {"position": [1.6, 0.1, -1.2], "radius": 0.5, "index": 2.4,
                    "color": _mat([0.3, 0.1, 0.1], refracted=[0.7, 0.7, 0.7])}},
        {"difference": [
            {"sphere": {"position": [0.0, 1.0, -2.5], "radius": 0.6, "index": 1.3,
                        "color": _mat([0.5, 0.5, 0.8], refracted=[0.6, 0.6, 0.6], reflected=[0.3, 0.3, 0.3])}},
            {"sphere": {"position": [0.0, 1.0, -2.5], "radius": 0.3, "color": _mat([0.9, 0.2, 0.2])}}]},
    ], recursion=6, dpi=dpi)
    t_sph = {"translation": {"factors": [-1.2, 0.2, -1.0], "subject": {
        "sphere": {"position": [0, 0, 0], "radius": 0.6, "color": _mat([0.8, 0.3, 0.3])}}}}
    r_sph = {"rotation": {"angle": 35, "direction": 2, "subject": {"scaling": {"factors": [1.6, 0.5, 0.8], "subject": {
        "sphere": {"position": [-0.5, 0, -1.2], "radius": 0.5, "color": _mat([0.3, 0.8, 0.3])}}}}}}
    t_half = {"translation": {"factors": [0.0, 0.3, 0.0], "subject": {
        "halfSpace": {"position": [1.3, 0.0, -1.0], "normal": [0, 1, 0.2], "color": _mat([0.9, 0.9, 0.9])}}}}
    s_poke = {"scaling": {"factors": [1.0, 2.0, 1.0], "subject": {
        "pokeball": {"position": [0.0, 0.4, -2.5], "radius": 0.5, "button_dir": [0, 0, 1]}}}}
    sc["xform_in_csg"] = _base([
        floor,
        {"union": [t_sph, r_sph]},
        {"difference": [{"sphere": {"position": [1.3, 0.0, -1.0], "radius": 0.8, "color": _mat([0.3, 0.3, 0.9])}},
                        t_half]},
        {"intersection": [s_poke,
                          {"sphere": {"position": [0.0, 0.9, -2.5], "radius": 0.7, "color": _mat([0.9, 0.6, 0.2])}}]},
    ], dpi=dpi)
    def _cluster(cx, cy, cz, r, n, col, spread=0.18):
        out = []
        for i in range(n):
            a = 2.399963 * i
            out.append({"sphere": {"position": [cx + spread * math.cos(a), cy + spread * math.sin(a), cz + 0.05 * i],
                                   "radius": r * (1.0 - 0.08 * i), "color": _mat(col)}})
        return out
    # n-ary folds with runs of small spheres: OP_IVL_GROUP culling inside the
    # CSG program (scene_compile.cpp emit_compact_ivl) for all three operators
    sc["csg_groups"] = _base([
        floor,
        {"translation": {"factors": [-1.3, 0.1, -0.5], "subject": {"union": [
            {"sphere": {"position": [0, 0, -1], "radius": 0.7, "color": _mat([0.2, 0.5, 0.5])}},
            *_cluster(0.0, 0.75, -0.8, 0.12, 5, [0.9, 0.9, 0.9]),
            {"pokeball": {"position": [0.6, -0.5, -0.7], "radius": 0.2, "button_dir": [0, 0, 1]}},
            *_cluster(-0.6, -0.4, -0.6, 0.08, 4, [0.3, 0.2, 0.1], spread=0.1),
            {"halfSpace": {"position": [0, -0.55, 0], "normal": [0, -1, 0], "color": _mat([0.5, 0.5, 0.5])}},
            *_cluster(0.5, 0.4, -0.5, 0.1, 3, [0.8, 0.2, 0.2], spread=0.12)]}}},
        {"difference": [
            {"sphere": {"position": [1.2, 0.1, -1.2], "radius": 0.8, "color": _mat([0.8, 0.7, 0.3])}},
            *_cluster(1.2, 0.1, -0.45, 0.22, 6, [0.2, 0.2, 0.8], spread=0.35),
            *_cluster(1.7, 0.6, -1.0, 0.15, 3, [0.2, 0.8, 0.2], spread=0.1)]},
        {"intersection": [
            {"sphere": {"position": [0.0, -0.6, -0.4], "radius": 0.45, "color": _mat([0.7, 0.3, 0.7])}},
            {"sphere": {"position": [0.15, -0.5, -0.4], "radius": 0.45, "color": _mat([0.3, 0.7, 0.7])}},
            {"sphere": {"position": [-0.1, -0.45, -0.35], "radius": 0.4, "color": _mat([0.7, 0.7, 0.3])}},
            {"sphere": {"position": [0.05, -0.7, -0.45], "radius": 0.42, "color": _mat([0.5, 0.5, 0.5])}}]},
    ], dpi=dpi)
    sc["csg_groups_inside"] = {
        # eye inside an n-ary union whose later operands are grouped
        "screen": {"dpi": dpi, "dimensions": [4, 3], "position": [-2, -1.5, 0], "observer": [0, 0, 1]},
        "medium": {"ambient": [0.3, 0.3, 0.3], "index": 1.0, "recursion": 2},
        "background": [0.1, 0.1, 0.1],
        "sources": [{"position": [0, 0.5, 0.5], "intensity": [5, 5, 5]}],
        "objects": [
            {"union": [
                {"sphere": {"position": [0, 0, 1], "radius": 3.0, "color": _mat([0.6, 0.5, 0.4])}},
                *_cluster(0.3, 0.2, -1.5, 0.25, 5, [0.2, 0.5, 0.9], spread=0.4),
                *_cluster(-1.0, -0.6, -1.0, 0.2, 3, [0.9, 0.5, 0.2], spread=0.2)]},
            {"difference": [
                {"sphere": {"position": [0, 0, 1], "radius": 2.5, "color": _mat([0.4, 0.6, 0.4])}},
                *_cluster(0.0, 0.0, 1.0, 0.3, 4, [0.9, 0.9, 0.2], spread=0.2)]},
        ],
    }
    sc["recursion0"] = copy.deepcopy(sc["reflect_refract"])
    sc["recursion0"]["medium"]["recursion"] = 0
    sc["inside_camera"] = {
        # eye inside a CSG union and inside a sphere: origin-inside paths (csg.cpp:113-122)
        "screen": {"dpi": dpi, "dimensions": [4, 3], "position": [-2, -1.5, 0], "observer": [0, 0, 1]},
        "medium": {"ambient": [0.3, 0.3, 0.3], "index": 1.0, "recursion": 2},
        "background": [0.1, 0.1, 0.1],
        "sources": [{"position": [0, 0.5, 0.5], "intensity": [5, 5, 5]}],
        "objects": [
            {"union": [
                {"sphere": {"position": [0, 0, 1], "radius": 3.0, "color": _mat([0.6, 0.5, 0.4])}},
                {"sphere": {"position": [0, 0, -3], "radius": 1.0, "color": _mat([0.2, 0.5, 0.4])}}]},
            {"sphere": {"position": [0.5, 0, -1], "radius": 0.5, "color": _mat([0.9, 0.1, 0.1])}},
        ],
    }
    return sc


def deep_scenes(dpi: int = 12) -> dict[str, dict]:
    """Valid scenes beyond the common kernels' stacks (rt_launch.hpp): the
    reference recurses without a limit through trace_recursive
    (tracer.cpp:22-73), the transform wrappers (transform.cpp:18-255) and
    binary csg nodes (json_loader.cpp:354-366); the device runs these on its
    big-stack kernels.
      mirrors_rec24   reflective floor + ceiling, medium.recursion 24 (23 frames)
      xform_nest12    a sphere under 12 nested transforms inside a CSG operand
                      (eager program, ray stack 12) and as a bare chain
      csg_right12     a 12-leaf right-nested binary csg (interval stack 12)"""
    lights = [{"position": [0.0, 1.0, 2.0], "intensity": [6, 6, 6]},
              {"position": [-1.5, 0.5, -1.0], "intensity": [4, 3, 3]}]
    sc = {}
    sc["mirrors_rec24"] = _base([
        {"halfSpace": {"position": [0, -1.2, 0], "normal": [0, 1, 0],
                       "color": _mat([0.2, 0.3, 0.2], reflected=[0.85, 0.85, 0.85])}},
        {"halfSpace": {"position": [0, 1.6, 0], "normal": [0, -1, 0],
                       "color": _mat([0.3, 0.2, 0.2], reflected=[0.8, 0.8, 0.8])}},
        {"sphere": {"position": [-0.8, 0.0, -1.5], "radius": 0.6, "color": _mat([0.8, 0.5, 0.2])}},
        {"sphere": {"position": [0.9, 0.2, -2.0], "radius": 0.5, "index": 1.4,
                    "color": _mat([0.1, 0.1, 0.3], refracted=[0.8, 0.8, 0.8])}},
    ], recursion=24, dpi=dpi, lights=lights)

    def nest(leaf, n):
        node = leaf
        for k in range(n):
            if k % 3 == 0:
                node = {"translation": {"factors": [0.03 * (1 - 2 * (k % 2)), 0.02, 0.0], "subject": node}}
            elif k % 3 == 1:
                node = {"rotation": {"angle": 8 + k, "direction": k % 3, "subject": node}}
            else:
                node = {"scaling": {"factors": [1.03, 0.97, 1.01], "subject": node}}
        return node

    sc["xform_nest12"] = _base([
        {"halfSpace": {"position": [0, -1.2, 0], "normal": [0, 1, 0], "color": _mat([0.5, 0.6, 0.5])}},
        {"union": [nest({"sphere": {"position": [-0.9, 0.0, -1.0], "radius": 0.6, "color": _mat([0.8, 0.3, 0.3])}},
                        12),
                   {"sphere": {"position": [-0.2, 0.5, -1.4], "radius": 0.4, "color": _mat([0.3, 0.3, 0.8])}}]},
        nest({"sphere": {"position": [1.0, 0.0, -1.2], "radius": 0.5, "color": _mat([0.3, 0.8, 0.3])}}, 12),
    ], dpi=dpi)

    def right_nested(leaves, ops):
        node = leaves[-1]
        for leaf, op in zip(reversed(leaves[:-1]), reversed(ops)):
            node = {"csg": {"operator": op, "left": leaf, "right": node}}
        return node

    leaves = [{"sphere": {"position": [-1.6 + 0.3 * i, 0.25 * math.sin(i), -1.2 - 0.1 * i], "radius": 0.35 + 0.02 * i,
                          "color": _mat([0.2 + 0.06 * i, 0.8 - 0.05 * i, 0.4])}} for i in range(12)]
    ops = ["union"] * 5 + ["difference"] + ["union"] * 3 + ["intersection"] + ["union"]
    sc["csg_right12"] = _base([
        {"halfSpace": {"position": [0, -1.2, 0], "normal": [0, 1, 0], "color": _mat([0.5, 0.6, 0.5])}},
        right_nested(leaves, ops),
    ], dpi=dpi)
    return sc


def dir_light_cases(dpi: int = 16) -> dict[str, tuple[str, list]]:
    """Scenes with directional lights (the reference's Scene::dir_lights,
    scene.h:10-15; its loader never creates them, so they are attached to the
    IR: rtamd.with_dir_lights).  Cases: a sun and a back light beside point
    lights, a zero direction (Vec4::normalized's (0,1,0) fallback,
    core.h:58-64), the deep-CSG scene, and reflection/refraction recursion."""
    sun = ([-0.4, -1.0, -0.3], [0.9, 0.85, 0.8])
    back = ([0.0, 0.3, 1.0], [0.3, 0.3, 0.5])       # from behind the camera's view: mostly ndotl <= 0
    zero = ([0.0, 0.0, 0.0], [0.2, 0.2, 0.2])
    tort = torture_scenes(dpi=dpi)
    return {
        "cfg2_sun_back": (config_json(2, dpi=dpi)[0], [sun, back]),
        "cfg2_zero_dir": (config_json(2, dpi=dpi)[0], [zero]),
        "snorlax_sun": (json.dumps(with_dpi(load_example("snorlax"), dpi)), [sun]),
        "reflect_refract_sun": (json.dumps(tort["reflect_refract"]), [sun, back]),
        "pokeball_csg_sun": (json.dumps(tort["pokeball_csg"]), [sun]),
    }


def crowd_scene(seed: int, n_objects: int = 150, dpi: int = 16) -> dict:
    """A seeded random scene with more top-level objects than one wave's
    transposed cull test covers (64 per pass): spheres (some reflective or
    refractive), pokeballs, n-ary and binary CSG of spheres (with a half-space
    now and then), transforms over spheres and CSG, bare half-spaces; 4 point
    lights, recursion 3.  Exercises the multi-pass wave culling, groups and
    the fold / compact / eager CSG paths together (tests/test_gpu_crowd.py)."""
    import random
    rnd = random.Random(seed)

    def col():
        m = _mat([rnd.random(), rnd.random(), rnd.random()], shininess=rnd.choice([4, 8, 16, 32]))
        u = rnd.random()
        if u < 0.12:
            m["reflected"] = [0.5, 0.5, 0.5]
        elif u < 0.2:
            m["refracted"] = [0.6, 0.6, 0.6]
        return m

    def pos(spread=3.0):
        return [rnd.uniform(-spread, spread), rnd.uniform(-1.0, 1.8), rnd.uniform(-7.0, -0.5)]

    def sphere(p=None, r=None):
        return {"sphere": {"position": p or pos(), "radius": r or rnd.uniform(0.08, 0.45), "color": col(),
                           "index": rnd.choice([1.0, 1.33, 1.5])}}

    def csg():
        c = pos()
        leaves = [sphere([c[0] + rnd.uniform(-0.3, 0.3), c[1] + rnd.uniform(-0.3, 0.3), c[2] + rnd.uniform(-0.3, 0.3)],
                         rnd.uniform(0.1, 0.4)) for _ in range(rnd.randint(2, 6))]
        op = rnd.choice(["union", "union", "difference", "intersection"])
        if op != "union" and rnd.random() < 0.3:
            # (a half-space only where the CSG stays bounded: a union with one
            # would contain the camera and reduce every pixel to the
            # origin-inside entry)
            leaves.append({"halfSpace": {"position": c, "normal": [rnd.uniform(-1, 1), 1.0, rnd.uniform(-1, 1)],
                                         "color": col()}})
        if rnd.random() < 0.3 and len(leaves) >= 2:
            return {"csg": {"operator": op, "left": leaves[0], "right": {"union": leaves[1:]} if len(leaves) > 2
                            else leaves[1]}}
        return {op: leaves}

    def xform(sub):
        k = rnd.randint(0, 2)
        if k == 0:
            return {"translation": {"factors": [rnd.uniform(-0.5, 0.5) for _ in range(3)], "subject": sub}}
        if k == 1:
            return {"rotation": {"angle": rnd.uniform(-60, 60), "direction": rnd.randint(0, 2), "subject": sub}}
        return {"scaling": {"factors": [rnd.uniform(0.6, 1.4) for _ in range(3)], "subject": sub}}

    objs = [{"halfSpace": {"position": [0, -1.3, 0], "normal": [0, 1, 0], "color": col()}}]
    while len(objs) < n_objects:
        u = rnd.random()
        if u < 0.5:
            objs.append(sphere())
        elif u < 0.58:
            objs.append({"pokeball": {"position": pos(), "radius": rnd.uniform(0.15, 0.4),
                                      "button_dir": [rnd.uniform(-1, 1), rnd.uniform(-1, 1), 1.0]}})
        elif u < 0.8:
            objs.append(csg())
        elif u < 0.97:
            objs.append(xform(rnd.choice([sphere(), csg()])))
        else:
            objs.append({"halfSpace": {"position": [0, 0, -9], "normal": [rnd.uniform(-0.2, 0.2), 0, 1], "color": col()}})
    lights = [{"position": [rnd.uniform(-6, 6), rnd.uniform(3, 7), rnd.uniform(-2, 6)],
               "intensity": [rnd.uniform(8, 25)] * 3} for _ in range(4)]
    return _base(objs, recursion=3, dpi=dpi, lights=lights)


# ------------------------------------------------------- scene-graph scenes
def _tr(f, sub):
    return {"translation": {"factors": [float(v) for v in f], "subject": sub}}


def _sc(f, sub):
    return {"scaling": {"factors": [float(v) for v in f], "subject": sub}}


def _rot(angle, axis, sub):
    return {"rotation": {"angle": angle, "direction": axis, "subject": sub}}


def _half(p, n, col):
    return {"halfSpace": {"position": [float(v) for v in p], "normal": [float(v) for v in n], "color": col}}


GRAPH_NULL_CENTRE = [-0.9, 0.0, -1.0]


def graph_cases(dpi: int = 24) -> dict[str, dict]:
    """Hand-written scenes for the compiled object forms and the scene shapes
    no other family has (scene_compile.cpp; tests/test_graph_scenes.py,
    tests/test_gpu_graph.py), each over a floor or another hit surface:
      never_top        a degenerate Scaling (a factor below 1e-6,
                       transform.cpp:103) as a top-level object: OBJ_NEVER
      never_in_csg     that subtree as the right operand of a union, a
                       difference and an intersection and as the left operand
                       of a difference (OP_NEVER in interval mode; an Empty
                       bound on either side of every operator)
      never_mid_chain  translation(scaling [1, 0, 1](rotation(sphere)))
      neg_scale        mirrors: negative factors over a sphere, a pokeball
                       (its button direction mirrored) and a difference
      big_scale_fallback  scaling [2e6] * 3: the local direction is shorter
                       than 1e-6 and Ray's constructor replaces it by
                       (0, 1, 0) (core.h:278), so the local ray is no image of
                       the world ray and no bound of the subtree holds
      scale_1e5        factors 1e5 over a sphere of radius 6e-6, 1e-5 over one
                       of radius 5e4
      scale_threshold  factor 1e-6 (not degenerate: a disc 1.6e-6 thick seen
                       from the side) and 0.99e-6 (degenerate)
      rot_right_angles rotations by 90, 180, 360, -450 and 0 degrees
      xform_half       transforms directly over half-spaces (unbounded chains)
      csg_self         union, intersection and difference of a sphere with
                       itself: every event a tie of the event order
      csg_concentric_tangent  a shell, externally tangent spheres, a disjoint
                       intersection, a small sphere minus one that encloses it
      csg_unbounded    a slab of two half-spaces, a wall minus a sphere
      mixed_deep       CSG of other operators under CSG, transforms inside
                       operands and over the whole
      null_mat_eager   a union with a leaf that has no material (graph_load
                       removes it): a non-compact core, so an eager program"""
    floor = _floor()
    sc = {}

    def put(name, objs):
        sc[name] = _base(objs, recursion=3, dpi=dpi)

    def deg():
        return _sc([1e-7, 1, 1], _sph([0, 0, 0], 0.5, _mat([0.9, 0.1, 0.9])))

    put("never_top", [floor, _sc([1e-7, 1, 1], _sph([-0.8, 0.0, -1.0], 0.6, _mat([0.9, 0.1, 0.9]))),
                      _sph([0.8, 0.0, -1.5], 0.6, _mat([0.2, 0.5, 0.9]))])
    put("never_in_csg", [
        floor,
        _tr([-1.5, 0.0, -1.0], {"union": [_sph([0, 0, 0], 0.5, _mat([0.9, 0.3, 0.2])), deg()]}),
        _tr([-0.3, 0.2, -1.5], {"difference": [_sph([0, 0, 0], 0.6, _mat([0.3, 0.9, 0.2])), deg()]}),
        _tr([0.9, 0.0, -1.0], {"intersection": [_sph([0, 0, 0], 0.5, _mat([0.2, 0.3, 0.9])), deg()]}),
        {"difference": [_tr([1.7, 0.5, -1.0], deg()), _sph([1.7, 0.5, -1.0], 0.4, _mat([0.9, 0.9, 0.2]))]},
        _sph([1.6, -0.5, -0.5], 0.4, _mat([0.2, 0.8, 0.8], reflected=[0.4, 0.4, 0.4])),
    ])
    put("never_mid_chain", [
        floor,
        _tr([-0.8, 0.0, -1.0], _sc([1, 0, 1], _rot(30, 1, _sph([0, 0, 0], 0.6, _mat([0.9, 0.1, 0.9]))))),
        _sph([0.8, 0.0, -1.5], 0.6, _mat([0.8, 0.6, 0.2], reflected=[0.3, 0.3, 0.3]))])
    put("neg_scale", [
        floor,
        _sc([-1.5, 1, 1], _sph([0.9, 0.1, -1.5], 0.5, _mat([0.9, 0.3, 0.2], reflected=[0.3, 0.3, 0.3]))),
        _sc([1, -1, -0.8], {"pokeball": {"position": [0.0, -0.3, 1.5], "radius": 0.5, "button_dir": [0.3, -0.2, -1.0]}}),
        _sc([-1, -1, -1], {"difference": [
            _sph([-1.3, -0.2, 1.2], 0.6, _mat([0.3, 0.4, 0.9], refracted=[0.5, 0.5, 0.5]), index=1.5),
            _sph([-1.3, -0.4, 0.7], 0.4, _mat([0.9, 0.9, 0.2]))]})])
    put("big_scale_fallback", [floor, _sc([2e6, 2e6, 2e6], _sph([0, 0.5, 0], 0.4, _mat([0.9, 0.5, 0.1]))),
                               _sph([1.2, 0.0, -1.5], 0.6, _mat([0.2, 0.5, 0.9]))])
    put("scale_1e5", [
        floor,
        _sc([1e5] * 3, _sph([-1e-5, 0.0, -1.2e-5], 6e-6, _mat([0.9, 0.3, 0.2]))),
        _sc([1e-5] * 3, _sph([1e5, 0.0, -1.5e5], 5e4, _mat([0.2, 0.5, 0.9], reflected=[0.3, 0.3, 0.3])))])
    put("scale_threshold", [
        floor,
        _sc([1e-6, 1, 1], _sph([1e6, 0.0, 1.5], 0.8, _mat([0.9, 0.3, 0.2]))),
        _sc([0.99e-6, 1, 1], _sph([-1e6 / 0.99, 0.0, 1.5], 0.8, _mat([0.9, 0.1, 0.9]))),
        _sph([0.0, -0.3, -1.5], 0.7, _mat([0.2, 0.5, 0.9]))])
    put("rot_right_angles", [
        floor,
        _rot(90, 0, _sph([-1.4, 1.0, -0.8], 0.45, _mat([0.9, 0.3, 0.2]))),               # -> (-1.4, 0.8, 1.0)
        _rot(180, 1, _sph([-1.0, -0.4, 1.5], 0.5, _mat([0.3, 0.9, 0.2]))),               # -> (1.0, -0.4, -1.5)
        _rot(360, 2, _sph([0.0, 0.9, -2.0], 0.5, _mat([0.2, 0.3, 0.9], reflected=[0.4, 0.4, 0.4]))),
        _rot(-450, 2, {"pokeball": {"position": [0.5, -0.9, -1.0], "radius": 0.45, "button_dir": [0.2, 0.1, 1.0]}}),
        _rot(0, 1, _tr([0, 0, 0], _sph([1.5, 0.7, -1.0], 0.4, _mat([0.9, 0.9, 0.2]))))])
    put("xform_half", [
        _rot(8, 2, _floor()),
        _sc([1, 2, 0.5], _half([0, 0, -12], [0, 0, 1], _mat([0.5, 0.5, 0.7]))),
        _tr([0.5, 0, 0], _sc([-1, 1, 1], _half([2.7, 0, 0], [-1, 0, 0.2], _mat([0.7, 0.5, 0.5])))),
        _sph([0.3, 0.0, -1.5], 0.7, _mat([0.2, 0.7, 0.4], reflected=[0.3, 0.3, 0.3]))])

    def same(c, r, col):
        return [_sph(c, r, _mat(col)), _sph(c, r, _mat(col))]

    put("csg_self", [floor, {"union": same([-1.4, 0.0, -1.0], 0.6, [0.9, 0.3, 0.2])},
                     {"intersection": same([0.0, 0.2, -1.5], 0.6, [0.3, 0.9, 0.2])},
                     {"difference": same([1.4, 0.0, -1.0], 0.6, [0.2, 0.3, 0.9])}])
    put("csg_concentric_tangent", [
        floor,
        {"difference": [_sph([-1.3, 0.0, -1.0], 0.6, _mat([0.9, 0.3, 0.2], refracted=[0.6, 0.6, 0.6]), index=1.3),
                        _sph([-1.3, 0.0, -1.0], 0.4, _mat([0.2, 0.9, 0.3]))]},
        {"union": [_sph([0.0, 0.3, -1.5], 0.4, _mat([0.3, 0.3, 0.9])), _sph([0.8, 0.3, -1.5], 0.4, _mat([0.9, 0.9, 0.2]))]},
        {"intersection": [_sph([1.6, -0.5, -0.6], 0.3, _mat([0.9, 0.1, 0.9])),
                          _sph([1.6, 0.9, -0.6], 0.3, _mat([0.9, 0.1, 0.9]))]},
        {"difference": [_sph([-0.3, -0.6, -0.3], 0.2, _mat([0.9, 0.1, 0.9])),
                        _sph([-0.3, -0.6, -0.3], 0.5, _mat([0.9, 0.1, 0.9]))]}])
    put("csg_unbounded", [
        # (a half-space is solid on the side its normal points to)
        {"intersection": [_half([0, -1.0, 0], [0, -1, 0], _mat([0.5, 0.6, 0.5])),
                          _half([0, -1.4, 0], [0, 1, 0], _mat([0.6, 0.5, 0.5]))]},
        {"difference": [_half([0, 0, -5], [0, 0, -1], _mat([0.5, 0.5, 0.7])),
                        _sph([0.0, 0.3, -5.0], 1.2, _mat([0.9, 0.6, 0.2]))]},
        _sph([1.2, -0.3, -1.5], 0.6, _mat([0.2, 0.5, 0.9], reflected=[0.3, 0.3, 0.3]))])
    put("mixed_deep", [
        floor,
        {"difference": [
            {"union": [_sph([-1.1, 0.1, -1.2], 0.6, _mat([0.9, 0.3, 0.2])),
                       _rot(40, 2, _sc([1.5, 0.6, 1.0], _sph([-0.35, 0.55, -1.2], 0.45, _mat([0.3, 0.9, 0.2]))))]},
            {"intersection": [_tr([-0.9, 0.2, -0.6], {"pokeball": {"position": [0, 0, 0], "radius": 0.45,
                                                                   "button_dir": [0.1, 0.2, 1.0]}}),
                              _half([0, 0.1, 0], [0, -1, 0], _mat([0.8, 0.8, 0.8]))]}]},
        _tr([1.2, 0.1, -1.3], _rot(25, 1, {"csg": {
            "operator": "intersection",
            "left": {"union": [_sph([-0.25, 0, 0], 0.5, _mat([0.2, 0.3, 0.9])),
                               _sph([0.25, 0, 0], 0.5, _mat([0.9, 0.9, 0.2], reflected=[0.3, 0.3, 0.3]))]},
            "right": {"difference": [_sph([0, 0.1, 0], 0.6, _mat([0.9, 0.2, 0.7])),
                                     _sph([0, 0.2, 0.5], 0.3, _mat([0.2, 0.9, 0.9]))]}}}))])
    put("null_mat_eager", [
        floor,
        {"union": [_sph(GRAPH_NULL_CENTRE, 0.6, _mat([0.5, 0.5, 0.5])),
                   _sph([-0.3, 0.3, -1.2], 0.5, _mat([0.3, 0.8, 0.3]))]},
        _sph([1.1, 0.0, -1.5], 0.6, _mat([0.2, 0.3, 0.4], reflected=[0.6, 0.6, 0.6]))])
    return sc


GRAPH_EAGER_CASES = ("never_in_csg", "mixed_deep", "null_mat_eager")
# the named cases with a transform or a never-hit form (the radiance tests)
GRAPH_XFORM_CASES = ("never_top", "never_in_csg", "never_mid_chain", "neg_scale", "big_scale_fallback", "scale_1e5",
                     "scale_threshold", "rot_right_angles", "xform_half", "mixed_deep")


def graph_load(rt, name: str, scene: dict):
    """graph_cases()[name] (or a graph_scene) as a loaded scene: null_mat_eager
    loses the material of the sphere at GRAPH_NULL_CENTRE, which the JSON
    schema cannot spell (rt = the rtamd module)."""
    sc = rt.load_scene_from_json_text(json.dumps(scene))
    if name == "null_mat_eager":
        sc = rt.with_null_materials(sc, rt.sphere_nodes_at(sc, [GRAPH_NULL_CENTRE]))
    return sc


# Transform parameters of graph_scene: scaling factor triples (mirrors, factors
# down to 1e-3 and up to 1e3, degenerate ones last) and rotation angles.
_GRAPH_FACTORS = ([-1, 1, 1], [1, -1, 1], [-1, -1, -1], [0.5, 2, 1], [1.3, 0.7, 1.0], [2, 0.5, -1.5], [1e-3, 1e-3, 1e-3],
                  [1e3, 1e3, 1e3], [-40, 40, 40], [0.02, 0.05, 0.02], [1, 1, 1], [0.8, 0.8, 1.25])
_GRAPH_DEGENERATE = ([1, 0, 1], [1e-7, 1, 1], [1, 1, -5e-7])
_GRAPH_ANGLES = (0, 90, 180, 270, 360, -90, 450, -450, 30, -45, 60, 137.5, 1e-9)


def graph_scene(seed: int, dpi: int = 16) -> dict:
    """A seeded random scene graph: about 10 top-level objects over a floor,
    each a recursive choice (depth up to 4) among sphere, pokeball,
    translation, rotation, scaling and the three CSG operators (n-ary arrays
    or a binary csg node) with operands of any kind - a CSG of another
    operator, a transform inside an operand, a half-space as the last operand
    of a difference or an intersection (never of a union, as crowd_scene
    explains).  Transform parameters come from _GRAPH_FACTORS / _GRAPH_ANGLES,
    now and then a degenerate factor.  A node is built around the point and
    size it should have in its parent's frame, so that every object stays in
    view whatever stands above it.  Lights and materials as crowd_scene."""
    import random
    rnd = random.Random(seed)

    def col():
        m = _mat([rnd.random(), rnd.random(), rnd.random()], shininess=rnd.choice([4, 8, 16, 32]))
        u = rnd.random()
        if u < 0.12:
            m["reflected"] = [0.5, 0.5, 0.5]
        elif u < 0.2:
            m["refracted"] = [0.6, 0.6, 0.6]
        return m

    def leaf(c, r):
        if rnd.random() < 0.25:
            return {"pokeball": {"position": list(c), "radius": r,
                                 "button_dir": [rnd.uniform(-1, 1), rnd.uniform(-1, 1), 1.0]}}
        return {"sphere": {"position": list(c), "radius": r, "color": col(), "index": rnd.choice([1.0, 1.33, 1.5])}}

    def near(c, r, k=0.6):
        return [c[i] + rnd.uniform(-k, k) * r for i in range(3)]

    def xform(c, r, depth):
        k = rnd.randint(0, 2)
        if k == 0:
            f = [rnd.uniform(-1.5, 1.5) * rnd.choice([0, 1, 1]) for _ in range(3)]
            return _tr(f, node([c[i] - f[i] for i in range(3)], r, depth - 1))
        if k == 1:
            ang, ax = rnd.choice(_GRAPH_ANGLES), rnd.randint(0, 2)
            a = -math.radians(ang)
            i, j = [(1, 2), (2, 0), (0, 1)][ax]
            q = list(c)
            q[i] = math.cos(a) * c[i] - math.sin(a) * c[j]
            q[j] = math.sin(a) * c[i] + math.cos(a) * c[j]
            return _rot(ang, ax, node(q, r, depth - 1))
        if rnd.random() < 0.06:
            return _sc(rnd.choice(_GRAPH_DEGENERATE), node(c, r, depth - 1))
        f = rnd.choice(_GRAPH_FACTORS)
        g = abs(f[0] * f[1] * f[2]) ** (1.0 / 3.0)
        return _sc(f, node([c[i] / f[i] for i in range(3)], r / g, depth - 1))

    def csg(c, r, depth):
        op = rnd.choice(["union", "union", "difference", "intersection"])
        n = rnd.choice([2, 2, 3, 4, 6])
        # a union's operands spread out, the others overlap the first
        spread = 0.8 if op == "union" else 0.45
        kids = [node(near(c, r, 0.3), 0.75 * r, depth - 1)]
        kids += [node(near(c, r, spread), rnd.uniform(0.35, 0.7) * r, depth - 1 if rnd.random() < 0.5 else 0)
                 for _ in range(n - 1)]
        if op != "union" and rnd.random() < 0.3:
            kids.append(_half(near(c, r, 0.3), [rnd.uniform(-1, 1), 1.0, rnd.uniform(-1, 1)], col()))
        if rnd.random() < 0.35:
            rest = kids[1:]
            right = rest[0] if len(rest) == 1 else {rnd.choice(["union", "union", "intersection"])
                                                    if op != "union" else "union": rest}
            if "halfSpace" in rest[-1] and len(rest) > 1:
                # (the half-space stays the last operand of its own operator)
                right = {op if op == "intersection" else "union": rest[:-1]}
                return {"csg": {"operator": op, "left": {"csg": {"operator": op, "left": kids[0], "right": right}},
                                "right": rest[-1]}}
            return {"csg": {"operator": op, "left": kids[0], "right": right}}
        return {op: kids}

    def node(c, r, depth):
        u = rnd.random()
        if depth <= 0 or u < 0.2:
            return leaf(c, r)
        if u < 0.6:
            return xform(c, r, depth)
        return csg(c, r, depth)

    objs = [{"halfSpace": {"position": [0, -1.3, 0], "normal": [0, 1, 0], "color": col()}}]
    for k in range(10):
        c = [-2.4 + 1.2 * (k % 5) + rnd.uniform(-0.2, 0.2), rnd.uniform(-0.6, 1.2), -1.0 - 1.6 * (k // 5)
             + rnd.uniform(-0.3, 0.3)]
        objs.append(node(c, rnd.uniform(0.35, 0.6), rnd.randint(1, 4)))
    lights = [{"position": [rnd.uniform(-6, 6), rnd.uniform(3, 7), rnd.uniform(-2, 6)],
               "intensity": [rnd.uniform(8, 25)] * 3} for _ in range(4)]
    return _base(objs, recursion=3, dpi=dpi, lights=lights)


# ------------------------------------------------------------ forest scenes
# Scalings of forest_scene: mirrors and anisotropic factors whose largest ratio
# is 4, so that two nested ones stay within the ratio of 16 up to which a
# Scaling keeps its bound (scene_compile.cpp xform_ball).
_FOREST_FACTORS = ([-1, 1, 1], [1, -1, 1], [-1, -1, -1], [0.5, 2, 1], [1.3, 0.7, 1.0], [2, 0.5, -1.5], [0.8, 0.8, 1.25])
_FOREST_ANGLES = (30, 90, 180, -45, 270)
FOREST_SUN = ([-0.4, -1.0, -0.3], [0.9, 0.85, 0.8])    # the sun of dir_light_cases
FOREST_SEEDS = (1, 2, 3, 4)
_FOREST_LIGHTS = [{"position": [4, 6, 3], "intensity": [30, 30, 30]}, {"position": [-5, 5, 2], "intensity": [20, 20, 20]},
                  {"position": [0, 8, -4], "intensity": [15, 15, 15]}]


def forest_scene(seed: int, n: int, n_unbounded: int = 1, eager: bool = False, dpi: int = 16) -> dict:
    """A seeded scene of n top-level objects of mixed compiled forms behind
    n_unbounded half-space floors (y = -1.4 - 0.01 k), for the wave BVH and the
    ray BVH (more than 256 objects; tests/test_forest_scenes.py,
    tests/test_gpu_forest.py).  The objects stand on a jittered
    ceil(sqrt(n))-square lattice that fills the view (x in [-3.4, 3.4], z from
    -1.5 to -7.5, y in [-1.1, 1.4], radius in [0.08, 0.2]); each is a leaf
    (about 35 %: a sphere, one in five a pokeball), an n-ary union, difference
    or intersection of 2-4 leaves (25 %; the last two now and then with a
    half-space as last operand), one transform over a leaf (20 %) or over such
    a CSG (13 %), or two nested transforms over a leaf (7 %).  A transform's
    subject is placed so that its image lands on the lattice point, as in
    graph_scene.  No transform stands inside a CSG operand, so no object
    compiles to an eager program; eager=True appends exactly one that does.
    10 % of the materials are reflective, 8 % refractive; recursion 2, three
    lights."""
    import random
    rnd = random.Random(seed)

    def col():
        m = _mat([rnd.random(), rnd.random(), rnd.random()], shininess=rnd.choice([4, 8, 16, 32]))
        u = rnd.random()
        if u < 0.10:
            m["reflected"] = [0.5, 0.5, 0.5]
        elif u < 0.18:
            m["refracted"] = [0.6, 0.6, 0.6]
        return m

    def leaf(c, r):
        if rnd.random() < 0.2:
            return {"pokeball": {"position": list(c), "radius": r,
                                 "button_dir": [rnd.uniform(-1, 1), rnd.uniform(-1, 1), 1.0]}}
        return {"sphere": {"position": list(c), "radius": r, "color": col(), "index": rnd.choice([1.0, 1.33, 1.5])}}

    def csg(c, r):
        op = rnd.choice(["union", "difference", "intersection"])
        spread = 0.8 if op == "union" else 0.45
        kids = [leaf(c, r)]
        kids += [leaf([c[i] + rnd.uniform(-spread, spread) * r for i in range(3)], rnd.uniform(0.5, 0.9) * r)
                 for _ in range(rnd.randint(1, 3))]
        if op != "union" and rnd.random() < 0.25:
            kids.append(_half([c[i] + rnd.uniform(-0.3, 0.3) * r for i in range(3)],
                              [rnd.uniform(-1, 1), 1.0, rnd.uniform(-1, 1)], col()))
        return {op: kids}

    def xform(c, r, levels, core):
        if levels == 0:
            return core(c, r)
        k = rnd.randint(0, 2)
        if k == 0:
            f = [rnd.uniform(-1.5, 1.5) for _ in range(3)]
            return _tr(f, xform([c[i] - f[i] for i in range(3)], r, levels - 1, core))
        if k == 1:
            ang, ax = rnd.choice(_FOREST_ANGLES), rnd.randint(0, 2)
            a = -math.radians(ang)
            i, j = [(1, 2), (2, 0), (0, 1)][ax]
            q = list(c)
            q[i] = math.cos(a) * c[i] - math.sin(a) * c[j]
            q[j] = math.sin(a) * c[i] + math.cos(a) * c[j]
            return _rot(ang, ax, xform(q, r, levels - 1, core))
        f = rnd.choice(_FOREST_FACTORS)
        g = abs(f[0] * f[1] * f[2]) ** (1.0 / 3.0)
        return _sc(f, xform([c[i] / f[i] for i in range(3)], r / g, levels - 1, core))

    objs = [_half([0, -1.4 - 0.01 * k, 0], [0, 1, 0], col()) for k in range(n_unbounded)]
    side = max(1, math.ceil(math.sqrt(n)))
    for k in range(n):
        i, j = k % side, k // side
        c = [-3.4 + 6.8 * (i + 0.5 + rnd.uniform(-0.3, 0.3)) / side, rnd.uniform(-1.1, 1.4),
             -1.5 - 6.0 * (j + 0.5 + rnd.uniform(-0.3, 0.3)) / side]
        r = rnd.uniform(0.08, 0.2)
        u = rnd.random()
        if u < 0.35:
            objs.append(leaf(c, r))
        elif u < 0.60:
            objs.append(csg(c, r))
        elif u < 0.80:
            objs.append(xform(c, r, 1, leaf))
        elif u < 0.93:
            objs.append(xform(c, r, 1, csg))
        else:
            objs.append(xform(c, r, 2, leaf))
    if eager:
        c = [0.2, 0.4, -1.2]
        objs.append({"union": [leaf(c, 0.2), _tr([0.3, 0.1, 0.0], leaf([c[0] - 0.1, c[1] - 0.1, c[2]], 0.15))]})
    return _base(objs, recursion=2, dpi=dpi, lights=copy.deepcopy(_FOREST_LIGHTS))


FOREST_TIE_KINDS = ("tr/rot", "rot/sc", "sc/tr", "rot/tr_union", "tr_union/tr")


def forest_tie_scene(dpi: int = 16, reverse=()) -> dict:
    """The lattice of bvh_scenes' ties with pairs of coincident objects of
    other compiled forms, pair k of kind FOREST_TIE_KINDS[k % 5], every second
    run of five in the other order.  The chain forms - the sphere under
    Translation [0, 0, 0] (tr), Rotation 0 (rot), Scaling [1, 1, 1] (sc), and
    Translation [0, 0, 0] over the far-sphere union of ties (tr_union) - give
    the same first-hit t as each other, so those pairs tie exactly and the
    reference's object order decides.  A chain against the bare sphere or the
    bare union, which do not normalise the ray's direction anew, is left out:
    their t differ in the last bits on about half the rays (5.417072566979102
    against ...124 on one), which any rounding of the ray turns over - a shift
    of the origin by 1e-7, or the second normalisation of rtamd.oracle_trace's
    camera - and where the two do tie the sphere wins in either order, so the
    pair says nothing about order.
    reverse: the pair kinds whose pairs stand in the other order."""
    objs = [_half([0, -1.4, 0], [0, 1, 0], _mat([0.5, 0.5, 0.5]))]
    for k in range(150):
        i, j = k % 15, k // 15
        c = [-3.5 + 0.5 * i, -1.0 + 0.3 * j, -2.5 - 0.5 * j]
        r = 0.18 + 0.04 * (k % 3)

        def bare(col):
            return {"sphere": {"position": list(c), "radius": r, "color": _mat(col)}}

        def wrapped(col, side):
            far = {"sphere": {"position": [c[0] + 40.0 * side, c[1] + 30.0, c[2] - 60.0], "radius": 0.01,
                              "color": _mat([0.5, 0.5, 0.5])}}
            return {"union": [bare(col), far]}

        red, green, blue, yellow = [1.0, 0.1, 0.1], [0.1, 1.0, 0.1], [0.1, 0.1, 1.0], [1.0, 1.0, 0.1]
        kind = FOREST_TIE_KINDS[k % 5]
        pair = {"tr/rot": lambda: [_tr([0, 0, 0], bare(red)), _rot(0, k % 3, bare(green))],
                "rot/sc": lambda: [_rot(0, k % 3, bare(green)), _sc([1, 1, 1], bare(blue))],
                "sc/tr": lambda: [_sc([1, 1, 1], bare(blue)), _tr([0, 0, 0], bare(yellow))],
                "rot/tr_union": lambda: [_rot(0, k % 3, bare(red)), _tr([0, 0, 0], wrapped(blue, -1))],
                "tr_union/tr": lambda: [_tr([0, 0, 0], wrapped(yellow, 1)), _tr([0, 0, 0], bare(blue))]}[kind]()
        if ((k // 5) % 2 == 1) != (kind in reverse):
            pair = pair[::-1]
        objs += pair
    return _base(objs, recursion=2, dpi=dpi, lights=copy.deepcopy(_FOREST_LIGHTS[:2]))


def forest_cases(dpi: int = 12) -> dict[str, dict]:
    """The named forest scenes, each the smallest that reaches its edge of the
    wave list (64 objects a chunk, 64 chunks a round of the device's chunk
    tests, a list only above 256 objects) or of the ray tree:
      mixed320    320 objects, one floor: six full chunks, no partial one
      partial330  330 objects, three floors: a partial last chunk, three
                  leading unbounded objects
      floors70    400 objects, 70 floors: two unbounded chunks
      bare257     257 objects, no unbounded one: the first chunk is all balls
      rounds8300  8300 objects, one floor, at two thirds of dpi (32 x 24 at
                  dpi 12): 131 chunks, three rounds of every chunk test
      eager301    299 objects, a floor and one eager object: no list, the
                  general kernels over 301 objects
      form_ties   forest_tie_scene
      concentric, collinear, far_clusters, giant_floor, nonfinite_bounds,
      zero_scale  300 small spheres over a floor, arranged as the name says or
                  standing beside such objects: one centre; one line; two
                  clusters 1e6 apart; a radius-1e6 sphere as floor; spheres
                  whose bounds overflow float (the centre, or only its
                  square) and an image that overflows double (a sphere whose
                  own bound overflows double answers every ray with a NaN hit
                  in the reference: no scene to compare on); Scalings by 0
                  and 1e-6 (never-hit objects and ones without a bound)
      seed/<s>    s in FOREST_SEEDS: forest_scene(s, n, u) with n drawn from
                  257..700 and u from {0, 1, 3}
    mixed320+sun is mixed320 with FOREST_SUN attached (forest_load)."""
    import random
    out = {"mixed320": forest_scene(11, 320, 1, dpi=dpi), "partial330": forest_scene(12, 330, 3, dpi=dpi),
           "floors70": forest_scene(13, 400, 70, dpi=dpi), "bare257": forest_scene(14, 257, 0, dpi=dpi),
           "rounds8300": forest_scene(15, 8300, 1, dpi=max(1, dpi * 2 // 3)),
           "eager301": forest_scene(16, 299, 1, eager=True, dpi=dpi), "form_ties": forest_tie_scene(dpi)}
    out["mixed320+sun"] = out["mixed320"]
    rnd = random.Random(17)
    floor = _half([0, -1.4, 0], [0, 1, 0], _mat([0.6, 0.6, 0.6]))

    def col(k):
        return _mat([(k % 7) / 7.0, (k % 5) / 5.0, (k % 3) / 3.0], shininess=8 + 4 * (k % 5))

    def small(k, p):
        return _sph(p, 0.05 + 0.02 * (k % 4), col(k))

    def cloud(k):
        return small(k, [rnd.uniform(-3.4, 3.4), rnd.uniform(-1.1, 1.4), rnd.uniform(-7.5, -1.5)])

    deg = {}
    deg["concentric"] = [floor] + [_sph([0.0, 0.2, -3.0], 0.9 - 0.002 * k, col(k)) for k in range(300)]
    deg["collinear"] = [floor] + [small(k, [-3.3 + 0.022 * k, -1.0 + 0.007 * k, -1.5 - 0.018 * k]) for k in range(300)]
    deg["far_clusters"] = [floor] + [cloud(k) for k in range(150)] + \
        [small(k, [1e6 + rnd.uniform(-3, 3), rnd.uniform(-1, 1), rnd.uniform(-7, -1)]) for k in range(150)]
    deg["giant_floor"] = [_sph([0.0, -1e6 - 1.4, 0.0], 1e6, _mat([0.6, 0.6, 0.6]))] + [cloud(k) for k in range(300)]
    deg["nonfinite_bounds"] = [floor] + [cloud(k) for k in range(300)] + [
        _sph([1e39, 2e39, -1e39], 1e38, col(1)),                      # no float holds the centre
        _sph([3e19, 1e19, -5e19], 1e19, col(2)),                      # ... nor its square
        _tr([2e38, 2e38, 0], _sph([2e38, 2e38, -3.0], 1e30, col(3))),   # the image's centre, not the subject's
        # an image beyond double: a Scaling by 1e6 or more carries no bound, the chain joins the unbounded lead
        _sc([1e200, 1e200, 1e200], _sph([1e150, 1e150, 0], 1e100, col(4)))]
    deg["zero_scale"] = [floor] + [cloud(k) for k in range(300)] + [
        _sc([0, 0, 0], small(1, [0.0, 0.5, -2.0])), _sc([1, 0, 1], small(2, [0.5, 0.5, -2.0])),
        _sc([1e-6, 1, 1], _sph([1e5, 0.3, -2.0], 0.5, col(3))),
        _sc([1e-6, 1e-6, 1e-6], _sph([-5e5, 4e5, -2.5e6], 3e5, col(4))),
        _tr([0.3, 0, 0], _sc([1, 1e-6, 1], _sph([0.0, 2e5, -3.0], 0.4, col(5))))]
    for name, objs in deg.items():
        out[name] = _base(objs, recursion=2, dpi=dpi, lights=copy.deepcopy(_FOREST_LIGHTS))
    for s in FOREST_SEEDS:
        rnd_s = random.Random(1000 + s)
        out[f"seed/{s}"] = forest_scene(s, rnd_s.randint(257, 700), rnd_s.choice([0, 1, 3]), dpi=dpi)
    return out


FOREST_TREELESS = ("eager301",)


def forest_load(rt, name: str, scene: dict):
    """forest_cases()[name] as a loaded scene: mixed320+sun gets its directional light (rt = the rtamd module)."""
    sc = rt.load_scene_from_json_text(json.dumps(scene))
    return rt.with_dir_lights(sc, [FOREST_SUN]) if name.endswith("+sun") else sc


# --------------------------------------------------- leaf-parameter scenes
# Edge values of the leaf primitives' own parameters; the reference's loader
# checks none of them (json_loader.cpp:211-297).
LEAF_HALF_NORMALS = ([0, 0, 0], [0, 1e-200, 0], [0, 1e200, 1e200], [0, 5e-324, 0], [0, 6e149, 8e149])
LEAF_BELT_HALF = (0, -0.1, 1.0, 2.0)
LEAF_BUTTON_OUTER = (0, -1, math.pi, 4.0)
LEAF_RING_WIDTH = (0, 1.0)
LEAF_BUTTON_DIR = ([0, 0, 0], [0, 0, 1e-7], [1e200, 0, 0])
LEAF_INDEX = (0, -1.5, 1e-300, 1e300)
LEAF_COEFF = ([-1, -0.5, -0.3], [2, 2, 2], [1, -1, 0])
LEAF_LAYOUT = {   # case -> layout: few (< 4 bounded objects), wave (>= 4), bvh (> 256 objects)
    "neg_radius_bare": "few", "neg_radius_bare_bvh": "bvh", "neg_radius_glass": "wave", "neg_radius_csg": "wave",
    "neg_radius_xform": "few", "radius_edges": "few", "radius_edges_wave": "wave", "radius_edges_bvh": "bvh",
    "huge_enclosing": "wave", "half_normals_few": "few", "half_normals": "wave", "poke_params_few": "few",
    "poke_params": "wave", "poke_params_bvh": "bvh", "index_edges": "wave", "index_huge": "wave",
    "index_medium0": "few", "coeff_edges": "wave", "neg_radius_eager": "wave"}
# the cases with an eager program (a transform inside a CSG operand): the general kernels
LEAF_EAGER_CASES = ("neg_radius_eager",)
# marker colours (diffuse) the CPU tests find a case's objects by
LEAF_NEG_COL, LEAF_ZERO_COL, LEAF_TINY_COL, LEAF_HUGE_COL = [0.9, 0.3, 0.2], [0.9, 0.1, 0.9], [0.1, 0.9, 0.9], [0.5, 0.6, 0.5]
LEAF_POKE_DIR = [0.2, 0.1, 1.0]


def _poke(c, r, **kw):
    p = {"position": [float(v) for v in c], "radius": r, "button_dir": list(LEAF_POKE_DIR)}
    p.update(kw)
    return {"pokeball": p}


def _leaf_extra(layout: str) -> list:
    """What a layout adds to a case's own objects: nothing (few), four
    ordinary spheres at the frame's corners (wave: the capsule and cone tests
    run), or the lattice of shading_layout("bvh") (the wave BVH)."""
    if layout == "few":
        return []
    if layout == "bvh":
        return shading_layout("bvh")[1:]
    return [_sph([-1.7, 1.1, -2.0], 0.3, _mat([0.3, 0.8, 0.3])),
            _sph([1.7, 1.1, -2.0], 0.3, _mat([0.2, 0.5, 0.8], reflected=[0.4, 0.4, 0.4])),
            _sph([-1.8, -0.8, -0.5], 0.3, _mat([0.8, 0.8, 0.2])),
            _sph([1.8, -0.8, -0.5], 0.3, _mat([0.7, 0.3, 0.7], refracted=[0.5, 0.5, 0.5]), index=1.5)]


def leaf_poke_variants() -> list[dict]:
    """The odd pokeball parameter sets of poke_params, one key each (the last: custom colours)."""
    out = [{"belt_half": v} for v in LEAF_BELT_HALF] + [{"button_outer": v} for v in LEAF_BUTTON_OUTER]
    out += [{"ring_width": v} for v in LEAF_RING_WIDTH]
    # (a button wide enough to be seen where the fallback direction +Y puts it)
    out += [{"button_dir": list(v), "button_outer": 0.9, "ring_width": 0.3} for v in LEAF_BUTTON_DIR]
    grey = _mat([0.4, 0.4, 0.4])
    out.append({"colors": {"top": _mat([0.9, 0.2, 0.2]), "bottom": _mat([0.9, 0.9, 0.9]), "ring": grey, "button": grey,
                           "belt": _mat([0.1, 0.1, 0.1], reflected=[0.5, 0.5, 0.5], refracted=[0.3, 0.3, 0.3])}})
    return out


def leaf_cases(dpi: int = 12) -> dict[str, dict]:
    """Hand-written scenes whose leaves carry parameters no other family has
    (tests/test_leaf_scenes.py, tests/test_gpu_leaves.py); the odd leaf is what
    the camera looks at, LEAF_LAYOUT names the layout around it:
      neg_radius_*   a sphere and a pokeball of negative radius ((p - c) / r
                     flips front_face, the pokeball's regions and eta): bare,
                     as glass at recursion 4, as left and right operand of
                     every operator (binary csg and n-ary), under a Scaling
                     and a Rotation
      radius_edges*  radius 0 and 1e-7 over a sphere of radius 1e6 as the floor
      huge_enclosing a sphere of radius 1e6 around the eye
      half_normals*  LEAF_HALF_NORMALS (zero and underflowing -> +Y,
                     overflowing -> n = 0: never hit, all of space as an
                     interval) bare, under a Translation and as CSG operands
      poke_params*   leaf_poke_variants()
      neg_radius_eager  negative-radius leaves as untransformed operands of
                     eager programs (the other operand under a transform):
                     sphere_interval / pick_region of the eager interpreter
      index_edges    index 0 and -1.5 on spheres with kt > 0; index_huge:
                     1e-300 and 1e300; index_medium0: medium.index 0.  The
                     last two at recursion 2: eta = 1e-300 or 0 sends the
                     refracted ray along -n through the centre, and whether
                     it leaves (eta = 1e300 or 1 / 0 times 1 - cos^2, which is
                     0 or an ulp) is decided by the origin's last bits - the
                     oracle alone was unstable on 28 of 33 such rays - so the
                     ray that enters is traced and its exit is not
      coeff_edges    reflected / refracted blocks LEAF_COEFF (kr, kt < 0, > 1, 0)"""
    sc = {}

    def put(name, objs, recursion=3, floor=True, index=1.0):
        d = _base(([_floor()] if floor else []) + objs + _leaf_extra(LEAF_LAYOUT[name]), recursion=recursion, dpi=dpi)
        d["medium"]["index"] = index
        sc[name] = d

    neg = _mat(LEAF_NEG_COL)
    bare = [_sph([-0.7, 0.1, -1.0], -0.55, neg), _poke([0.7, 0.1, -1.0], -0.55)]
    put("neg_radius_bare", bare)
    put("neg_radius_bare_bvh", bare)
    glass = _mat(LEAF_NEG_COL, reflected=[0.3, 0.3, 0.3], refracted=[0.5, 0.5, 0.5])
    put("neg_radius_glass", [
        _sph([-0.7, 0.1, -1.0], -0.55, glass, index=1.5),
        _poke([0.7, 0.1, -1.0], -0.55, colors={"top": dict(glass), "bottom": dict(glass)}),
        _sph([0.0, -0.7, -2.5], 0.5, _mat([0.2, 0.3, 0.9]))], recursion=4)
    objs = []
    for k, (op, side) in enumerate((o, s) for o in ("union", "intersection", "difference") for s in (0, 1)):
        for form in (0, 1):
            c = [-1.25 + 0.5 * k, -0.5 + 1.0 * form, -1.0]
            odd = _sph(c, -0.3, neg) if (k + form) % 2 else _poke(c, -0.3)
            other = _sph([c[0] + 0.12, c[1] + 0.1, c[2] + 0.15], 0.25, _mat([0.2, 0.4, 0.9]))
            third = _sph([c[0] - 0.05, c[1] - 0.12, c[2] + 0.1], 0.28, _mat([0.3, 0.8, 0.3]))
            if form == 0:
                a, b = (odd, other) if side == 0 else (other, odd)
                objs.append({"csg": {"operator": op, "left": a, "right": b}})
            else:
                objs.append({op: [odd, other, third] if side == 0 else [other, third, odd]})
    put("neg_radius_csg", objs)
    put("neg_radius_xform", [_sc([1.3, 0.7, 1.0], _sph([-0.6, 0.2, -1.0], -0.5, neg)),
                             _rot(30, 2, _poke([0.6, -0.3, -1.0], -0.5))])
    edges = [_sph([0, -1e6 - 1.2, 0], 1e6, _mat(LEAF_HUGE_COL)), _sph([0.0, 0.3, -1.0], 0.0, _mat(LEAF_ZERO_COL)),
             _sph([0.5, 0.2, -1.0], 1e-7, _mat(LEAF_TINY_COL))]
    put("radius_edges", edges, floor=False)
    put("radius_edges_wave", edges, floor=False)
    put("radius_edges_bvh", edges, floor=False)
    put("huge_enclosing", [_sph([0, 0, 0], 1e6, _mat([0.4, 0.5, 0.8])), _sph([0.0, 0.0, -1.5], 0.6, _mat(LEAF_NEG_COL))])
    # half-spaces: [0, 0, 0] is the floor, the translated [0, 1e-200, 0] a ceiling at y = 1.5
    hm = [_mat([0.5, 0.6, 0.5]), _mat([0.6, 0.5, 0.5]), _mat([0.9, 0.0, 0.9]), _mat([0.5, 0.5, 0.6]), _mat([0.6, 0.6, 0.4])]
    planes = []
    for k, n in enumerate(LEAF_HALF_NORMALS):
        y = [-1.2, -1.3, -1.0, -1.4, 0.0][k]
        planes.append({"halfSpace": {"position": [0, y, -6.0 if k == 4 else 0], "normal": list(n), "color": hm[k]}})
        up = [3.0, 2.7, 2.0, 3.2, 0.0][k]
        planes.append(_tr([0, up, -1.0 if k == 4 else 0],
                          {"halfSpace": {"position": [0, -1.2, -6.0 if k == 4 else 0], "normal": list(n), "color": hm[k]}}))
    put("half_normals_few", planes, floor=False)
    cut = []
    for k, n in enumerate(LEAF_HALF_NORMALS):
        c = [-1.2 + 0.6 * k, -0.4, -1.0]
        h = {"halfSpace": {"position": list(c), "normal": list(n), "color": _mat([0.9, 0.9, 0.1 * k])}}
        cut.append({"difference": [_sph(c, 0.28, _mat([0.2, 0.4, 0.9])), h]})
        c2 = [c[0], 0.5, -1.0]
        h2 = {"halfSpace": {"position": list(c2), "normal": list(n), "color": _mat([0.1 * k, 0.9, 0.9])}}
        cut.append({"csg": {"operator": "intersection", "left": h2, "right": _sph(c2, 0.28, _mat([0.9, 0.4, 0.2]))}})
    put("half_normals", planes + cut, floor=False)
    # (the button_dir variants in the bottom row: their +Y button is seen from above)
    balls = [_poke([-1.4 + 0.7 * (k % 5), 0.7 - 0.65 * (k // 5), -1.0], 0.3, **kw) for k, kw in enumerate(leaf_poke_variants())]
    put("poke_params_few", [balls[1], balls[7], balls[10]])
    put("poke_params", balls, recursion=2)
    put("poke_params_bvh", balls, recursion=2)
    tm = _mat([0.3, 0.5, 0.8], refracted=[0.6, 0.6, 0.6])
    put("index_edges", [_sph([-0.6 + 1.2 * k, 0.0, -1.0], 0.5, tm, index=v) for k, v in enumerate(LEAF_INDEX[:2])])
    put("index_huge", [_sph([-0.6 + 1.2 * k, 0.0, -1.0], 0.5, tm, index=v) for k, v in enumerate(LEAF_INDEX[2:])],
        recursion=2)
    put("index_medium0", [_sph([-0.6, 0.0, -1.0], 0.5, tm, index=1.5), _sph([0.6, 0.0, -1.0], 0.5, tm, index=0)],
        recursion=2, index=0)
    blue = _mat([0.2, 0.4, 0.9])
    put("neg_radius_eager", [
        {"union": [_sph([-1.0, 0.3, -1.0], -0.45, neg), _tr([-1.0, 0.0, 0.0], _sph([0.4, 0.0, -1.0], 0.3, blue))]},
        {"csg": {"operator": "difference", "left": _poke([0.1, 0.3, -1.0], -0.45),
                 "right": _rot(20, 1, _sph([0.5, 0.6, -0.7], 0.3, blue))}},
        {"intersection": [_sc([1.0, 1.2, 1.0], _sph([1.2, 0.25, -1.0], 0.5, blue)),
                          _sph([1.2, 0.3, -1.0], -0.45, glass, index=1.5)]}], recursion=4)
    put("coeff_edges", [_sph([-0.8 + 0.8 * k, 0.6, -1.0], 0.36, _mat([0.8, 0.5, 0.2], reflected=list(v)))
                        for k, v in enumerate(LEAF_COEFF)] +
                       [_sph([-0.8 + 0.8 * k, -0.4, -1.0], 0.36, _mat([0.2, 0.5, 0.8], refracted=list(v)), index=1.4)
                        for k, v in enumerate(LEAF_COEFF)])
    assert set(sc) == set(LEAF_LAYOUT)
    return sc


def leaf_scene(seed: int, dpi: int = 12) -> dict:
    """graph_scene(seed) with its leaves' parameters replaced, each with
    probability 1/3, by a draw from the edge lists above: a negated, zero or
    1e-7 radius, an odd pokeball parameter set, an odd sphere index, odd
    reflected / refracted blocks, an odd half-space normal."""
    import random
    rnd = random.Random(7919 * seed + 13)
    scene = graph_scene(seed, dpi=dpi)
    variants = leaf_poke_variants()[:-1]

    def walk(node, top):
        (kind, body), = node.items()
        if kind in ("sphere", "pokeball"):
            if rnd.random() < 1 / 3:
                body["radius"] = rnd.choice([-body["radius"], -body["radius"], 0.0, 1e-7])
            if kind == "pokeball" and rnd.random() < 1 / 3:
                body.update(copy.deepcopy(rnd.choice(variants)))
            if kind == "sphere":
                if rnd.random() < 1 / 3:
                    body["index"] = rnd.choice(LEAF_INDEX)
                if rnd.random() < 1 / 3:
                    body["color"][rnd.choice(["reflected", "refracted"])] = list(rnd.choice(LEAF_COEFF))
        elif kind == "halfSpace":
            # (the floor keeps its normal: the scene stays a scene over a floor)
            if not top and rnd.random() < 1 / 3:
                body["normal"] = list(rnd.choice(LEAF_HALF_NORMALS))
        elif kind == "csg":
            walk(body["left"], False)
            walk(body["right"], False)
        elif kind in ("union", "intersection", "difference"):
            for sub in body:
                walk(sub, False)
        else:
            walk(body["subject"], False)

    for obj in scene["objects"]:
        walk(obj, True)
    return scene


# ------------------------------------------- non-finite and overflowing rays
ODD_RAY_SCENES = ("config5", "torture/halfspace_in_csg", "bvh/ties", "leaf/radius_edges_wave")
ODD_RAY_N = 64


def odd_ray_scene(name: str) -> str:
    """JSON text of an ODD_RAY_SCENES entry (the first three as tests/test_gpu_query.py loads them)."""
    if name == "config5":
        return config_json(5, dpi=24)[0]
    if name.startswith("torture/"):
        return json.dumps(torture_scenes(dpi=24)[name[8:]])
    if name == "bvh/ties":
        return json.dumps(bvh_scenes(16)["ties"])
    return json.dumps(leaf_cases()[name[5:]])


def odd_ray_pixels(W: int, H: int) -> list:
    """The 64 pixels (an 8 x 8 grid) whose pixel-centre camera rays the groups are made from."""
    return [((2 * (k % 8) + 1) * W // 16, (2 * (k // 8) + 1) * H // 16) for k in range(ODD_RAY_N)]


def odd_ray_groups(o, d) -> dict:
    """Ray groups with non-finite or overflowing components, made from 64
    ordinary rays (o, d: (64, 3), d of unit length): tag -> (o, d, tmin,
    tmax).  Which component is odd rotates with the ray's index."""
    import numpy as np
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    n = len(o)
    assert o.shape == d.shape == (ODD_RAY_N, 3)
    nan, inf = float("nan"), float("inf")
    ax = np.arange(n) % 3
    rows = np.arange(n)

    def one(a, v):
        a = a.copy()
        a[rows, ax] = v
        return a

    def rng(tmin=1e-4, tmax=inf):
        return np.full(n, tmin), np.full(n, tmax)

    g = {}
    g["o one nan"] = (one(o, nan), d, *rng())
    g["o all nan"] = (np.full((n, 3), nan), d, *rng())
    g["o +inf"] = (one(o, inf), d, *rng())
    g["o -inf"] = (one(o, -inf), d, *rng())
    g["d one nan"] = (o, one(d, nan), *rng())
    g["d all nan"] = (o, np.full((n, 3), nan), *rng())
    g["d inf"] = (o, one(d, np.where(rows % 2 == 0, inf, -inf)), *rng())
    g["d 1e200"] = (o, d * 1e200, *rng())
    g["d 1e-200"] = (o, d * 1e-200, *rng())
    g["d subnormal"] = (o, d * 1e-310, *rng())
    # the `L > 1e-6` edge of Dir3::normalized from both sides: exactly 1e-6 long
    # (-> (0, 1, 0)), one ulp longer, and the ray's own direction 1e-6 (1 -+ 1e-9) long
    edge = d * 1e-6
    k = rows % 4
    edge[k == 0] = [0.0, 0.0, -1e-6]
    edge[k == 1] = [0.0, 0.0, -float(np.nextafter(1e-6, 1.0))]
    edge[k == 2] *= 1.0 - 1e-9
    edge[k == 3] *= 1.0 + 1e-9
    g["d 1e-6 long"] = (o, edge, *rng())
    g["tmin nan"] = (o, d, *rng(tmin=nan))
    g["tmin -inf"] = (o, d, *rng(tmin=-inf))
    g["tmin +inf"] = (o, d, *rng(tmin=inf))
    g["tmax nan"] = (o, d, *rng(tmax=nan))
    g["tmax -inf"] = (o, d, *rng(tmax=-inf))
    g["both nan"] = (o, d, *rng(nan, nan))
    return g


def odd_hit_groups(H, wo) -> dict:
    """Shading inputs with a NaN or an infinity in t, p, n or wo, made from
    ordinary hits H (an rt_hit record array) and view directions wo: tag ->
    (hits, wo).  Which component is odd rotates with the index."""
    import numpy as np
    H, wo = np.asarray(H).copy(), np.asarray(wo, dtype=np.float64).copy()
    ax, rows = np.arange(len(H)) % 3, np.arange(len(H))
    out = {}
    for f in ("t", "p", "n", "wo"):
        for tag, v in (("nan", float("nan")), ("+inf", float("inf")), ("-inf", -float("inf"))):
            h, w = H.copy(), wo.copy()
            if f == "t":
                h["t"] = v
            elif f == "wo":
                w[rows, ax] = v
            else:
                h[f][rows, ax] = v
            out[f"{f} {tag}"] = (h, w)
    h = H.copy()
    h["t"], h["p"], h["n"] = float("nan"), float("nan"), float("nan")
    out["all nan"] = (h, np.full_like(wo, float("nan")))
    # a finite wo whose specular power overflows (unit wo: r.wo <= 1)
    out["wo 1e200"] = (H.copy(), wo * 1e200)
    # and one whose power stays finite above 1 (r.wo up to 10: 1e5 at shininess 5, 1e64 at 64)
    out["wo x10"] = (H.copy(), wo * 10.0)
    return out


def zero_radius_centre_rays(centre) -> tuple:
    """64 axis-parallel rays aimed exactly through `centre` (the zero_radius
    sphere's): oc is a multiple of d, so disc == 0 exactly, the hit point is
    the centre and outward = 0 / 0.  (o, d, tmin, tmax)."""
    import numpy as np
    o, d = np.zeros((ODD_RAY_N, 3)), np.zeros((ODD_RAY_N, 3))
    for k in range(ODD_RAY_N):
        a, sgn = k % 3, 1.0 if (k // 3) % 2 == 0 else -1.0
        d[k, a] = sgn
        o[k] = centre
        o[k, a] -= sgn * (0.25 + 0.125 * (k // 6))
    return o, d, np.full(ODD_RAY_N, 1e-4), np.full(ODD_RAY_N, float("inf"))


# ------------------------------------------------------------ shading scenes
SHADING_LAYOUTS = ("few", "wave", "csg", "xform", "bvh")
SHADING_EXPONENTS = (0, 1, 2, 3, 5, 7, 127, 255, 1000, 1023, 1024, 2000, 12.5, 0.5, -2)
ONE_OF_65 = (0, 4, 5, 31, 32, 36, 37, 63, 64)
_FLOOR_Y = -1.2


def _sph(p, r, col, **kw):
    s = {"position": [float(v) for v in p], "radius": r, "color": col}
    s.update(kw)
    return {"sphere": s}


def _floor(y=_FLOOR_Y, **kw):
    return {"halfSpace": {"position": [0, y, 0], "normal": [0, 1, 0], "color": _mat([0.5, 0.6, 0.5], **kw)}}


def shading_layout(layout: str) -> list:
    """The object sets that decide which kernel's shade() runs (frame_plan.cpp
    pick_variant): few (< 4 bounded objects: no wave culls), wave (>= 4: wave
    culls, plain kernels), csg (+ a leaf-only CSG and a pokeball: non-plain),
    xform (+ a transform inside a CSG operand: eager, the D variant), bvh (a
    lattice of more than 256 spheres: the wave BVH)."""
    balls = [
        _sph([-1.3, -0.5, -1.0], 0.7, _mat([0.8, 0.3, 0.2])),
        _sph([0.9, -0.4, -1.6], 0.8, _mat([0.2, 0.5, 0.8], shininess=12)),
        _sph([-0.2, 0.7, -2.6], 0.6, _mat([0.3, 0.8, 0.3], reflected=[0.5, 0.5, 0.5])),
        _sph([1.7, 0.7, -0.8], 0.4, _mat([0.8, 0.8, 0.2], refracted=[0.6, 0.6, 0.6]), index=1.5),
        _sph([-1.7, 0.9, -1.8], 0.45, _mat([0.7, 0.3, 0.7], shininess=5)),
    ]
    if layout == "few":
        return [_floor()] + balls[:2]
    if layout == "wave":
        return [_floor()] + balls
    diff = {"difference": [_sph([0.0, -0.7, -0.1], 0.5, _mat([0.9, 0.6, 0.2])),
                           _sph([0.1, -0.5, 0.3], 0.35, _mat([0.2, 0.2, 0.9]))]}
    poke = {"pokeball": {"position": [-0.6, 1.5, -1.2], "radius": 0.35, "button_dir": [0.2, 0.1, 1.0]}}
    if layout == "csg":
        return [_floor()] + balls + [diff, poke]
    if layout == "xform":
        xf = {"union": [{"translation": {"factors": [0.9, 1.5, -1.4], "subject":
                                          _sph([0, 0, 0], 0.35, _mat([0.3, 0.7, 0.9]))}},
                        _sph([1.25, 1.7, -1.3], 0.25, _mat([0.9, 0.5, 0.1]))]}
        return [_floor()] + balls + [diff, poke, xf]
    if layout == "bvh":
        objs = [_floor()]
        for k in range(17 * 16):
            i, j = k % 17, k // 17
            m = _mat([(k % 7) / 7.0, (k % 5) / 5.0, (k % 3) / 3.0], shininess=8 + 4 * (k % 5))
            if k % 5 == 0:
                m["reflected"] = [0.4, 0.4, 0.4]
            elif k % 7 == 0:
                m["refracted"] = [0.5, 0.5, 0.5]
            objs.append(_sph([-2.4 + 0.3 * i, -1.0 + 0.05 * (i % 3), -1.0 - 0.3 * j], 0.1 + 0.03 * ((i + j) % 3), m,
                             index=1.5))
        return objs
    raise KeyError(layout)


def ring_lights(n: int) -> list:
    """n dim point lights on a golden-angle spiral above and around the layouts."""
    out = []
    for l in range(n):
        a = 2.399963 * l
        R = 2.0 + 3.0 * ((l * 5) % n) / n
        out.append({"position": [R * math.cos(a), 4.0 + 2.0 * ((l * 7) % n) / n, -1.2 + R * math.sin(a)],
                    "intensity": [0.35 + 0.25 * ((l * 3) % 7) / 6.0, 0.35 + 0.25 * ((l * 5) % 7) / 6.0,
                                  0.35 + 0.25 * (l % 7) / 6.0]})
    return out


def _window(scene, points, size, dpi):
    """Narrow the screen to a size[0] x size[1] window (in screen-plane units)
    centred on the projection of `points` through the observer."""
    scr = scene["screen"]
    eye, z0 = scr["observer"], scr["position"][2]
    px = []
    for p in points:
        f = (z0 - eye[2]) / (p[2] - eye[2])
        px.append((eye[0] + (p[0] - eye[0]) * f, eye[1] + (p[1] - eye[1]) * f))
    cx = sum(x for x, _ in px) / len(px)
    cy = sum(y for _, y in px) / len(px)
    # centre snapped to the pixel grid, so that width and height stay exact
    cx, cy = round(cx * dpi) / dpi, round(cy * dpi) / dpi
    scr["dpi"] = dpi
    scr["dimensions"] = [size[0], size[1]]
    scr["position"] = [cx - size[0] / 2.0, cy - size[1] / 2.0, z0]
    return scene


def shading_scenes(dpi: int = 24, detail: float = 1.0) -> dict[str, dict]:
    """Shading and recursion inputs no other scene family has (shade() and the
    trace loops of rt_device.hpp; shading.cpp:31-138, tracer.cpp:22-104), as
    "<case>_<layout>" -> scene, over the layouts of shading_layout():
      lights33/64/65  more point lights than one 32-light round of shade(), at
                      the round edges
      one65_kNN       the 65-light scene, every intensity 0 but light NN's
      near_light      a light 0.05 above the floor (dist_squared <= 0.01), one
                      0.3 off a sphere (max(0.5, distance)), one ordinary,
                      on a screen narrowed around the two
      far_skip        hits at t ~ 2000 (shadow_epsilon ~ 0.2) with lights 0.25
                      off the surface: max_shadow_t <= shadow_epsilon
      exponents       one sphere per shininess of SHADING_EXPONENTS (integers
                      up to 1023, 1024, 2000, 12.5, 0.5, -2: pow(0, -2) = inf)
      extremes        a light that saturates the 1.5 clamp, a negative
                      intensity, albedo > 1, ks = 0, zero ambient, kd = 0
      media           medium.index 1.33 around spheres of index 1.5, 1.33,
                      1.0, one with kr and kt, one refractive CSG operand
      null_mat        spheres without a material, bare and as a CSG operand
    dpi scales every frame (24: at most 128 x 96 pixels, 256 x 192 for
    exponents); detail scales the extra pixel density of the cases on a
    narrowed screen (near_light, far_skip, exponents), which the tests need to
    count branch hits and the fixtures do not.  Materials and nodes the JSON schema cannot spell are listed
    by shading_patches() and applied by shading_load()."""
    sc = {}

    def put(name, objs, lights, recursion=3, scr_dpi=dpi):
        sc[name] = _base(copy.deepcopy(objs), recursion=recursion, dpi=scr_dpi, lights=copy.deepcopy(lights))
        return sc[name]

    # ---- many lights
    for n in (33, 64, 65):
        for lay in SHADING_LAYOUTS:
            if lay == "bvh" and n != 33:
                continue
            put(f"lights{n}_{lay}", shading_layout(lay), ring_lights(n))
    for lay in ("wave", "csg"):
        for k in ONE_OF_65:
            lights = ring_lights(65)
            for i, L in enumerate(lights):
                if i != k:
                    L["intensity"] = [0, 0, 0]
            put(f"one65_k{k:02d}_{lay}", shading_layout(lay), lights, scr_dpi=max(1, dpi // 2))

    # ---- near lights: A just above the floor, B 0.3 off a sphere's surface
    ordinary = {"position": [3, 5, 4], "intensity": [12, 12, 12]}
    for lay in ("few", "wave", "bvh"):
        objs = shading_layout(lay)
        s0 = objs[1]["sphere"]
        c, r = s0["position"], s0["radius"]
        u = [0.3, 0.3, 1.0]
        un = math.sqrt(sum(v * v for v in u))
        u = [v / un for v in u]
        B = [c[i] + (r + 0.3) * u[i] for i in range(3)]
        cap = [c[i] + r * u[i] for i in range(3)]
        A = [cap[0] + 0.25, _FLOOR_Y + 0.05, cap[2] + 0.8]
        lights = [{"position": A, "intensity": [0.02, 0.02, 0.015]}, {"position": B, "intensity": [0.2, 0.15, 0.2]},
                  ordinary]
        s = put(f"near_light_{lay}", objs, lights)
        size = (1.2, 1.2) if lay != "bvh" else (0.6, 0.6)
        px = int(detail * ((dpi * 10) // 3 if lay != "bvh" else (dpi * 20) // 3))
        _window(s, [A, cap], size, px)

    # ---- lights inside the shadow epsilon of a far hit
    for lay in ("few", "wave"):
        big = _sph([0, 0, -2100], 100.0, _mat([0.7, 0.6, 0.5]))
        small = [_sph([1.5, 1.0, -1996.0], 0.5, _mat([0.2, 0.5, 0.9])),
                 _sph([-2.0, 1.5, -1997.0], 0.6, _mat([0.9, 0.5, 0.2])),
                 _sph([-1.0, -2.0, -1995.0], 0.4, _mat([0.3, 0.8, 0.3])),
                 _sph([2.5, -1.5, -1998.0], 0.7, _mat([0.8, 0.3, 0.7]))]
        objs = [_floor(-120.0), big] + (small[:1] if lay == "few" else small)
        lights = []
        for (x, y) in ((0.0, 0.0), (1.2, -0.6)):
            z = math.sqrt(100.0 ** 2 - x * x - y * y)
            nrm = [x / 100.0, y / 100.0, z / 100.0]
            lights.append({"position": [x + 0.25 * nrm[0], y + 0.25 * nrm[1], -2100 + z + 0.25 * nrm[2]],
                           "intensity": [0.05, 0.04, 0.03]})
        lights.append({"position": [30, 40, -1950], "intensity": [600, 600, 500]})
        s = put(f"far_skip_{lay}", objs, lights, recursion=1)
        s["screen"] = {"dpi": int(detail * dpi * 200), "dimensions": [0.02, 0.015], "position": [-0.01 + 0.000003, -0.0075 - 0.0000015, 0],
                       "observer": [0, 0, 5]}

    # ---- specular exponents
    def expo_sphere(k):
        i, j = k % 5, k // 5
        ks = 0.4 + 0.5 * ((k * 4) % 15) / 14.0
        return _sph([-1.6 + 0.8 * i, 1.2 - 0.9 * j, 0.0], 0.38,
                    _mat([0.3 + 0.1 * (k % 5), 0.25, 0.7 - 0.1 * (k % 4)], specular=[ks, ks, ks],
                         shininess=SHADING_EXPONENTS[k]))
    expo_lights = [{"position": [0.6, 1.2, 6.0], "intensity": [30, 30, 30]},
                   {"position": [-2.5, 3.0, 5.0], "intensity": [20, 25, 30]}]
    expo_dpi = int(detail * ((dpi * 8) // 3))
    s = put("exponents_wave", [_floor(-1.5)] + [expo_sphere(k) for k in range(15)], expo_lights, scr_dpi=expo_dpi)
    s["screen"]["position"] = [-2, -1.2, 0]
    for i in range(5):   # fewer than 4 bounded objects: one column of three at a time
        s = put(f"exponents_few{i}", [_floor(-1.5)] + [expo_sphere(i + 5 * j) for j in range(3)], expo_lights,
                scr_dpi=expo_dpi)
        s["screen"]["dimensions"] = [0.75, 3]
        s["screen"]["position"] = [-1.6 + 0.8 * i - 0.375, -1.2, 0]

    # ---- extreme intensities and coefficients
    for lay in ("few", "csg"):
        objs = shading_layout(lay)
        objs[0] = _floor(ambient=[0, 0, 0])
        objs[1]["sphere"]["color"] = {"diffuse": [1.5, 1.2, 2.0], "ambient": [0, 0, 0], "shininess": 6}   # ks = 0
        objs[2]["sphere"]["color"] = _mat([0.6, 0.7, 0.2], specular=[0.9, 0.9, 0.9], shininess=3)         # kd -> 0
        lights = [{"position": [1.0, 1.5, 1.0], "intensity": [60, 50, 40]},
                  {"position": [-3, 4, 2], "intensity": [-4, 6, -1]},
                  {"position": [2, 5, -4], "intensity": [5, 5, 5]}]
        put(f"extremes_{lay}", objs, lights)

    # ---- a medium that is not vacuum
    tir = _sph([-1.2, -0.3, -1.0], 0.8, _mat([0.2, 0.2, 0.3], refracted=[0.8, 0.8, 0.8]), index=1.0)
    same = _sph([0.6, -0.5, -0.6], 0.6, _mat([0.3, 0.2, 0.2], refracted=[0.7, 0.7, 0.7]), index=1.33)
    both = _sph([0.3, 0.9, -2.2], 0.7, _mat([0.2, 0.3, 0.2], refracted=[0.5, 0.5, 0.5], reflected=[0.4, 0.4, 0.4]),
                index=1.5)
    glass = _sph([1.7, 0.2, -1.5], 0.5, _mat([0.1, 0.1, 0.1], refracted=[0.9, 0.9, 0.9]), index=1.5)
    mirror = _sph([-1.6, 1.1, -2.4], 0.5, _mat([0.2, 0.2, 0.2], reflected=[0.8, 0.8, 0.8]))
    lens = {"difference": [_sph([1.5, -0.7, 0.2], 0.45, _mat([0.2, 0.2, 0.4], refracted=[0.8, 0.8, 0.8]), index=1.5),
                           _sph([1.5, -0.5, 0.6], 0.3, _mat([0.9, 0.3, 0.3]))]}
    media = {"few": [_floor(), tir, same, both], "wave": [_floor(), tir, same, both, glass, mirror],
             "csg": [_floor(), tir, same, both, glass, mirror, lens]}
    for name, lay, rec in (("media_few", "few", 4), ("media_wave", "wave", 4), ("media_csg", "csg", 4),
                           ("media_few_rec2", "few", 2), ("media_few_rec1", "few", 1)):
        put(name, media[lay], None, recursion=rec)["medium"]["index"] = 1.33

    # ---- null materials (shading_patches: the spheres at NULL_CENTRES)
    n0 = _sph(NULL_CENTRES[0], 0.7, _mat([0.5, 0.5, 0.5]))
    shiny = _sph([0.9, -0.4, -1.6], 0.8, _mat([0.2, 0.3, 0.4], reflected=[0.7, 0.7, 0.7]))
    put("null_mat_few", [_floor(), n0, shiny], None)
    left = {"union": [_sph(NULL_CENTRES[1], 0.5, _mat([0.5, 0.5, 0.5])),
                      _sph([-0.1, 0.85, -2.0], 0.5, _mat([0.3, 0.8, 0.3]))]}
    right = {"union": [_sph([1.3, 0.9, -1.2], 0.45, _mat([0.8, 0.8, 0.2])),
                       _sph(NULL_CENTRES[2], 0.45, _mat([0.5, 0.5, 0.5]))]}
    glass2 = _sph([0.0, -0.7, 0.2], 0.4, _mat([0.1, 0.1, 0.1], refracted=[0.9, 0.9, 0.9]), index=1.5)
    poke = {"pokeball": {"position": [-1.7, 1.2, -1.0], "radius": 0.35, "button_dir": [0.2, 0.1, 1.0]}}
    put("null_mat_csg", [_floor(), n0, shiny, left, right, glass2, poke], None)
    return sc


NULL_CENTRES = ([-1.3, -0.5, -1.0], [-0.6, 0.8, -2.0], [1.8, 0.9, -1.2])


def shading_patches(name: str) -> dict:
    """What shading_scenes()[name] needs beyond its JSON: "null" the centres of
    the spheres that lose their material (rt_node.mat = -1), "kd0" the centres
    of the spheres whose material gets kd = 0."""
    if name == "null_mat_few":
        return {"null": [NULL_CENTRES[0]], "kd0": []}
    if name == "null_mat_csg":
        return {"null": list(NULL_CENTRES), "kd0": []}
    if name.startswith("extremes_"):
        return {"null": [], "kd0": [[0.9, -0.4, -1.6]]}
    return {"null": [], "kd0": []}


def shading_patch_indices(rt, sc, name: str) -> tuple[list, list]:
    """shading_patches(name) as (null node indices, kd = 0 material indices) of the loaded scene."""
    p = shading_patches(name)
    null_nodes = rt.sphere_nodes_at(sc, p["null"])
    kd0 = [int(sc.desc.nodes[i].mat) for i in rt.sphere_nodes_at(sc, p["kd0"])]
    return null_nodes, kd0


def shading_apply(rt, sc, null_nodes, kd0_mats):
    if len(kd0_mats):
        sc = rt.with_material_fields(sc, {int(m): {"kd": 0.0} for m in kd0_mats})
    if len(null_nodes):
        sc = rt.with_null_materials(sc, null_nodes)
    return sc


def shading_load(rt, name: str, scene: dict):
    """shading_scenes()[name] as a loaded scene (rt = the rtamd module)."""
    sc = rt.load_scene_from_json_text(json.dumps(scene))
    return shading_apply(rt, sc, *shading_patch_indices(rt, sc, name))


def shading_light_branches(rt, sc, with_shadows: bool = False) -> list[dict]:
    """Which branches of the point-light loop (shading.cpp:79-104) the frame's
    pixel-centre primary hits reach, per light, computed from the oracle's hits
    alone (rt.oracle_primary_hits): counts of hits that face the light
    (n . wi > 0) and have
      clamped   dist_squared <= 0.01
      half      a clamped distance below 0.5 (effective_dist = 0.5)
      skipped   max_shadow_t <= shadow_epsilon
      queried   a shadow query
      lit       (with_shadows) a shadow query that finds nothing."""
    import numpy as np

    rec = rt.oracle_primary_hits(sc)
    h = rec[rec["hit"] & (rec["mat"] >= 0)]
    eps = np.maximum(1e-3, 1e-4 * h["t"])
    d = sc.desc
    out = []
    for li in range(d.n_lights):
        tl = np.array(d.lights[li].pos[:]) - h["p"]
        d2 = (tl * tl).sum(1)
        clamped = d2 <= 0.01
        dist = np.sqrt(np.where(clamped, 0.01, d2))
        wi = tl / dist[:, None]
        facing = (h["n"] * wi).sum(1) > 0.0
        skipped = facing & (dist - eps <= eps)
        queried = facing & ~skipped
        b = {"clamped": int((facing & clamped).sum()), "half": int((facing & (dist < 0.5)).sum()),
             "skipped": int(skipped.sum()), "queried": int(queried.sum())}
        if with_shadows:
            q = np.flatnonzero(queried)
            so = h["p"][q] + h["n"][q] * eps[q, None]
            occ = rt.oracle_occluded(sc, so, wi[q], eps[q], dist[q] - eps[q])
            b["lit"] = int((~occ).sum())
        out.append(b)
    return out


def deep_recursion_scene(recursion: int, dpi: int = 8) -> dict:
    """deep_scenes()["mirrors_rec24"] at another medium.recursion, its opaque
    sphere given kr and kt > 0 so that both child slots of a frame are used at
    the deepest level (the stack tiers of rt_launch.hpp: kMaxDepth = 16 frames,
    kBigDepth = 128)."""
    s = deep_scenes(dpi=dpi)["mirrors_rec24"]
    col = s["objects"][2]["sphere"]["color"]
    col["reflected"] = [0.3, 0.3, 0.3]
    col["refracted"] = [0.5, 0.5, 0.5]
    s["objects"][2]["sphere"]["index"] = 1.3
    s["medium"]["recursion"] = recursion
    return s


# ------------------------------------------------------------ placed scenes
# name -> (scale, offset): where the culling tests put a scene (placed()).
# Frames stop at x24 (dpi is an integer: 24 -> 1); queries have no camera and
# carry the large scales.  e25: the f32 squares of the coordinates overflow
# while the coordinates are finite; e39: the f32 copies themselves are inf.
PLACEMENTS = {
    "mid": (1.0, (3000.7, -2000.3, 1000.1)),
    "far": (1.0, (1e6 + 0.3, -7.5e5 - 0.7, 5e5 + 0.1)),
    "x24": (24.0, (0.0, 0.0, 0.0)),
    "x24_far": (24.0, (7.2e4 + 0.3, -4.8e4 - 0.7, 2.4e4 + 0.1)),
    "d100_mid": (0.01, (30.007, -20.003, 10.001)),
    "big": (1000.0, (0.0, 0.0, 0.0)),
    "huge_far": (1e5, (3e8 + 0.3, -2e8, 1e8)),
    "tiny": (1e-3, (0.0, 0.0, 0.0)),
    "e25": (1e25, (0.0, 0.0, 0.0)),
    "e39": (1e39, (0.0, 0.0, 0.0)),
}
FRAME_PLACEMENTS = ("mid", "far", "x24", "x24_far", "d100_mid")
QUERY_PLACEMENTS = ("mid", "far", "big", "huge_far", "tiny", "e25", "e39")


def placed(scene: dict, scale: float, offset) -> dict:
    """The JSON scene under the similarity x -> scale * x + offset, as a deep
    copy: positions mapped, lengths (radii, translation factors, the screen's
    dimensions) x scale, dpi / scale (an integer >= 1, so that a frame keeps
    its W x H; ValueError otherwise), light intensities x scale^2 (the falloff
    is 1 / d^2).  Normals, angles, button directions, materials, the medium
    and the background stay.  scaling and rotation nodes act about the origin
    and do not commute with an offset: with a non-zero offset they become
    translation(+offset) o node o translation(-offset) o placed subject.  A
    key this function does not know raises KeyError."""
    scale = float(scale)
    off = [float(v) for v in offset]
    if len(off) != 3:
        raise ValueError("offset must have three components")
    moved = any(v != 0.0 for v in off)

    def point(p):
        return [scale * float(p[i]) + off[i] for i in range(3)]

    def node(nd):
        (kind, body), = nd.items()
        if kind in ("union", "intersection", "difference"):
            return {kind: [node(c) for c in body]}
        out = copy.deepcopy(body)
        if kind == "sphere":
            _known(body, ("position", "radius", "color", "index"), kind)
            out["position"], out["radius"] = point(body["position"]), scale * body["radius"]
        elif kind == "pokeball":
            _known(body, ("position", "radius", "button_dir", "belt_half", "button_outer", "ring_width", "colors"),
                   kind)
            out["position"], out["radius"] = point(body["position"]), scale * body["radius"]
        elif kind == "halfSpace":
            _known(body, ("position", "normal", "color", "index"), kind)
            out["position"] = point(body["position"])
        elif kind == "translation":
            _known(body, ("factors", "subject"), kind)
            out["factors"] = [scale * float(v) for v in body["factors"]]
            out["subject"] = node(body["subject"])
        elif kind in ("scaling", "rotation"):
            _known(body, ("factors", "subject") if kind == "scaling" else ("angle", "direction", "subject"), kind)
            out["subject"] = node(body["subject"])
            if moved:
                out["subject"] = {"translation": {"factors": [-v for v in off], "subject": out["subject"]}}
                return {"translation": {"factors": list(off), "subject": {kind: out}}}
        elif kind == "csg":
            _known(body, ("operator", "left", "right"), kind)
            out["left"], out["right"] = node(body["left"]), node(body["right"])
        else:
            raise KeyError(kind)
        return {kind: out}

    s = {}
    for key, val in scene.items():
        if key == "screen":
            _known(val, ("dpi", "dimensions", "position", "observer"), key)
            scr = copy.deepcopy(val)
            dpi = val["dpi"] / scale
            if dpi < 1 or dpi != int(dpi):
                raise ValueError(f"dpi {val['dpi']} / scale {scale} is no integer >= 1")
            scr["dpi"] = int(dpi)
            scr["position"], scr["observer"] = point(val["position"]), point(val["observer"])
            if "dimensions" in val:
                scr["dimensions"] = [scale * float(v) for v in val["dimensions"]]
            s[key] = scr
        elif key == "sources":
            s[key] = []
            for L in val:
                _known(L, ("position", "intensity"), key)
                s[key].append({"position": point(L["position"]),
                               "intensity": [scale * scale * float(v) for v in L["intensity"]]})
        elif key == "objects":
            s[key] = [node(o) for o in val]
        elif key in ("medium", "background"):
            s[key] = copy.deepcopy(val)
        else:
            raise KeyError(key)
    return s


def _known(body: dict, keys, where: str) -> None:
    for k in body:
        if k not in keys:
            raise KeyError(f"{where}.{k}")


# ------------------------------------------------------------ kernel recipes
# rt_flags (include/rt.h)
_COUNT, _NO_CULL, _FP32, _NO_BVH, _FORCE_BVH = 1, 2, 4, 8, 16


class Recipe(NamedTuple):
    """How to launch one row of a launch table (kernel_recipes)."""
    row: str              # "ns::kernel<...>", the table row's own name
    scene_name: str       # key of recipe_scene()
    mode: int             # 0 standard, 1 paper (query rows: 0)
    flags: int
    frame: int            # 0-based frame of one Tracer on a fresh scene handle that must launch the row
    world: int = 1        # > 1: a distributed frame of that many simulated ranks (the CODES finish kernels)
    query: int = -1       # 0 / 1: the row is the closest-hit / any-hit query kernel


def recipe_scene(name: str) -> tuple[str, list | None]:
    """(JSON text, directional lights or None) of a recipe's scene: the
    existing families at 64x48 (deep scenes 48x36), "<scene>@WxH" the same
    screen centre at another size.  The shading scenes used here need no
    shading_patches()."""
    base, _, size = name.partition("@")
    fam, _, key = base.partition("/")
    lights = None
    if fam == "cfg":
        s = json.loads(config_json(int(key), dpi=16)[0])
    elif fam == "torture":
        s = torture_scenes(dpi=16)[key]
    elif fam == "bvh":
        s = bvh_perf_scene(300, dpi=16) if key == "perf300" else bvh_scenes(16)[key]
    elif fam == "deep":
        s = deep_scenes()[key]
    elif fam == "dir":
        text, lights = dir_light_cases()[key]
        s = json.loads(text)
    elif fam == "shading":
        s = shading_scenes(dpi=16)[key]
    # the scenes of tests/test_gpu_query.py, for the query rows
    elif fam == "query":
        if key.startswith("torture/"):
            s = torture_scenes(dpi=24)[key[8:]]
        elif key.startswith("config"):
            s = json.loads(config_json(int(key[6:]), dpi=24)[0])
        else:
            return recipe_scene(key)
    else:
        raise KeyError(name)
    if size:
        w, h = (int(v) for v in size.split("x"))
        s = with_size(s, w, h)
    return json.dumps(s), lights


def kernel_recipes() -> list[Recipe]:
    """One Recipe per row of every launch table (rt_test.h rt_test_kernel_row):
    the smallest scene of the existing families whose frame launches the row.
    Wave-BVH rows (WV = 2) force the BVH and their WV = 1 twins switch it off,
    so that no BVH trial frame decides the kernel; the untimed paper kernels
    are the second frame of a scene handle, the timed ones (T = true) the first.
    tests/test_kernel_table.py holds this list against the tables,
    tests/test_gpu_kernel_table.py renders every entry."""
    C, F, NB, FB = _COUNT, _FP32, _NO_BVH, _FORCE_BVH
    out = []

    def add(row, scene, mode, flags=0, frame=0, **kw):
        out.append(Recipe(row, scene, mode, flags, frame, **kw))

    b = lambda v: "true" if v else "false"   # noqa: E731

    # the common kernels in both precisions (rtf: no plain rows)
    for ns, f in (("rtd", 0), ("rtf", F)):
        # the wave-BVH lattice: FP64 with exact closest-hit ties, FP32 without
        # (bvh_scenes: whole spheres of ties change colour when FP32 rounding
        # breaks a tie, which the silhouette bars of the FP32 path do not cover)
        lean, secw = ("bvh/nested", "bvh/nested_mirror") if f else ("bvh/ties", "bvh/ties_mirror")
        # ---- standard mode: k_std<E, D, SEC, C, false>
        for e, d, sec, scene in ((1, 1, 0, "torture/xform_in_csg"), (1, 1, 1, "shading/lights33_xform"),
                                 (0, 1, 0, "dir/cfg2_sun_back"), (0, 1, 1, "dir/reflect_refract_sun"),
                                 (0, 0, 1, "shading/media_few")):
            for c in (0, 1):
                add(f"{ns}::k_std<{b(e)}, {b(d)}, {b(sec)}, {b(c)}, false>", scene, 0, f | (C if c else 0))
        # k_std_lean<C, WV, PL>, k_std_secw<C, WV, PL>
        for c in (0, 1):
            fc = f | (C if c else 0)
            add(f"{ns}::k_std_lean<{b(c)}, 0, false>", "cfg/2" if (c or f) else "torture/csg_groups", 0, fc)
            add(f"{ns}::k_std_lean<{b(c)}, 1, false>", lean, 0, fc | NB)
            add(f"{ns}::k_std_lean<{b(c)}, 2, false>", lean, 0, fc | FB)
            add(f"{ns}::k_std_secw<{b(c)}, 1, false>", secw, 0, fc | NB)
            add(f"{ns}::k_std_secw<{b(c)}, 2, false>", secw, 0, fc | FB)
        # ---- paper mode: k_paper_primary<E, D, C[, T]>: untimed on the second frame, timed on the first
        for e, d, scene in ((1, 1, "torture/xform_in_csg"), (0, 1, "dir/cfg2_sun_back")):
            add(f"{ns}::k_paper_primary<{b(e)}, {b(d)}, false>", scene, 1, f, 1)
            add(f"{ns}::k_paper_primary<{b(e)}, {b(d)}, false, true>", scene, 1, f, 0)
            add(f"{ns}::k_paper_primary<{b(e)}, {b(d)}, true>", scene, 1, f | C, 0)
        # k_paper_primary_lean<C, WV, T, PL>
        for wv, scene, fl in ((0, "cfg/2" if f else "torture/csg_groups", 0), (1, lean, NB), (2, lean, FB)):
            add(f"{ns}::k_paper_primary_lean<false, {wv}, false, false>", scene, 1, f | fl, 1)
            add(f"{ns}::k_paper_primary_lean<false, {wv}, true, false>", scene, 1, f | fl, 0)
            add(f"{ns}::k_paper_primary_lean<true, {wv}, false, false>", "cfg/2" if wv == 0 else scene, 1, f | fl | C, 0)
    # ---- the plain kernels (FP64 only, never counting)
    for wv, scene, fl in ((0, "cfg/2", 0), (1, "bvh/perf300", NB), (2, "bvh/perf300", FB)):
        add(f"rtd::k_std_lean<false, {wv}, true>", scene, 0, fl)
        add(f"rtd::k_paper_primary_lean<false, {wv}, false, true>", scene, 1, fl, 1)
        add(f"rtd::k_paper_primary_lean<false, {wv}, true, true>", scene, 1, fl, 0)
    add("rtd::k_std_secw<false, 1, true>", "bvh/grid", 0, NB)
    add("rtd::k_std_secw<false, 2, true>", "bvh/grid", 0, FB)
    # ---- the big-stack build: general rows only
    for sec, scene in ((0, "deep/xform_nest12"), (1, "deep/mirrors_rec24")):
        for c in (0, 1):
            add(f"rtdb::k_std<true, true, {b(sec)}, {b(c)}, false>", scene, 0, C if c else 0)
    add("rtdb::k_paper_primary<true, true, false>", "deep/xform_nest12", 1, 0, 1)
    add("rtdb::k_paper_primary<true, true, false, true>", "deep/xform_nest12", 1, 0, 0)
    add("rtdb::k_paper_primary<true, true, true>", "deep/xform_nest12", 1, C, 0)
    # ---- ray queries: k_query_isect / k_query_occl<E, D, PL>
    for ns, e, d, pl, scene in (("rtd", 1, 1, 0, "query/torture/xform_in_csg"), ("rtd", 0, 1, 0, "query/dir/pokeball_csg_sun"),
                                ("rtd", 0, 0, 0, "query/bvh/ties"), ("rtd", 0, 0, 1, "query/config3"),
                                ("rtdb", 1, 1, 0, "query/deep/xform_nest12")):
        for kind, k in enumerate(("k_query_isect", "k_query_occl")):
            add(f"{ns}::{k}<{b(e)}, {b(d)}, {b(pl)}>", scene, 0, 0, 0, query=kind)
    # ---- the finish pass: k_paper_finish<CODES, PAIR>.  PAIR by the width's
    # parity; CODES in the ranks of a distributed FP64 frame (taller than one
    # RT_PAPER_STRIP_ROWS strip, so that both ranks render)
    add("rtd::k_paper_finish<false, false>", "cfg/5@51x36", 1)
    add("rtd::k_paper_finish<false, true>", "cfg/5@52x36", 1)
    add("rtd::k_paper_finish<true, false>", "cfg/5@17x48", 1, world=2)
    add("rtd::k_paper_finish<true, true>", "cfg/5@16x48", 1, world=2)
    add("rtf::k_paper_finish<false, false>", "cfg/5@51x36", 1, F)
    add("rtf::k_paper_finish<false, true>", "cfg/5@52x36", 1, F)
    return out


def radiance_recipes() -> list[Recipe]:
    """One Recipe (row, scene name, flags; mode, frame unused) per row of the
    radiance launch tables (rt_test.h rt_test_radiance_kernel_row):
    k_radiance<E, D, SEC, PL>.  The SEC rows' scenes reflect or refract, so a
    bounce really runs.  tests/test_radiance_plan.py holds this list against
    the tables, tests/test_gpu_radiance.py queries every entry."""
    out = []
    b = lambda v: "true" if v else "false"   # noqa: E731
    for ns, e, d, sec, pl, scene in (("rtd", 1, 1, 1, 0, "shading/lights33_xform"),
                                     ("rtd", 0, 1, 1, 0, "dir/reflect_refract_sun"),
                                     ("rtd", 0, 1, 0, 0, "dir/cfg2_sun_back"),
                                     ("rtd", 0, 0, 1, 0, "torture/reflect_refract"),
                                     ("rtd", 0, 0, 0, 0, "cfg/4"),
                                     ("rtd", 0, 0, 1, 1, "cfg/5"),
                                     ("rtd", 0, 0, 0, 1, "cfg/3"),
                                     ("rtdb", 1, 1, 1, 0, "deep/mirrors_rec24")):
        out.append(Recipe(f"{ns}::k_radiance<{b(e)}, {b(d)}, {b(sec)}, {b(pl)}>", scene, 0, 0, 0))
    return out


def shade_recipes() -> list[Recipe]:
    """One Recipe (row, scene name, flags; mode, frame unused) per row of the
    shade launch tables (rt_test.h rt_test_shade_kernel_row): k_shade<E, D,
    PL>, the occluded query's columns, so the query rows' scenes fit.
    tests/test_shade_plan.py holds this list against the tables,
    tests/test_gpu_shade.py queries every entry."""
    out = []
    b = lambda v: "true" if v else "false"   # noqa: E731
    for ns, e, d, pl, scene in (("rtd", 1, 1, 0, "query/torture/xform_in_csg"), ("rtd", 0, 1, 0, "query/dir/pokeball_csg_sun"),
                                ("rtd", 0, 0, 0, "query/bvh/ties"), ("rtd", 0, 0, 1, "query/config3"),
                                ("rtdb", 1, 1, 0, "query/deep/xform_nest12")):
        out.append(Recipe(f"{ns}::k_shade<{b(e)}, {b(d)}, {b(pl)}>", scene, 0, 0, 0))
    return out


class NodeRecipe(NamedTuple):
    """How to launch one row of a node launch table (node_recipes)."""
    row: str              # "ns::kernel<...>", the table row's own name
    scene_name: str       # key of recipe_scene()
    obj: int              # the queried node is top-level object `obj`'s root: desc.objects[obj]
    kind: int             # 0 rt_query_node_intersect, 1 rt_query_node_interval


def node_recipes() -> list[NodeRecipe]:
    """One NodeRecipe per row of the node launch tables (rt_test.h
    rt_test_node_kernel_row): k_node_isect<PROG> / k_node_ivl<PROG>.  The leaf
    rows take a half-space, the program rows of rtd a CSG with transforms
    inside its operands, those of rtdb the bare chain of 12 transforms (a ray
    stack of 12) and the right-nested CSG of 12 leaves (an interval stack of
    12).  tests/test_node_query_plan.py holds this list against the tables,
    tests/test_gpu_node_query.py queries every entry."""
    return [NodeRecipe("rtd::k_node_isect<true>", "torture/xform_in_csg", 1, 0),
            NodeRecipe("rtd::k_node_ivl<true>", "torture/xform_in_csg", 1, 1),
            NodeRecipe("rtd::k_node_isect<false>", "torture/xform_in_csg", 0, 0),
            NodeRecipe("rtd::k_node_ivl<false>", "torture/xform_in_csg", 0, 1),
            NodeRecipe("rtdb::k_node_isect<true>", "deep/xform_nest12", 2, 0),
            NodeRecipe("rtdb::k_node_ivl<true>", "deep/csg_right12", 1, 1)]


def row_timed(row: str, timed: bool) -> str:
    """A paper primary row's name with its T argument set (k_paper_primary<E,
    D, C[, T]>: the untimed rows leave T out; k_paper_primary_lean<C, WV, T,
    PL>); every other row unchanged."""
    head, _, args = row.partition("<")
    a = [v.strip() for v in args.rstrip(">").split(",")]
    if head.endswith("::k_paper_primary"):
        a = a[:3] + (["true"] if timed else [])
    elif head.endswith("::k_paper_primary_lean"):
        a[2] = "true" if timed else "false"
    else:
        return row
    return f"{head}<{', '.join(a)}>"
