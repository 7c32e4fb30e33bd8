"""Translated and scaled scenes on the CPU (no device is touched):
scenes.placed / scenes.PLACEMENTS and the oracle's own behaviour on them, held
here before tests/test_gpu_placed.py relies on either, plus the host half of
the float32 culls (scene_compile.cpp float_ball and the wave BVH records) on
scenes whose float32 bounds overflow.

Frames: the oracle's standard frame of a scale-1 placement is the unplaced
frame within 1e-7 (FP64 cancellation at 1e6 is of order 1e-10 in a hit point;
measured: 1.5e-11 at `mid`, 2.8e-9 at `far`) with identical ray counts; x24
keeps the counts; d100_mid only stays finite and mostly off the background
(the reference's absolute constants - tmin 1e-4, the shadow epsilon, the 0.01
and 0.5 falloff clamps - legitimately change that image).

Query rays: the 768 rays of tests/test_gpu_query.py mapped through the
placement (origins mapped, directions and finite tmax x scale, tmin 1e-4).
For scale >= 1 the oracle's hit flag and material are the unplaced scene's for
every ray; the oracle-unstable rays (probe: the origin +-1e-7 * scale per axis)
stay within the GPU files' caps: 1 % for intersect and occluded, 15 of 768 for
radiance.  Every test prints its counts."""
import json

import numpy as np
import pytest

import scenes
from test_bvh import _bvh
from test_gpu_query import SCENES, Case, case
from test_gpu_radiance import TOL, Ref

UNPLACED = "unplaced"
PL = dict(scenes.PLACEMENTS)
PL[UNPLACED] = (1.0, (0.0, 0.0, 0.0))
FRAME_SCENES = ("torture/csg_ops", "torture/halfspace_in_csg", "torture/pokeball_csg", "torture/rotation_scaling",
                "torture/reflect_refract", "torture/xform_in_csg", "config4", "bvh/grid")
QUERY_SCENES = ("config5", "torture/csg_ops", "torture/xform_in_csg", "torture/halfspace_in_csg",
                "torture/pokeball_csg", "bvh/ties")
RADIANCE_SCENES = ("config5", "torture/reflect_refract", "torture/csg_ops", "bvh/ties", "dir/pokeball_csg_sun")
_frames, _placed, _radiance = {}, {}, {}


# ------------------------------------------------------------------ helpers
def scene_dict(name, dpi=24):
    """(scene dict at `dpi`, directional lights or None) of a frame or query scene name."""
    fam, _, key = name.partition("/")
    if fam == "torture":
        return scenes.torture_scenes(dpi=dpi)[key], None
    if fam == "bvh":
        return scenes.bvh_scenes(dpi)[key], None
    if fam == "deep":
        return scenes.deep_scenes(dpi=dpi)[key], None
    if fam == "dir":
        text, lights = scenes.dir_light_cases(dpi=dpi)[key]
        return json.loads(text), lights
    return json.loads(scenes.config_json(int(name[6:]), dpi=dpi)[0]), None


def placed_any_scale(scene, scale, offset):
    """scenes.placed for a caller without a camera: the dpi is first raised to
    k * scale (k = 24 where the division gives it back exactly, else 1), so
    that placed()'s dpi / scale is the integer k."""
    k = 24 if (24 * scale) / scale == 24 else 1
    return scenes.placed(scenes.with_dpi(scene, k * scale), scale, offset)


def load(rt, scene, lights=None):
    sc = rt.load_scene_from_json_text(json.dumps(scene))
    return rt.with_dir_lights(sc, lights) if lights else sc


def oracle_frame(rt, name, pl, mode=0):
    """(loaded scene, oracle frame, oracle stats) of frame scene `name` under placement `pl`, computed once."""
    key = (name, pl, mode)
    if key not in _frames:
        scene, lights = scene_dict(name)
        sc = load(rt, scenes.placed(scene, *PL[pl]), lights)
        fb, st = rt.oracle_render(sc, sc.width, sc.height, mode, threads=8)
        fb.setflags(write=False)
        _frames[key] = (sc, fb, (st.rays_intersect, st.rays_occluded))
    return _frames[key]


def map_rays(rays, scale, offset):
    out = rays.copy()
    out["o"] = scale * rays["o"] + np.array(offset, dtype=np.float64)
    out["d"] = scale * rays["d"]
    out["tmax"] = np.where(np.isfinite(rays["tmax"]), scale * rays["tmax"], rays["tmax"])
    return out


class PlacedCase(Case):
    """test_gpu_query.Case of `name` under placement `pl`: the placed scene,
    the unplaced case's rays mapped through the placement and the oracle's
    answers for them, computed once."""

    def __init__(self, rt, name, pl):
        self.base = case(rt, name)
        self.scale, self.offset = PL[pl]
        self.step = 1e-7 * self.scale
        text, lights = SCENES[name]
        self.scene = load(rt, placed_any_scale(json.loads(text), self.scale, self.offset), lights)
        self.rt, self.olib, self.desc = rt, rt.oracle_lib(), self.scene.desc_ptr
        self.rays = map_rays(self.base.rays, self.scale, self.offset)
        self.seg_rays = map_rays(self.base.seg_rays, self.scale, self.offset)
        self.ref_hit, self.ref_rec = self.oracle_intersect(self.rays)
        self.ref_occ = self.oracle_occluded(self.seg_rays)
        for a in (self.rays, self.seg_rays, self.ref_hit, self.ref_rec, self.ref_occ):
            a.setflags(write=False)


def placed_case(rt, name, pl):
    if (name, pl) not in _placed:
        _placed[name, pl] = PlacedCase(rt, name, pl)
    return _placed[name, pl]


def placed_ref(rt, name, pl):
    """test_gpu_radiance.Ref of the placed case's rays (the oracle's trace of
    them), computed once.  At e25 and e39 the scene's recursion limit is 1:
    the reference starts a reflected or refracted ray at tmin = 1e-4, an
    absolute length that drowns in the FP64 rounding of a hit point of size
    1e25 (2e9), so there the oracle's own bounces are noise (213 of config 5's
    768 rays move under the probe); direct shading, whose shadow epsilon is
    relative (1e-4 t), stays exact."""
    if (name, pl) not in _radiance:
        c = placed_case(rt, name, pl)
        sc = rt.with_recursion_limit(c.scene, 1) if c.scale >= 1e25 else c.scene
        _radiance[name, pl] = Ref(rt, sc, c.rays["o"], c.rays["d"])
    return _radiance[name, pl]


# ------------------------------------------------------------------- placed()
def test_placed_maps_every_field():
    s = {"screen": {"dpi": 48, "dimensions": [4, 3], "position": [-2, -1.5, 0], "observer": [0, 0.3, 5]},
         "medium": {"ambient": [0.2, 0.2, 0.2], "index": 1.0, "recursion": 3}, "background": [0.3, 0.4, 0.6],
         "sources": [{"position": [1, 2, 3], "intensity": [4, 5, 6]}],
         "objects": [
             {"sphere": {"position": [1, 0, -1], "radius": 0.5, "color": {"diffuse": [1, 0, 0]}, "index": 1.5}},
             {"halfSpace": {"position": [0, -1, 0], "normal": [0, 1, 0]}},
             {"pokeball": {"position": [0, 1, 0], "radius": 0.25, "button_dir": [0, 0, 1], "belt_half": 0.1}},
             {"translation": {"factors": [1, 2, 3], "subject": {"sphere": {"position": [0, 0, 0], "radius": 1}}}},
             {"csg": {"operator": "union", "left": {"sphere": {"position": [0, 0, 0], "radius": 1}},
                      "right": {"difference": [{"sphere": {"position": [2, 0, 0], "radius": 1}},
                                               {"rotation": {"angle": 30, "direction": 1, "subject": {
                                                   "sphere": {"position": [2, 0, 0], "radius": 0.5}}}}]}}},
             {"scaling": {"factors": [1, 2, 1], "subject": {"sphere": {"position": [0, 1, 0], "radius": 1}}}}]}
    before = json.dumps(s)
    p = scenes.placed(s, 2.0, (10.0, 20.0, 30.0))
    assert json.dumps(s) == before   # a deep copy
    assert p["screen"] == {"dpi": 24, "dimensions": [8.0, 6.0], "position": [6.0, 17.0, 30.0],
                           "observer": [10.0, 20.6, 40.0]}
    assert p["medium"] == s["medium"] and p["background"] == s["background"]
    assert p["sources"] == [{"position": [12.0, 24.0, 36.0], "intensity": [16.0, 20.0, 24.0]}]
    o = p["objects"]
    assert o[0] == {"sphere": {"position": [12.0, 20.0, 28.0], "radius": 1.0, "color": {"diffuse": [1, 0, 0]},
                               "index": 1.5}}
    assert o[1] == {"halfSpace": {"position": [10.0, 18.0, 30.0], "normal": [0, 1, 0]}}
    assert o[2] == {"pokeball": {"position": [10.0, 22.0, 30.0], "radius": 0.5, "button_dir": [0, 0, 1],
                                 "belt_half": 0.1}}
    assert o[3] == {"translation": {"factors": [2.0, 4.0, 6.0],
                                    "subject": {"sphere": {"position": [10.0, 20.0, 30.0], "radius": 2.0}}}}
    rot = o[4]["csg"]["right"]["difference"][1]
    assert o[4]["csg"]["operator"] == "union" and o[4]["csg"]["left"]["sphere"]["radius"] == 2.0
    assert rot == {"translation": {"factors": [10.0, 20.0, 30.0], "subject": {"rotation": {
        "angle": 30, "direction": 1, "subject": {"translation": {"factors": [-10.0, -20.0, -30.0], "subject": {
            "sphere": {"position": [14.0, 20.0, 30.0], "radius": 1.0}}}}}}}}
    assert o[5]["translation"]["subject"]["scaling"]["factors"] == [1, 2, 1]
    # without an offset the linear nodes commute with the scale: no conjugation
    q = scenes.placed(s, 2.0, (0, 0, 0))
    assert q["objects"][5] == {"scaling": {"factors": [1, 2, 1],
                                           "subject": {"sphere": {"position": [0.0, 2.0, 0.0], "radius": 2.0}}}}


def test_placed_refuses_what_it_does_not_know():
    s, _ = scene_dict("torture/csg_ops")
    for scale in (48.0, 5.0, 0.7):   # dpi 24 / scale: below 1, not an integer
        with pytest.raises(ValueError):
            scenes.placed(s, scale, (0, 0, 0))
    assert scenes.placed(s, 24.0, (0, 0, 0))["screen"]["dpi"] == 1
    assert scenes.placed(s, 0.01, (0, 0, 0))["screen"]["dpi"] == 2400
    with pytest.raises(KeyError):
        scenes.placed(dict(s, fog=1), 1.0, (0, 0, 0))
    with pytest.raises(KeyError):
        scenes.placed(dict(s, objects=[{"torus": {"position": [0, 0, 0]}}]), 1.0, (0, 0, 0))
    with pytest.raises(KeyError):
        scenes.placed(dict(s, objects=[{"sphere": {"position": [0, 0, 0], "radius": 1, "centre": [0, 0, 0]}}]), 1.0,
                      (0, 0, 0))
    assert set(scenes.FRAME_PLACEMENTS) | set(scenes.QUERY_PLACEMENTS) == set(scenes.PLACEMENTS)
    for name in scenes.QUERY_PLACEMENTS:   # (every scale has a dpi that divides exactly)
        assert placed_any_scale(s, *scenes.PLACEMENTS[name])["screen"]["dpi"] in (1, 24)


# --------------------------------------------------------------------- frames
@pytest.mark.parametrize("pl", scenes.FRAME_PLACEMENTS)
@pytest.mark.parametrize("name", FRAME_SCENES)
def test_oracle_frame_under_placement(rt, name, pl):
    sc0, fb0, counts0 = oracle_frame(rt, name, UNPLACED)
    sc, fb, counts = oracle_frame(rt, name, pl)
    assert (sc.width, sc.height) == (sc0.width, sc0.height) and sc.width <= 96 and sc.height <= 72
    scale = PL[pl][0]
    err = float(np.abs(fb - fb0).max())
    print(f"  {name} {pl}: {sc.width}x{sc.height}, max|d| to the unplaced oracle frame {err:.3g}, counts {counts} "
          f"(unplaced {counts0})")
    if scale == 1.0:
        assert err <= 1e-7 and counts == counts0
    elif scale > 1.0:
        assert counts == counts0
    else:
        assert np.isfinite(fb).all()
        off_bg = (np.abs(fb - np.array(list(sc.desc.background))).max(axis=2) > 0).sum()
        assert off_bg >= sc.width * sc.height // 4


# ----------------------------------------------------------------- query rays
@pytest.mark.parametrize("pl", scenes.QUERY_PLACEMENTS)
@pytest.mark.parametrize("name", QUERY_SCENES)
def test_oracle_queries_under_placement(rt, name, pl):
    c = placed_case(rt, name, pl)
    b = c.base
    if c.scale >= 1.0:
        assert np.array_equal(c.ref_hit, b.ref_hit) and np.array_equal(c.ref_rec["mat"], b.ref_rec["mat"])
        assert np.array_equal(c.ref_occ, b.ref_occ)
    else:
        assert c.ref_hit.sum() >= len(c.rays) // 4
    n_i = sum(c.oracle_unstable(r, False, c.step) for r in c.rays)
    n_o = sum(c.oracle_unstable(r, True, c.step) for r in c.seg_rays)
    print(f"  {name} {pl}: {int(c.ref_hit.sum())} hits, {int(c.ref_occ.sum())} occluded, oracle-unstable: "
          f"intersect {n_i}, occluded {n_o} of {len(c.rays)}")
    assert n_i <= len(c.rays) // 100 and n_o <= len(c.rays) // 100


@pytest.mark.parametrize("pl", scenes.QUERY_PLACEMENTS)
@pytest.mark.parametrize("name", RADIANCE_SCENES)
def test_oracle_radiance_under_placement(rt, name, pl):
    r = placed_ref(rt, name, pl)
    step = placed_case(rt, name, pl).step
    n, unstable = len(r), 0
    for ax in range(3):
        moved = np.zeros(n, dtype=bool)
        for sgn in (1.0, -1.0):
            o = r.o.copy()
            o[:, ax] += sgn * step
            rgb, ni, no = rt.oracle_trace(r.sc, o, r.d)
            moved |= (np.abs(rgb - r.rgb).max(axis=1) > TOL) | (ni != r.ni) | (no != r.no)
        unstable = moved if ax == 0 else (unstable | moved)
    hits = int((np.abs(r.rgb - r.background).max(axis=1) > 0).sum())
    print(f"  {name} {pl}: {hits} of {n} rays off the background, oracle-unstable (colour at 1e-5 or counts): "
          f"{int(unstable.sum())}")
    assert np.isfinite(r.rgb).all() and hits >= n // 4
    assert int(unstable.sum()) <= n * 15 // 768


# ------------------------------------------------------------------ host half
@pytest.mark.parametrize("pl", ["far", "e25", "e39"])
def test_placed_scenes_compile(rt, pl):
    """Scenes whose float32 bounds overflow (e25: the squares; e39: the
    coordinates themselves) still compile, and their wave BVH lists every
    object the unplaced scene's lists, exactly once."""
    for name in sorted(set(FRAME_SCENES) | set(QUERY_SCENES)):
        scene, _ = scene_dict(name)
        b = _bvh(rt, placed_any_scale(scene, *PL[pl]))
        b0 = _bvh(rt, scene)
        assert b["n_objs"] > 0
        print(f"  {name} {pl}: {b['n_objs']} objects, {b['groups']} groups, BVH {b['n']} entries in {b['chunks']} chunks")
        if name.startswith("bvh/"):
            assert b0["n"] > 0
        if b0["n"] > 0:
            assert b["n"] > 0 and b["chunks"] > 0
            real, real0 = b["worig"][b["worig"] >= 0], b0["worig"][b0["worig"] >= 0]
            assert len(real) == len(set(real.tolist()))
            # (the compiled table's order follows the bounds, so the indices themselves may differ)
            assert len(real) == len(real0) and (b["n_objs"], b["groups"]) == (b0["n_objs"], b0["groups"])
