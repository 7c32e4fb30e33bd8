"""The shading scene family (scenes.shading_scenes) reaches what it is built
for.  Every condition here is computed from the CPU oracle and the frame's
pixel-centre primary hits (rtamd.oracle_primary_hits), never from the GPU, so
the GPU parity tests of tests/test_gpu_shading.py compare frames that are
known to contain the branch each case names: the second and third 32-light
round of shade(), the dist_squared <= 0.01 clamp, max(0.5, distance), the
max_shadow_t <= shadow_epsilon skip, visible highlights of every exponent,
total internal reflection on entry.  Kernel choice is host logic
(rt_test_kernel_name), so the layouts' kernels are checked here too."""
import numpy as np
import pytest

import scenes

DPI = 24
SCENES = scenes.shading_scenes(DPI)
_cache = {}


def _scene(rt, name):
    if name not in _cache:
        _cache[name] = scenes.shading_load(rt, name, SCENES[name])
    return _cache[name]


def _ops(rt, st):
    return {n: int(st.ops[i]) for i, n in enumerate(rt.OP_NAMES)}


def test_frames_are_small():
    for name, s in SCENES.items():
        scr = s["screen"]
        w, h = round(scr["dimensions"][0] * scr["dpi"]), round(scr["dimensions"][1] * scr["dpi"])
        cap = (256, 192) if name.startswith("exponents") else (128, 96)
        assert w <= cap[0] and h <= cap[1], (name, w, h)


def test_layouts_reach_four_kernels(rt):
    names = {}
    for lay in scenes.SHADING_LAYOUTS:
        rc, names[lay] = rt.kernel_name(_scene(rt, f"lights33_{lay}"), 0)
        assert rc == 0
        print(f"  {lay:6s} {names[lay]}")
    assert all(n.startswith("rtd::") for n in names.values()), names
    assert len(set(names.values())) >= 4, names
    # few: no wave culls; wave / csg: wave culls, plain and not; xform: eager (D); bvh: the wave BVH
    arg = lambda n: [a.strip() for a in n.split("<", 1)[1].rsplit(">", 1)[0].split(",")]
    assert arg(names["few"])[1] == "0" and arg(names["wave"])[1] == "1" and arg(names["bvh"])[1] == "2", names
    assert arg(names["wave"])[-1] == "true" and arg(names["csg"])[-1] == "false", names
    assert names["xform"].startswith("rtd::k_std<true"), names


MANY = sorted(n for n in SCENES if n.startswith("lights"))


@pytest.mark.parametrize("name", MANY)
def test_many_lights_conditions(rt, name):
    sc = _scene(rt, name)
    assert sc.desc.n_lights == int(name[6:8])
    fb, st = rt.oracle_render(sc, sc.width, sc.height, 0, threads=8)
    ops = _ops(rt, st)
    clamp = float(np.mean(fb == 1.5))
    unlit = 1.0 - ops["shade_light"] / ops["light_eval"]
    lit = [b["lit"] for b in scenes.shading_light_branches(rt, sc, with_shadows=True)]
    print(f"  {name}: max {fb.max():.3f} clamped {clamp:.4f} unlit {unlit:.3f} min lit pixels {min(lit)}")
    assert clamp <= 0.10
    assert 0.05 <= unlit <= 0.60
    assert min(lit) >= 16, lit


@pytest.mark.parametrize("lay", ["wave", "csg"])
def test_one_of_65_conditions(rt, lay):
    base = _scene(rt, f"one65_k00_{lay}")
    d = rt.SceneDesc.from_buffer_copy(base.desc)
    dark = (rt.Light * d.n_lights)()
    for i in range(d.n_lights):
        dark[i].pos[:] = d.lights[i].pos[:]
    import ctypes as C

    d.lights = C.cast(dark, C.POINTER(rt.Light))
    zero = rt.scene_from_desc(d)
    fb0, _ = rt.oracle_render(zero, zero.width, zero.height, 0, threads=8)
    for k in scenes.ONE_OF_65:
        sc = _scene(rt, f"one65_k{k:02d}_{lay}")
        L = sc.desc.lights
        assert [i for i in range(65) if any(L[i].intensity[:])] == [k]
        fb, st = rt.oracle_render(sc, sc.width, sc.height, 0, threads=8)
        n = int((np.abs(fb - fb0).max(axis=2) > 1e-3).sum())
        print(f"  one65_k{k:02d}_{lay}: {n} pixels differ from the dark frame, {st.rays_occluded} shadow rays")
        assert n >= 32


@pytest.mark.parametrize("lay", ["few", "wave", "bvh"])
def test_near_light_conditions(rt, lay):
    sc = _scene(rt, f"near_light_{lay}")
    br = scenes.shading_light_branches(rt, sc)
    print(f"  near_light_{lay}: {br}")
    assert br[0]["clamped"] >= 32          # the light 0.05 above the floor
    assert br[1]["half"] >= 32 and br[1]["clamped"] == 0   # the light 0.3 off the sphere
    assert br[2]["half"] == 0 and br[2]["queried"] >= 32   # the ordinary one


@pytest.mark.parametrize("lay", ["few", "wave"])
def test_far_skip_conditions(rt, lay):
    sc = _scene(rt, f"far_skip_{lay}")
    br = scenes.shading_light_branches(rt, sc)
    fb, _ = rt.oracle_render(sc, sc.width, sc.height, 0, threads=8)
    print(f"  far_skip_{lay}: {br} frame in [{fb.min():.3f}, {fb.max():.3f}]")
    assert br[0]["skipped"] >= 32 and br[1]["skipped"] >= 32
    assert br[2]["skipped"] == 0
    assert -2.0 <= fb.min() and fb.max() <= 2.0


EXPO = sorted(n for n in SCENES if n.startswith("exponents"))


@pytest.mark.parametrize("name", EXPO)
def test_every_exponent_is_visible(rt, name):
    sc = _scene(rt, name)
    fb, _ = rt.oracle_render(sc, sc.width, sc.height, 0, threads=8)
    d = sc.desc
    shin = {}
    for i in range(d.n_nodes):
        if d.nodes[i].kind == rt.NODE_SPHERE:
            shin[int(d.nodes[i].mat)] = d.materials[d.nodes[i].mat].shininess
    assert len(shin) == (15 if name == "exponents_wave" else 3)
    for m, y in sorted(shin.items()):
        assert 0.4 <= d.materials[m].ks <= 0.9
        off = rt.with_material_fields(sc, {m: {"ks": 0.0}})
        fb1, _ = rt.oracle_render(off, sc.width, sc.height, 0, threads=8)
        same = (fb == fb1) | (np.isnan(fb) & np.isnan(fb1))   # (the -2 sphere's pixels are +-inf / NaN in both)
        with np.errstate(invalid="ignore"):
            diff = np.where(same, 0.0, np.abs(fb - fb1))
        n = int((~(diff <= 1e-4)).any(axis=2).sum())
        print(f"  {name}: shininess {y:g} changes {n} pixels")
        assert n >= 8, (y, n)
    if name == "exponents_wave":
        assert set(shin.values()) == set(float(v) for v in scenes.SHADING_EXPONENTS)


def test_exponents_few_cover_every_exponent(rt):
    seen = set()
    for name in EXPO:
        if name != "exponents_wave":
            d = _scene(rt, name).desc
            seen |= {d.materials[d.nodes[i].mat].shininess for i in range(d.n_nodes)
                     if d.nodes[i].kind == rt.NODE_SPHERE}
    assert seen == set(float(v) for v in scenes.SHADING_EXPONENTS)


def test_extremes_conditions(rt):
    for lay in ("few", "csg"):
        sc = _scene(rt, f"extremes_{lay}")
        d = sc.desc
        mats = [d.materials[i] for i in range(d.n_materials)]
        assert any(m.kd == 0.0 for m in mats) and any(m.ks == 0.0 for m in mats)
        assert any(max(m.albedo[:]) > 1.0 for m in mats) and any(not any(m.ambient[:]) for m in mats)
        assert any(min(d.lights[i].intensity[:]) < 0 for i in range(d.n_lights))
        fb, _ = rt.oracle_render(sc, sc.width, sc.height, 0, threads=8)
        on_clamp = float(np.mean(fb == 1.5))
        print(f"  extremes_{lay}: {on_clamp:.3f} of the values on the 1.5 clamp, min {fb.min():.3f}")
        assert 0.02 <= on_clamp <= 0.9 and fb.min() < 0.0


@pytest.mark.parametrize("name", sorted(n for n in SCENES if n.startswith("media")))
def test_media_conditions(rt, name):
    sc = _scene(rt, name)
    d = sc.desc
    assert d.medium_index == 1.33
    _, st = rt.oracle_render(sc, sc.width, sc.height, 0, threads=8)
    sec = _ops(rt, st)["secondary"]
    assert (sec > 0) == (d.recursion_limit >= 2)
    tir_mat = [i for i in range(d.n_materials) if d.materials[i].refractive_index == 1.0 and d.materials[i].kt > 0]
    assert len(tir_mat) == 1
    assert any(d.materials[i].refractive_index == 1.33 and d.materials[i].kt > 0 for i in range(d.n_materials))
    assert any(d.materials[i].kr > 0 and d.materials[i].kt > 0 for i in range(d.n_materials))
    rec = rt.oracle_primary_hits(sc)
    h = rec[rec["hit"] & (rec["mat"] == tir_mat[0]) & (rec["front_face"] == 1)]
    cos_i = -(h["d"] * h["n"]).sum(1)
    eta = d.medium_index / 1.0
    tir = eta * eta * np.maximum(0.0, 1.0 - cos_i * cos_i) >= 1.0   # tracer.cpp:100-104
    print(f"  {name}: secondary {sec}, index-1.0 sphere: {int(tir.sum())} TIR on entry, {int((~tir).sum())} refracted")
    assert tir.sum() >= 16 and (~tir).sum() >= 16


def test_null_mat_scenes(rt):
    for name, n_null in (("null_mat_few", 1), ("null_mat_csg", 3)):
        sc = _scene(rt, name)
        d = sc.desc
        null = [i for i in range(d.n_nodes) if d.nodes[i].kind == rt.NODE_SPHERE and d.nodes[i].mat == -1]
        assert len(null) == n_null
        rec = rt.oracle_primary_hits(sc)
        n_hit = int((rec["hit"] & (rec["mat"] == -1)).sum())
        fb, _ = rt.oracle_render(sc, sc.width, sc.height, 0, threads=8)
        magenta = int(np.all(fb == [1.0, 0.0, 1.0], axis=2).sum())
        print(f"  {name}: {n_hit} pixel-centre hits without a material, {magenta} magenta pixels")
        assert n_hit >= 32 and magenta >= 16
    # the left operand of one union and the right operand of another
    d = _scene(rt, "null_mat_csg").desc
    csg = [d.nodes[i] for i in range(d.n_nodes) if d.nodes[i].kind == rt.NODE_CSG]
    assert any(d.nodes[c.a].mat == -1 and d.nodes[c.b].mat >= 0 for c in csg)
    assert any(d.nodes[c.b].mat == -1 and d.nodes[c.a].mat >= 0 for c in csg)
