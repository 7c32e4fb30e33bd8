"""Shading queries on the CPU (no device is touched): the reference the GPU
tests use, rtamd.oracle_shade (a numpy restatement of shading.cpp:31-138 whose
Scene::occluded is the oracle's), held to the pinned oracle's own
shade_lambert_phong; the kernel a shading query launches (frame_plan.cpp
pick_shade_variant + the shade table of rt_shade_kernels.hpp) through
rt_test_shade_kernel_name; and the census list scenes.shade_recipes() against
the tables.  The kernels' results are checked against oracle_shade by
tests/test_gpu_shade.py, which takes its hits and expected values from
shade_ref() here.

The oracle's own shading: at recursion limit 1 Tracer::trace returns `direct`
(tracer.cpp:26-38: every child ray needs depth < limit - 1), so
oracle_trace(with_recursion_limit(scene, 1), o, d) is shade_lambert_phong of
the ray's closest hit with wo = -d, and its Scene::occluded count is the
shading's.

Bars: occluded counts equal per hit; missed rays return the background; finite
channels within 1e-9; non-finite channels equal as non-finite values.  Measured
on the CPU over all the scenes below: the largest difference is 3.3e-11
(numpy's pow and summation order; colours are at most 1.5), so the bar leaves a
30x margin; shading/exponents_wave has 7 hits with an infinite channel
(pow(0, -2)), which exercise the non-finite rule."""
import ctypes as C
import json

import numpy as np
import pytest

import scenes
from test_gpu_query import SCENES, case
from test_gpu_radiance import recipe_rays

RT_ERR_INVALID_ARG, RT_ERR_UNSUPPORTED = -1, -6
BAR = 1e-9
SHADING = ("lights65_csg", "near_light_wave", "far_skip_few", "null_mat_csg", "exponents_wave", "extremes_few",
           "extremes_csg", "lights33_xform")
OVERRIDES = [("config4", 0), ("config4", 1), ("config4", 33), ("dir/pokeball_csg_sun", 2)]
_refs = {}


# ---------------------------------------------------------------- reference
def override_lights(name, n):
    """n point lights [(pos, intensity), ...] for scene `name`, fixed by (name, n)."""
    rng = np.random.default_rng(9000 + 131 * n + len(name))
    pos = rng.uniform([-4.0, 0.5, -5.0], [4.0, 5.0, 3.0], (n, 3))
    inten = rng.uniform(0.1, 0.6, (n, 3)) * min(1.0, 4.0 / max(1, n))
    return [(p.tolist(), i.tolist()) for p, i in zip(pos, inten)]


def view_dirs(d):
    """wo = (-r.d).normalized() of Ray(o, d) (tracer.cpp:30, core.h:278)."""
    d = np.asarray(d, dtype=np.float64)
    dh = d / np.sqrt((d * d).sum(axis=1))[:, None]
    return -dh / np.sqrt((dh * dh).sum(axis=1))[:, None]


class ShadeRef:
    """Rays of one scene, the oracle's closest hits H of them (hit: the flags;
    a miss is mat -1 and zeros), wo = -d, and oracle_shade of the hits under
    `lights` (None: the scene's own), computed once and left unchanged."""

    def __init__(self, rt, sc, o, d, lights=None):
        self.sc, self.lights = sc, lights
        self.o = np.ascontiguousarray(o, dtype=np.float64)
        self.d = rt.oracle_trace_dirs(self.o, d)
        olib, desc = rt.oracle_lib(), sc.desc_ptr
        n = len(self.o)
        self.hit = np.zeros(n, dtype=bool)
        self.H = np.zeros(n, dtype=rt.HIT_DTYPE)
        self.H["mat"] = -1
        h = rt.OracleHit()
        for k in range(n):
            ok = olib.oracle_scene_intersect(desc, self.o[k].ctypes.data_as(C.POINTER(C.c_double)),
                                             self.d[k].ctypes.data_as(C.POINTER(C.c_double)), 1e-4, float("inf"),
                                             C.byref(h))
            if ok:
                self.hit[k] = True
                self.H[k] = (h.t, tuple(h.p), tuple(h.n), h.mat, h.front_face)
        self.wo = view_dirs(self.d)
        self.background = np.array(list(sc.desc.background))
        self.rgb = np.tile(self.background, (n, 1))
        self.no = np.zeros(n, dtype=np.int64)
        self.rgb[self.hit], self.no[self.hit] = rt.oracle_shade(sc, self.H[self.hit], self.wo[self.hit], lights)
        for a in (self.o, self.d, self.hit, self.H, self.wo, self.rgb, self.no):
            a.setflags(write=False)

    def __len__(self):
        return len(self.o)

    def trace_scene(self, rt):
        """The scene whose Tracer::trace is this reference's shading."""
        sc = self.sc if self.lights is None else rt.with_point_lights(self.sc, self.lights)
        return rt.with_recursion_limit(sc, 1)


def _load(rt, name):
    text, lights = scenes.recipe_scene(name)
    sc = rt.load_scene_from_json_text(text)
    return rt.with_dir_lights(sc, lights) if lights else sc


def shade_ref(rt, key):
    """The ShadeRef of `key`: a scene of test_gpu_query.SCENES with that file's
    768 rays; "shading/<name>" (scenes.shading_scenes(dpi=16), 192 + 192 rays
    of test_gpu_radiance.recipe_rays); "override/<SCENES name>/<n>" (n
    override_lights instead of the scene's); "census/<recipe scene>" (128 +
    128 rays)."""
    if key in _refs:
        return _refs[key]
    if key in SCENES:
        c = case(rt, key)
        r = ShadeRef(rt, c.scene, c.rays["o"], c.rays["d"])
    elif key.startswith("shading/"):
        name = key[8:]
        sc = scenes.shading_load(rt, name, scenes.shading_scenes(dpi=16)[name])
        r = ShadeRef(rt, sc, *recipe_rays(rt, sc, 192, 192, 7100 + len(name)))
    elif key.startswith("override/"):
        name, n = key[9:].rsplit("/", 1)
        c = case(rt, name)
        r = ShadeRef(rt, c.scene, *recipe_rays(rt, c.scene, 192, 192, 8100 + int(n)), lights=override_lights(name, int(n)))
    elif key.startswith("census/"):
        sc = _load(rt, key[7:])
        r = ShadeRef(rt, sc, *recipe_rays(rt, sc, 128, 128, 4242))
    else:
        raise KeyError(key)
    _refs[key] = r
    return r


def hold_to_oracle(rt, r, what):
    """oracle_shade of r against the pinned oracle's shading of the same rays
    at this file's bars; returns (largest finite difference, non-finite hits)."""
    rgb, ni, no = rt.oracle_trace(r.trace_scene(rt), r.o, r.d)
    assert np.array_equal(ni, np.ones(len(r), dtype=np.int64)), what   # (one Scene::intersect call per ray: no bounce)
    assert np.array_equal(no, r.no), (what, np.flatnonzero(no != r.no)[:8])
    assert not r.no[~r.hit].any()
    # (oracle_trace returns the mean of 8 equal samples: the background up to that sum's rounding)
    assert float(np.abs(rgb[~r.hit] - r.background).max(initial=0.0)) <= 1e-15, what
    assert np.array_equal(r.rgb[~r.hit], np.tile(r.background, (int((~r.hit).sum()), 1)))
    fin = np.isfinite(rgb)
    assert np.array_equal(fin, np.isfinite(r.rgb)), what
    with np.errstate(invalid="ignore"):
        err = float(np.abs(np.where(fin, r.rgb - rgb, 0.0)).max(initial=0.0))
    # non-finite channels: the same value (+inf, -inf or NaN)
    assert np.array_equal(r.rgb[~fin], rgb[~fin], equal_nan=True), what
    nonfinite = int((~fin).any(axis=1).sum())
    print(f"  {what}: {len(r)} rays, {int(r.hit.sum())} hits, {int(r.no.sum())} occluded calls, max|d|={err:.3g}, "
          f"{nonfinite} hits with a non-finite channel")
    assert err <= BAR, what
    return err, nonfinite


# ------------------------------------- 1. the restatement is the oracle's shading
@pytest.mark.parametrize("name", sorted(SCENES))
def test_oracle_shade_is_the_oracles_shading(rt, name):
    r = shade_ref(rt, name)
    assert len(r) == 768
    hold_to_oracle(rt, r, name)
    assert r.hit.sum() >= len(r) // 4


@pytest.mark.parametrize("name", SHADING)
def test_oracle_shade_on_the_shading_inputs(rt, name):
    r = shade_ref(rt, "shading/" + name)
    _, nonfinite = hold_to_oracle(rt, r, "shading/" + name)
    if name == "exponents_wave":
        assert nonfinite > 0   # (pow(0, -2): the non-finite rule is exercised)
    if name == "null_mat_csg":
        null = r.hit & (r.H["mat"] == -1)
        assert null.any() and not r.no[null].any()
        assert np.array_equal(r.rgb[null], np.tile([1.0, 0.0, 1.0], (int(null.sum()), 1)))


@pytest.mark.parametrize("name,n", OVERRIDES, ids=[f"{a}-{b}" for a, b in OVERRIDES])
def test_oracle_shade_with_other_point_lights(rt, name, n):
    r = shade_ref(rt, f"override/{name}/{n}")
    assert len(r.lights) == n
    hold_to_oracle(rt, r, f"{name} with {n} lights")
    if name.startswith("dir/"):
        assert r.sc.desc.n_dir_lights > 0   # (the directional lights stay the scene's)


def test_out_of_range_material_is_a_null_material(rt):
    r = shade_ref(rt, "config4")
    H = r.H[r.hit][:4].copy()
    H["mat"] = [-1, -2, r.sc.desc.n_materials, 2**31 - 1]
    rgb, no = rt.oracle_shade(r.sc, H, r.wo[r.hit][:4])
    assert np.array_equal(rgb, np.tile([1.0, 0.0, 1.0], (4, 1))) and not no.any()


# ------------------------------------------------------------ 2. the planner
def _args(name):
    return [a.strip() for a in name.split("<", 1)[1].rsplit(">", 1)[0].split(",")]


def _kernel(rt, sc, flags=0):
    rc, name = rt.shade_kernel_name(sc, flags)
    assert rc == 0, rt.last_error()
    assert "::k_shade<" in name and len(_args(name)) == 3   # E, D, PL
    return name


def _plan_scenes():
    out = {}
    for k, v in scenes.torture_scenes(dpi=12).items():
        out["torture/" + k] = json.dumps(v)
    for k, v in scenes.deep_scenes().items():
        out["deep/" + k] = json.dumps(v)
    for n in (1, 2, 3, 4, 5, 6):
        out[f"config{n}"] = scenes.config_json(n, dpi=24)[0]
    return out


@pytest.mark.parametrize("name", sorted(_plan_scenes()))
def test_kernel_choice_is_the_occluded_querys(rt, name):
    sc = rt.load_scene_from_json_text(_plan_scenes()[name])
    for flags in (0, rt.RT_FLAG_NO_CULL, rt.RT_FLAG_NO_BVH, rt.RT_FLAG_FORCE_BVH):
        rc, q = rt.query_kernel_name(sc, 1, flags)
        assert rc == 0 and "k_query_occl<" in q
        assert _kernel(rt, sc, flags) == q.replace("k_query_occl<", "k_shade<")
    assert _kernel(rt, sc, rt.RT_FLAG_NO_CULL) == _kernel(rt, sc)


def test_directional_lights_take_a_d_row(rt):
    text, lights = SCENES["dir/pokeball_csg_sun"]
    sc = rt.with_dir_lights(rt.load_scene_from_json_text(text), lights)
    assert _args(_kernel(rt, sc))[1] == "true"


def test_refused_flags(rt):
    sc = rt.load_scene_from_json_text(scenes.config_json(3, dpi=24)[0])
    rc, _ = rt.shade_kernel_name(sc, rt.RT_FLAG_FP32)
    assert rc == RT_ERR_UNSUPPORTED and "FP32" in rt.last_error()
    rc, _ = rt.shade_kernel_name(sc, rt.RT_FLAG_COUNT_OPS)
    assert rc == RT_ERR_UNSUPPORTED and "COUNT_OPS" in rt.last_error()
    buf = C.create_string_buffer(16)
    assert rt.amd_lib().rt_test_shade_kernel_name(None, 0, buf, 16) == RT_ERR_INVALID_ARG
    assert rt.amd_lib().rt_test_shade_kernel_name(sc.handle, 0, None, 16) == RT_ERR_INVALID_ARG


def test_scene_beyond_the_big_stacks_is_refused_like_the_other_queries(rt):
    leaves = [{"sphere": {"position": [0.01 * i, 0, -2], "radius": 0.5, "color": {"diffuse": [1, 1, 1]}}}
              for i in range(80)]
    node = leaves[-1]
    for leaf in reversed(leaves[:-1]):
        node = {"csg": {"operator": "union", "left": leaf, "right": node}}
    sc = rt.load_scene_from_json_text(json.dumps({"screen": {"dpi": 4, "dimensions": [2, 2], "position": [-1, -1, 0],
                                                             "observer": [0, 0, 3]}, "objects": [node]}))
    assert rt.query_kernel_name(sc, 1)[0] == RT_ERR_UNSUPPORTED
    query_msg = rt.last_error()
    rc, _ = rt.shade_kernel_name(sc)
    assert rc == RT_ERR_UNSUPPORTED and "CSG operand depth 80" in rt.last_error()
    assert rt.last_error() == query_msg
    # a recursion depth beyond the stacks is no obstacle: shading traces no bounce
    deep = rt.load_scene_from_json_text(json.dumps(scenes.deep_recursion_scene(131)))
    assert rt.shade_kernel_name(deep)[0] == 0


# ------------------------------------------------------------------- census
def test_every_row_has_exactly_one_recipe(rt):
    recipes = scenes.shade_recipes()
    assert len(rt.SHADE_TABLES) == 2
    rows = []
    for table, ns in enumerate(("rtd", "rtdb")):
        got = rt.shade_rows(table)
        assert got and all(r.startswith(ns + "::k_shade<") for r in got), (table, got)
        assert len(set(got)) == len(got)
        rows += got
    assert rt.shade_rows(0) == ["rtd::k_shade<true, true, false>", "rtd::k_shade<false, true, false>",
                                "rtd::k_shade<false, false, false>", "rtd::k_shade<false, false, true>"]
    assert rt.shade_rows(1) == ["rtdb::k_shade<true, true, false>"]
    assert sorted(r.row for r in recipes) == sorted(rows)   # one each, none for a row no table has


@pytest.mark.parametrize("recipe", scenes.shade_recipes(), ids=lambda r: r.row)
def test_each_recipes_scene_picks_its_row(rt, recipe):
    assert _kernel(rt, _load(rt, recipe.scene_name), recipe.flags) == recipe.row


def test_row_hook_bounds(rt):
    lib = rt.amd_lib()
    buf = C.create_string_buffer(160)
    assert lib.rt_test_shade_kernel_row(2, 0, buf, 160) == RT_ERR_INVALID_ARG
    assert lib.rt_test_shade_kernel_row(-1, 0, buf, 160) == RT_ERR_INVALID_ARG
    assert lib.rt_test_shade_kernel_row(0, -1, buf, 160) == RT_ERR_INVALID_ARG
    assert lib.rt_test_shade_kernel_row(0, len(rt.shade_rows(0)), buf, 160) == RT_ERR_INVALID_ARG
    assert lib.rt_test_shade_kernel_row(1, 1, buf, 160) == RT_ERR_INVALID_ARG
    assert lib.rt_test_shade_kernel_row(0, 0, None, 160) == RT_ERR_INVALID_ARG
    assert lib.rt_test_shade_kernel_row(0, 0, buf, 160) == 0 and buf.value.decode() == rt.shade_rows(0)[0]
