"""GPU parity of shade() and the trace loops (rt_device.hpp; shading.cpp:31-138,
tracer.cpp:22-104) on the inputs no other scene has: scenes.shading_scenes,
whose frames tests/test_shading_inputs.py shows to contain the branches they
are named after and tests/golden/shading.npz pins to the reference.

Every case x layout, both modes, against the CPU oracle at the bar of
test_gpu_parity.py: per-channel |d| <= 1e-5 (where the oracle is not finite
- pow(0, -2) = inf - the GPU must be non-finite of the same kind in the same
place), equal Scene::intersect / Scene::occluded counts, paper mode bit-exact.
Then the op counters (a lit-mask or light-round error whose pixel contribution
is small still changes light_eval / shade_light / shade_spec), RT_FLAG_NO_CULL
frames, partial waves and ray queries of null-material hits.  No pixel and no
ray is left out."""
import json

import numpy as np
import pytest

import scenes
from test_gpu_parity import CULL_FREE_OPS, FLOP_COUNTERS, _odd_size

pytestmark = pytest.mark.gpu

TOL = 1e-5
DPI = 24
SCENES = scenes.shading_scenes(DPI)
NAMES = sorted(SCENES)
_scenes, _oracle = {}, {}


def _scene(rt, name):
    if name not in _scenes:
        _scenes[name] = scenes.shading_load(rt, name, SCENES[name])
    return _scenes[name]


def _ref(rt, name, mode):
    """The oracle's frame and stats of a scene, computed once per module."""
    if (name, mode) not in _oracle:
        sc = _scene(rt, name)
        _oracle[name, mode] = rt.oracle_render(sc, sc.width, sc.height, mode, threads=8)
    return _oracle[name, mode]


def _max_diff(fb, ref):
    """Largest |d| over the finite values, after requiring the non-finite ones
    to be the same kind (+inf, -inf, NaN) in the same place."""
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(fb), fin), "non-finite values in different places"
    assert np.array_equal(fb[~fin], ref[~fin], equal_nan=True), "non-finite values of another kind"
    return float(np.abs(fb[fin] - ref[fin]).max()) if fin.any() else 0.0


def _check(rt, sc, mode, ref, ost, flags=0, what=""):
    W, H = sc.width, sc.height
    st = rt.Stats()
    fb = rt.Tracer(sc, W, H, mode, flags=flags).render(st)
    d = _max_diff(fb, ref)
    print(f"  {what} {W}x{H} mode={mode} kernel {rt.kernel_name(sc, mode, flags)[1]} max|d|={d:.3g} "
          f"non-finite {int((~np.isfinite(ref)).sum())} rays=({st.rays_intersect},{st.rays_occluded})")
    assert d <= TOL
    assert (st.rays_intersect, st.rays_occluded) == (ost.rays_intersect, ost.rays_occluded)
    if mode == 1:
        assert np.array_equal(fb, ref, equal_nan=True), "paper mode must be bit-exact"
    return fb, st


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", [0, 1])
def test_shading_scene_matches_oracle(gpu, name, mode):
    ref, ost = _ref(gpu, name, mode)
    _check(gpu, _scene(gpu, name), mode, ref, ost, what=name)


def _ops(rt, st):
    return {n: int(st.ops[i]) for i, n in enumerate(rt.OP_NAMES)}


def _is_eager(rt, sc):
    # eager (transform-inside-CSG) programs re-run once for the winner: only the
    # shading counters are the reference's own there (test_gpu_parity.py)
    return rt.kernel_name(sc, 0)[1].startswith("rtd::k_std<true")


@pytest.mark.parametrize("name", NAMES)
def test_unculled_opcounts_match_oracle(gpu, name):
    rt = gpu
    sc = _scene(rt, name)
    ref, ost = _ref(rt, name, 0)
    st = rt.Stats()
    fb = rt.Tracer(sc, sc.width, sc.height, 0, flags=rt.RT_FLAG_COUNT_OPS | rt.RT_FLAG_NO_CULL).render(st)
    assert _max_diff(fb, ref) <= TOL
    g, o = _ops(rt, st), _ops(rt, ost)
    counters = CULL_FREE_OPS if _is_eager(rt, sc) else FLOP_COUNTERS
    print(f"  {name}: " + " ".join(f"{n}={g[n]}" for n in CULL_FREE_OPS))
    assert {n: g[n] for n in counters} == {n: o[n] for n in counters}
    assert (st.rays_intersect, st.rays_occluded) == (ost.rays_intersect, ost.rays_occluded)


@pytest.mark.parametrize("name", NAMES)
def test_culled_counts_and_frames_match_unculled(gpu, name):
    """Culling changes neither the frame (byte for byte, with and without the
    counting kernels) nor the cull-independent counters."""
    rt = gpu
    sc = _scene(rt, name)
    W, H = sc.width, sc.height
    s0, s1 = rt.Stats(), rt.Stats()
    a = rt.Tracer(sc, W, H, 0, flags=rt.RT_FLAG_COUNT_OPS).render(s0)
    b = rt.Tracer(sc, W, H, 0, flags=rt.RT_FLAG_COUNT_OPS | rt.RT_FLAG_NO_CULL).render(s1)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    for op in CULL_FREE_OPS:
        k = rt.OP_NAMES.index(op)
        assert s0.ops[k] == s1.ops[k], (op, s0.ops[k], s1.ops[k])
    assert (s0.rays_intersect, s0.rays_occluded) == (s1.rays_intersect, s1.rays_occluded)
    for mode in (0, 1):
        c = rt.Tracer(sc, W, H, mode).render()
        d = rt.Tracer(sc, W, H, mode, flags=rt.RT_FLAG_NO_CULL).render()
        assert np.array_equal(c.view(np.uint64), d.view(np.uint64)), mode
        if mode == 0:
            assert np.array_equal(a.view(np.uint64), c.view(np.uint64))


ODD = ["lights65_wave", "lights65_csg", "lights65_xform", "near_light_wave", "near_light_bvh", "media_wave",
       "media_csg"]


@pytest.mark.parametrize("name", ODD)
@pytest.mark.parametrize("mode", [0, 1])
def test_shading_partial_waves_match_oracle(gpu, name, mode):
    rt = gpu
    base = rt.load_scene_from_json_text(_odd_size(json.dumps(SCENES[name]), 55, 25))
    sc = scenes.shading_apply(rt, base, *scenes.shading_patch_indices(rt, base, name))
    assert (sc.width, sc.height) == (55, 25)
    ref, ost = rt.oracle_render(sc, 55, 25, mode, threads=8)
    _check(rt, sc, mode, ref, ost, what=name + " (odd size)")


@pytest.mark.parametrize("name", ["null_mat_few", "null_mat_csg"])
def test_query_reports_null_material_hits(gpu, name):
    """rt_query_intersect on a hit without a material: hit_mask 1, mat -1 and
    the hit's own t, p, n (a miss: hit_mask 0, mat -1, zeros)."""
    rt = gpu
    sc = _scene(rt, name)
    rec = rt.oracle_primary_hits(sc)
    eye = np.array(sc.desc.camera.eye[:])
    got = rt.query_intersect(sc, np.broadcast_to(eye, rec["d"].shape), rec["d"])
    assert np.array_equal(got.hit, rec["hit"])
    null = rec["hit"] & (rec["mat"] == -1)
    assert null.sum() >= 32 and (~rec["hit"]).sum() >= 32
    h = rec["hit"]
    assert np.array_equal(got.mat[h], rec["mat"][h]) and np.array_equal(got.front_face[h], rec["front_face"][h])
    assert np.all(got.mat[null] == -1) and np.all(got.hit[null])
    rel = lambda a, b: float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())
    print(f"  {name}: {int(null.sum())} null-material hits, t {rel(got.t[h], rec['t'][h]):.3g} "
          f"p {rel(got.p[h], rec['p'][h]):.3g} n {float(np.abs(got.n[h] - rec['n'][h]).max()):.3g}")
    assert rel(got.t[h], rec["t"][h]) <= TOL and rel(got.p[h], rec["p"][h]) <= TOL
    assert float(np.abs(got.n[h] - rec["n"][h]).max()) <= TOL
    miss = got.records[~h]
    assert np.all(miss["mat"] == -1) and not miss["t"].any() and not miss["p"].any() and not miss["n"].any()
