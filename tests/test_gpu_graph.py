"""Every compiled object form on the GPU, on the scene-graph scenes
(scenes.graph_cases, scenes.graph_scene at test_graph_scenes.SEEDS): frames in
both modes, batched queries and radiance, each against the CPU oracle at the
existing files' bars and against its own RT_FLAG_NO_CULL run, bit for bit.

The forms (scene_compile.cpp) decide which interpreter and which culls run in
rt_device.hpp; tests/test_graph_scenes.py shows that these scenes reach every
one of them, pins the oracle to the reference on them (tests/golden/graph.npz)
and counts the oracle's own unstable rays (none for intersect and occluded).

Bars (unchanged): frames |fb - oracle| <= 1e-5 per channel with identical
Scene::intersect / Scene::occluded counts, paper mode array_equal, the same
against graph.npz; queries through test_gpu_query's check_hits /
check_occluded (1 % cap), radiance through test_gpu_radiance's check (15 of
768); the NO_CULL run of everything byte-identical.

Measured on an MI355X (profiles/graph_scenes/gpu_tests.txt): all 40 frames
equal to the oracle's and the fixture's (max|d| = 0 in standard mode too);
every hit record of the 20 intersect batches equal to the oracle's, t, p and n
included; radiance within 2.4e-13 except scale_threshold, 2.2e-7 (under
scaling [1e-6, 1, 1] the reference's sphere test is decided by its last bits,
DESIGN.md Culling); no ray had to be left out anywhere.  Before the bound rule
for such Scalings (scene_compile.cpp xform_ball) 2 cases failed
(profiles/graph_scenes/before_fix.txt): the frames of big_scale_fallback (off
by 0.59, 25194 occlusion queries for the oracle's 41307) and of
scale_threshold (the culled frame 7.9e-9 off the unculled one).

Every test prints its largest difference and its left-out count."""
import numpy as np
import pytest

import scenes
import test_gpu_radiance as R
from test_gpu_query import check_hits, check_occluded, q_isect, q_occl
from test_graph_scenes import KEYS, NAMED, fallback_rays, gold, graph_case, graph_ref, load, oracle_frame

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _render(rt, sc, mode, flags=0):
    """A frame of a fresh handle's first Tracer: (fb, counts, launch log)."""
    st = rt.Stats()
    rt.launch_log(True)
    try:
        fb = rt.Tracer(sc, sc.width, sc.height, mode, flags=flags).render(st)
        rows = rt.launch_log_get()
    finally:
        rt.launch_log(False)
    return fb, (int(st.rays_intersect), int(st.rays_occluded)), rows


def _eager_rows(rows, what):
    """Which of the logged trace / query kernels are eager variants (template argument E, the first)."""
    out = []
    for row in rows:
        name, _, args = row.partition("<")
        kernel = name.split("::")[1]
        if kernel in ("k_std", "k_paper_primary", "k_query_isect", "k_query_occl", "k_radiance"):
            out.append(args.split(",")[0].strip() == "true")
        else:
            assert kernel in ("k_std_lean", "k_std_secw", "k_paper_primary_lean", "k_paper_finish"), (what, row)
            if kernel != "k_paper_finish":
                out.append(False)
    assert out, (what, rows)
    return out


def _has_eager(rt, key):
    return rt.compile_forms(load(rt, key))["obj/eager"] > 0


# --------------------------------------------------------------------- frames
@pytest.mark.parametrize("key", KEYS)
def test_frames(gpu, key):
    """Both modes at the fixture's size against the oracle and the fixture,
    culling on and off; the launch log: an eager kernel variant exactly for
    the scenes with an eager program."""
    z = gold()
    dpi = int(z["dpi"])
    eager = _has_eager(gpu, key)
    if key in NAMED:
        assert eager == (key in scenes.GRAPH_EAGER_CASES)
    for mode in (0, 1):
        ref, counts = oracle_frame(gpu, key, mode)
        fb, got_counts, rows = _render(gpu, load(gpu, key, dpi), mode)
        with np.errstate(invalid="ignore"):
            err = float(np.nanmax(np.abs(fb - ref)))
            err_gold = float(np.nanmax(np.abs(fb - z[f"{key}/{mode}/fb"])))
        print(f"  {key} mode {mode}: {fb.shape[1]}x{fb.shape[0]} max|d|={err:.3g} (fixture {err_gold:.3g}) "
              f"rays {got_counts} oracle {counts} rows {rows}")
        assert got_counts == counts == tuple(int(v) for v in z[f"{key}/{mode}/counts"])
        if mode == 1:
            assert np.array_equal(fb, ref, equal_nan=True) and np.array_equal(fb, z[f"{key}/{mode}/fb"], equal_nan=True)
        else:
            assert np.isfinite(fb).all() and err <= TOL and err_gold <= TOL
        assert _eager_rows(rows, key) == [eager] * len(_eager_rows(rows, key)), (key, rows)
        nc, nc_counts, _ = _render(gpu, load(gpu, key, dpi), mode, gpu.RT_FLAG_NO_CULL)
        assert np.array_equal(fb, nc, equal_nan=True) and nc_counts == counts, key


# ------------------------------------------------------ intersect and occluded
@pytest.mark.parametrize("key", KEYS)
def test_intersect_and_occluded(gpu, key):
    c = graph_case(gpu, key)
    gpu.launch_log(True)
    try:
        got = q_isect(gpu, c.scene, c.rays)
        occ = q_occl(gpu, c.scene, c.seg_rays)
        rows = gpu.launch_log_get()
    finally:
        gpu.launch_log(False)
    check_hits(c, c.rays, got, c.ref_hit, c.ref_rec, key + " intersect")
    check_occluded(c, c.seg_rays, occ, c.ref_occ, key + " occluded")
    assert c.ref_hit.sum() >= len(c.rays) // 4 and c.ref_occ.any()
    assert len(rows) == 2 and _eager_rows(rows, key) == [_has_eager(gpu, key)] * 2, (key, rows)
    nc = q_isect(gpu, c.scene, c.rays, flags=gpu.RT_FLAG_NO_CULL)
    assert got.records.tobytes() == nc.records.tobytes() and np.array_equal(got.hit, nc.hit), key
    assert np.array_equal(occ, q_occl(gpu, c.scene, c.seg_rays, flags=gpu.RT_FLAG_NO_CULL)), key


def test_big_scale_fallback_rays_hit_off_the_image(gpu):
    """The rays the case is there for - oracle hits on the scaled sphere whose
    world line misses the sphere's image, at least 64 of them - get the
    oracle's hit from the device, culling on."""
    c = graph_case(gpu, "big_scale_fallback")
    k = fallback_rays(c)
    got = q_isect(gpu, c.scene, c.rays)
    same = got.hit[k] & (got.records["mat"][k] == c.ref_rec["mat"][k])
    print(f"  big_scale_fallback: {len(k)} rays hit the scaled sphere off its image, the device agrees on {int(same.sum())}")
    assert len(k) >= 64
    assert same.all()


# ------------------------------------------------------------------- radiance
@pytest.mark.parametrize("key", scenes.GRAPH_XFORM_CASES)
def test_radiance(gpu, key):
    r = graph_ref(gpu, key)
    sa, sb = gpu.Stats(), gpu.Stats()
    gpu.launch_log(True)
    try:
        got = gpu.query_radiance(r.sc, r.o, r.d, stats=sa)
        rows = gpu.launch_log_get()
    finally:
        gpu.launch_log(False)
    R.check(gpu, r, got, key + " radiance")
    assert (np.abs(r.rgb - r.background).max(axis=1) > 0).sum() >= len(r) // 4
    assert len(rows) == 1 and _eager_rows(rows, key) == [_has_eager(gpu, key)], (key, rows)
    nc = gpu.query_radiance(r.sc, r.o, r.d, gpu.RT_FLAG_NO_CULL, sb)
    assert got.tobytes() == nc.tobytes(), key
    assert (sa.rays_intersect, sa.rays_occluded) == (sb.rays_intersect, sb.rays_occluded), key
