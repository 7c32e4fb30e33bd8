"""The wave BVH and the ray BVH on the GPU on the forest scenes
(scenes.forest_cases: more than 256 top-level objects of mixed compiled forms,
at the edges of the wave list and the ray tree): frames in both modes, batched
queries and radiance, each against the CPU oracle at the existing files' bars,
against its own runs under the BVH and cull flags bit for bit, and under three
placements.

tests/test_forest_scenes.py shows what the scenes reach (transform chains,
folds, prefilter balls and cull groups inside a wave list; a second and a
third 64-chunk round of every chunk test; two unbounded chunks; none), pins
the oracle to the reference on them (tests/golden/forest.npz) and counts the
oracle's own unstable rays.

Bars (unchanged): frames |fb - oracle| <= 1e-5 per channel with identical
Scene::intersect / Scene::occluded counts, paper mode array_equal, the same
against forest.npz; queries through test_gpu_query's check_hits /
check_occluded (1 % cap), radiance through test_gpu_radiance's check (15 of
768); every flagged run byte-identical with equal counts.  The placements
compare the device with itself only.

Measured on an MI355X (profiles/forest_scenes/gpu_tests.txt): all 36 frames
equal to the oracle's and the fixture's (max|d| = 0 in standard mode too);
every hit record of the 18 intersect batches equal to the oracle's, t, p and n
included; radiance within 1.2e-11; no ray had to be left out anywhere.  Before
the overflow rule of cone_touch_t (rt_device.hpp) the two frames of
nonfinite_bounds failed (profiles/forest_scenes/before_fix.txt): off by 0.52,
26024 occlusion queries for the oracle's 26126, a sphere of radius 1e19 at
5.9e19 culled from the bundle that saw it.

Every test prints its largest difference and its left-out count."""
import numpy as np
import pytest

import scenes
import test_gpu_radiance as R
from test_forest_scenes import (KEYS, RADIANCE_KEYS, ROWS, TREE_KEYS, forest_case, forest_ref, fresh, gold, oracle_frame,
                                scene_dict)
from test_gpu_bounce import _differing, _full_trace
from test_gpu_bvh import _wv
from test_gpu_node_query import logged
from test_gpu_query import check_hits, check_occluded, q_isect, q_occl
from test_gpu_ray_bvh import F, both
from test_leaf_scenes import odd_base_rays
from test_placed_scenes import PL, load as load_dict, map_rays, placed_any_scale

pytestmark = pytest.mark.gpu

TOL = 1e-5
PLACEMENTS = ("far", "huge_far", "e39")


def _render(rt, sc, mode, flags=0):
    """A frame of a new Tracer: (fb, counts, launch log)."""
    st = rt.Stats()
    t = rt.Tracer(sc, sc.width, sc.height, mode, flags=flags)
    fb, rows = logged(rt, lambda: t.render(st))
    return fb, (int(st.rays_intersect), int(st.rays_occluded)), rows


def _ran(row, rows):
    """The host's row is in the launch log (a paper frame's launch may be the timed twin of its row)."""
    return row in rows or scenes.row_timed(row, True) in rows


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _counts(st):
    return (st.rays_intersect, st.rays_occluded, st.rays_traced, st.n_gpus)


def _bvh_args(rt, sc):
    """The template arguments of the scene's ray-BVH rows, or None where RT_FLAG_RAY_BVH keeps the flat rows."""
    rc, name = rt.ray_bvh_kernel_name(sc, 0, F(rt))
    assert rc == 0, rt.last_error()
    return name.split("<", 1)[1].rstrip(">") if "_bvh<" in name else None


# --------------------------------------------------------------------- frames
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("key", KEYS)
def test_frames(gpu, key, mode):
    """The forced-BVH frame against the oracle and the fixture; the launch log
    holds the row the host names; the RT_FLAG_NO_BVH and RT_FLAG_NO_CULL
    frames and four unflagged frames in a row (across the BVH on/off trial)
    are that frame, with its counts."""
    z = gold()
    ref, counts = oracle_frame(gpu, key, mode)
    sc = fresh(gpu, key)
    rc, row = gpu.kernel_name(sc, mode, gpu.RT_FLAG_FORCE_BVH)
    assert rc == 0 and (key not in ROWS or row == ROWS[key][mode]), (key, row)
    fb, got_counts, rows = _render(gpu, sc, mode, gpu.RT_FLAG_FORCE_BVH)
    with np.errstate(invalid="ignore"):
        err = float(np.nanmax(np.abs(fb - ref)))
        err_gold = float(np.nanmax(np.abs(fb - z[f"{key}/{mode}/fb"])))
    print(f"  {key} mode {mode}: {fb.shape[1]}x{fb.shape[0]} max|d|={err:.3g} (fixture {err_gold:.3g}) "
          f"rays {got_counts} oracle {counts} rows {rows}")
    assert _ran(row, rows), (key, row, rows)
    if key in TREE_KEYS and key != "mixed320+sun":   # (a directional light: the general kernels, no list)
        assert _wv(row) == "2" and _wv(gpu.kernel_name(sc, mode, gpu.RT_FLAG_NO_BVH)[1]) == "1", row
    assert got_counts == counts == tuple(int(v) for v in z[f"{key}/{mode}/counts"])
    if mode == 1:
        assert _same(fb, ref) and _same(fb, z[f"{key}/{mode}/fb"])
    else:
        assert np.isfinite(fb).all() and err <= TOL and err_gold <= TOL
    for flag in (gpu.RT_FLAG_NO_BVH, gpu.RT_FLAG_NO_CULL):
        other, other_counts, other_rows = _render(gpu, sc, mode, flag)
        assert _same(fb, other) and other_counts == counts, (key, flag)
        assert _ran(gpu.kernel_name(sc, mode, flag)[1], other_rows), (key, flag, other_rows)
    t = gpu.Tracer(sc, sc.width, sc.height, mode)
    for i in range(4):
        st = gpu.Stats()
        assert _same(t.render(st), fb), (key, i)
        assert (int(st.rays_intersect), int(st.rays_occluded)) == counts, (key, i)


def test_counting_frame_is_the_plain_one(gpu):
    sc = fresh(gpu, "mixed320")
    a, ca, _ = _render(gpu, sc, 0, gpu.RT_FLAG_FORCE_BVH)
    b, cb, rows = _render(gpu, sc, 0, gpu.RT_FLAG_FORCE_BVH | gpu.RT_FLAG_COUNT_OPS)
    print(f"  mixed320 counting frame: rows {rows}, counts {cb}")
    assert ca == cb and _same(a, b)
    c, cc, _ = _render(gpu, sc, 0, gpu.RT_FLAG_COUNT_OPS)
    assert cc == ca and _same(a, c)


# ------------------------------------------------------ intersect and occluded
def _queries(gpu, c, rays, segs, what, ref=None):
    """The flat, RT_FLAG_RAY_BVH and RT_FLAG_NO_CULL calls of both queries:
    equal bytes and stats, `_bvh<` rows exactly where the scene has a tree;
    with ref = (hit, rec, occ) also the flat answers against the oracle."""
    sc = c.scene
    args = _bvh_args(gpu, sc)
    h, o = both(gpu, sc, rays, segs, want_row=args)
    if args is None:
        _, rows = logged(gpu, lambda: (q_isect(gpu, sc, rays, F(gpu)), q_occl(gpu, sc, segs, F(gpu))))
        assert rows == [gpu.query_kernel_name(sc, 0)[1], gpu.query_kernel_name(sc, 1)[1]], rows
        assert not any("_bvh<" in r for r in rows)
    s0, s1, t0, t1 = gpu.Stats(), gpu.Stats(), gpu.Stats(), gpu.Stats()
    flat_h, flat_o = q_isect(gpu, sc, rays, 0, s0), q_occl(gpu, sc, segs, 0, t0)
    nc_h = q_isect(gpu, sc, rays, gpu.RT_FLAG_NO_CULL, s1)
    nc_o = q_occl(gpu, sc, segs, gpu.RT_FLAG_NO_CULL, t1)
    assert flat_h.records.tobytes() == h.records.tobytes() == nc_h.records.tobytes(), what
    assert np.array_equal(flat_h.hit, h.hit) and np.array_equal(flat_h.hit, nc_h.hit), what
    assert np.array_equal(flat_o, o) and np.array_equal(flat_o, nc_o), what
    assert _counts(s0) == _counts(s1) and _counts(t0) == _counts(t1), what
    if ref is not None:
        check_hits(c, rays, flat_h, ref[0], ref[1], what + " intersect")
        check_occluded(c, segs, flat_o, ref[2], what + " occluded")
    return flat_h, flat_o


@pytest.mark.parametrize("key", KEYS)
def test_intersect_and_occluded(gpu, key):
    c = forest_case(gpu, key)
    assert (_bvh_args(gpu, c.scene) is not None) == (key in TREE_KEYS)
    _queries(gpu, c, c.rays, c.seg_rays, key, (c.ref_hit, c.ref_rec, c.ref_occ))
    assert c.ref_hit.sum() >= len(c.rays) // 4 and c.ref_occ.any()


@pytest.mark.parametrize("key", ("mixed320", "floors70"))
def test_odd_rays(gpu, key):
    """Every group of scenes.odd_ray_groups alone and interleaved one in eight
    with ordinary rays: flat, RT_FLAG_RAY_BVH and RT_FLAG_NO_CULL agree in
    bytes, and the ordinary rays' bytes are theirs in a batch without the odd
    ones."""
    c = forest_case(gpu, key)
    ob, db = odd_base_rays(gpu, c.scene)
    plain = c.rays[:448].copy()          # 7 ordinary rays per odd one
    h_plain, o_plain = _queries(gpu, c, plain, plain, key)
    n = 0
    for tag, (o, d, tmin, tmax) in scenes.odd_ray_groups(ob, db).items():
        odd = gpu.make_rays(o, d, tmin, tmax)
        _queries(gpu, c, odd, odd, f"{key} {tag}")
        mixed = np.empty(512, dtype=plain.dtype)
        is_odd = np.arange(512) % 8 == 3
        mixed[is_odd], mixed[~is_odd] = odd, plain
        h, oc = _queries(gpu, c, mixed, mixed, f"{key} {tag} mixed")
        assert h.records[~is_odd].tobytes() == h_plain.records.tobytes(), tag
        assert np.array_equal(h.hit[~is_odd], h_plain.hit) and np.array_equal(oc[~is_odd], o_plain), tag
        n += 1
    print(f"  {key}: {n} odd ray groups alone and interleaved, flat = ray BVH = no cull; max difference 0, left out 0")


# ------------------------------------------------------------------- radiance
@pytest.mark.parametrize("key", RADIANCE_KEYS)
def test_radiance(gpu, key):
    r = forest_ref(gpu, key)
    sa, sb = gpu.Stats(), gpu.Stats()
    got, rows = logged(gpu, lambda: gpu.query_radiance(r.sc, r.o, r.d, stats=sa))
    print(f"  {key} radiance rows {rows}")
    R.check(gpu, r, got, key + " radiance")
    assert (np.abs(r.rgb - r.background).max(axis=1) > 0).sum() >= len(r) // 4
    assert len(rows) == 1 and rows[0] == gpu.radiance_kernel_name(r.sc)[1], rows
    nc = gpu.query_radiance(r.sc, r.o, r.d, gpu.RT_FLAG_NO_CULL, sb)
    assert got.tobytes() == nc.tobytes(), key
    assert (sa.rays_intersect, sa.rays_occluded) == (sb.rays_intersect, sb.rays_occluded), key


def test_bounce_loop_is_the_radiance_query(gpu):
    c = forest_case(gpu, "mixed320")
    n = len(c.rays)
    d_rays = gpu.DeviceBuffer(64 * n)
    d_rays.from_host(c.rays)
    want, wst = _full_trace(gpu, c.scene, d_rays, n, 0)
    d_rgb, sizes, st = gpu.radiance_bounces_device(c.scene, d_rays, n, 0)
    got = d_rgb.to_host()[:3 * n].reshape(n, 3)
    print(f"  mixed320 bounce loop: levels {sizes}, rays ({st.rays_intersect}, {st.rays_occluded}), "
          f"{_differing(got, want)} colours differ")
    assert _differing(got, want) == 0
    assert (st.rays_intersect, st.rays_occluded) == (wst.rays_intersect, wst.rays_occluded)
    assert len(sizes) >= 2   # (the batch does reflect or refract)


# ----------------------------------------------------------------- placements
@pytest.mark.parametrize("pl", PLACEMENTS)
def test_placements(gpu, pl):
    """mixed320 moved and scaled: the device against itself, so no new bar."""
    base = forest_case(gpu, "mixed320")
    scale, offset = PL[pl]
    pc = type("Placed", (), {})()
    pc.scene = load_dict(gpu, placed_any_scale(scene_dict("mixed320"), scale, offset))
    assert _bvh_args(gpu, pc.scene) is not None
    h, o = _queries(gpu, pc, map_rays(base.rays, scale, offset), map_rays(base.seg_rays, scale, offset), f"mixed320 {pl}")
    print(f"  mixed320 {pl}: {int(h.hit.sum())} hits (unplaced {int(base.ref_hit.sum())}), {int(o.sum())} occluded "
          f"(unplaced {int(base.ref_occ.sum())}); flat = ray BVH = no cull")
    assert h.hit.any()
    if pl != "far":
        return
    sc = load_dict(gpu, scenes.placed(scene_dict("mixed320"), scale, offset))
    for mode in (0, 1):
        fb, counts, rows = _render(gpu, sc, mode, gpu.RT_FLAG_FORCE_BVH)
        for flag in (gpu.RT_FLAG_NO_BVH, gpu.RT_FLAG_NO_CULL):
            other, other_counts, _ = _render(gpu, sc, mode, flag)
            assert _same(fb, other) and other_counts == counts, (mode, flag)
        off_bg = int((np.abs(fb - fb[0, 0]).max(axis=2) > 0).sum())
        print(f"  mixed320 far mode {mode}: rows {rows}, counts {counts}, {off_bg} pixels differ from the corner's")
        assert off_bg > fb.shape[0] * fb.shape[1] // 4
