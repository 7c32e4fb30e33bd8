"""Degenerate leaf parameters and non-finite rays on the GPU: the scenes of
scenes.leaf_cases and scenes.leaf_scene (test_leaf_scenes.SEEDS) as frames in
both modes, batched intersect / occluded / radiance / shading queries, and the
ray groups of scenes.odd_ray_groups through all four queries.
tests/test_leaf_scenes.py shows on the CPU that the cases do what their names
say, pins the oracle to the reference on them (tests/golden/leaves.npz,
leaf_seeds.npz, leaf_rays.npz) and counts the oracle's own unstable rays.

Bars (unchanged): frames |fb - oracle| <= 1e-5 per channel with identical
Scene::intersect / Scene::occluded counts, paper mode array_equal, the same
against the fixture; queries through test_gpu_query's check_hits /
check_occluded (1 % cap), radiance through test_gpu_radiance's check (15 of
768), shading through test_gpu_shade's check; everything byte-identical to its
RT_FLAG_NO_CULL run, and on the bvh layouts to RT_FLAG_NO_BVH and
RT_FLAG_FORCE_BVH.

Non-finite rays (rt.h, the ray-query contract): the hit flag, mat and
front_face equal the oracle's, each of t, p, n, rgb is NaN where the oracle's
is NaN, the same infinity where it is infinite and within the bar where it is
finite, occluded and the radiance ray counts are equal, and no ray is left
out.  Each group runs alone and interleaved lane by lane with the case's
ordinary rays: the ordinary lanes' records are the bytes of the batch without
the odd lanes, and the reverse.

Measured on an MI355X (profiles/leaf_edges/gpu_tests.txt): all 62 frames
equal to the oracle's and the fixture's (max|d| = 0), every hit record equal
in t, p and n, radiance within 2.9e-9, shading within 1.11e-16, one ray left
out in all (a radiance ray, oracle-unstable), none of the odd groups'.  Before
pow_spec's overflow rule in the shading-query kernels the wo +inf, -inf and
1e200 groups of test_odd_hits_shade failed (profiles/leaf_edges/before_fix.txt).

Every test prints its largest difference, its left-out count and the kernel
rows that ran."""
import numpy as np
import pytest

import scenes
import test_gpu_radiance as R
import test_gpu_shade as S
from test_gpu_query import (case, check_hits, check_hits_every_ray, check_occluded, q_isect, q_occl, same_value)
from test_leaf_scenes import (KEYS, NAMED, gold, leaf_case, leaf_ref, leaf_shade_ref, load, odd_groups, odd_hits,
                              odd_scene, oracle_frame)

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _bvh(key):
    return scenes.LEAF_LAYOUT.get(key) == "bvh"


def _logged(rt, fn):
    rt.launch_log(True)
    try:
        out = fn()
        rows = rt.launch_log_get()
    finally:
        rt.launch_log(False)
    return out, rows


def _render(rt, sc, mode, flags=0):
    st = rt.Stats()
    fb, rows = _logged(rt, lambda: rt.Tracer(sc, sc.width, sc.height, mode, flags=flags).render(st))
    return fb, (int(st.rays_intersect), int(st.rays_occluded)), rows


def _same_hits(a, b):
    return a.records.tobytes() == b.records.tobytes() and np.array_equal(a.hit, b.hit)


# --------------------------------------------------------------------- frames
@pytest.mark.parametrize("key", KEYS)
def test_frames(gpu, key):
    z = gold(key)
    for mode in (0, 1):
        ref, counts = oracle_frame(gpu, key, mode)
        fb, got_counts, rows = _render(gpu, load(gpu, key), mode)
        # (the oracle's frames are finite, tests/test_leaf_scenes.py; a NaN pixel would show as nan here)
        assert np.isfinite(fb).all(), key
        err = float(np.abs(fb - ref).max())
        err_gold = float(np.abs(fb - z[f"{key}/{mode}/fb"]).max())
        print(f"  {key} mode {mode}: {fb.shape[1]}x{fb.shape[0]} max|d|={err:.3g} (fixture {err_gold:.3g}) "
              f"rays {got_counts} oracle {counts} left out 0 rows {rows}")
        assert fb.shape == (36, 48, 3)
        assert got_counts == counts == tuple(int(v) for v in z[f"{key}/{mode}/counts"])
        if mode == 1:
            assert np.array_equal(fb, ref, equal_nan=True) and np.array_equal(fb, z[f"{key}/{mode}/fb"], equal_nan=True)
        else:
            assert np.isfinite(fb).all() and err <= TOL and err_gold <= TOL
        if key in scenes.LEAF_EAGER_CASES:
            assert all(r.split("<")[1].split(",")[0] == "true" for r in rows if "k_paper_finish" not in r), (key, rows)
        elif key in NAMED:
            wv = ("few", "wave", "bvh").index(scenes.LEAF_LAYOUT[key])
            # (the trace kernel's wave-cull argument: 0 none, 1 wave culls, 2 the wave BVH; the general
            # k_std has no such argument in its name)
            trace = [r for r in rows if "k_paper_finish" not in r and "rtd::k_std<" not in r]
            assert all(r.split("<")[1].split(",")[1].strip() == str(wv) for r in trace), (key, rows)
        for f in (gpu.RT_FLAG_NO_CULL,) + ((gpu.RT_FLAG_NO_BVH, gpu.RT_FLAG_FORCE_BVH) if _bvh(key) else ()):
            other, other_counts, _ = _render(gpu, load(gpu, key), mode, f)
            assert np.array_equal(fb, other, equal_nan=True) and other_counts == counts, (key, f)


# ------------------------------------------------------ intersect and occluded
@pytest.mark.parametrize("key", KEYS)
def test_intersect_and_occluded(gpu, key):
    c = leaf_case(gpu, key)
    (got, occ), rows = _logged(gpu, lambda: (q_isect(gpu, c.scene, c.rays), q_occl(gpu, c.scene, c.seg_rays)))
    check_hits(c, c.rays, got, c.ref_hit, c.ref_rec, key + " intersect")
    check_occluded(c, c.seg_rays, occ, c.ref_occ, key + " occluded")
    print(f"  {key} rows {rows}")
    assert c.ref_hit.sum() >= len(c.rays) // 4 and c.ref_occ.any() and len(rows) == 2
    for f in (gpu.RT_FLAG_NO_CULL,) + ((gpu.RT_FLAG_NO_BVH, gpu.RT_FLAG_FORCE_BVH) if _bvh(key) else ()):
        assert _same_hits(got, q_isect(gpu, c.scene, c.rays, flags=f)), (key, f)
        assert np.array_equal(occ, q_occl(gpu, c.scene, c.seg_rays, flags=f)), (key, f)


# ------------------------------------------------------------------- radiance
@pytest.mark.parametrize("key", KEYS)
def test_radiance(gpu, key):
    r = leaf_ref(gpu, key)
    sa, sb = gpu.Stats(), gpu.Stats()
    got, rows = _logged(gpu, lambda: gpu.query_radiance(r.sc, r.o, r.d, stats=sa))
    R.check(gpu, r, got, key + " radiance")
    print(f"  {key} rows {rows}")
    assert (np.abs(r.rgb - r.background).max(axis=1) > 0).sum() >= len(r) // 4 and len(rows) == 1
    nc = gpu.query_radiance(r.sc, r.o, r.d, gpu.RT_FLAG_NO_CULL, sb)
    assert got.tobytes() == nc.tobytes(), key
    assert (sa.rays_intersect, sa.rays_occluded) == (sb.rays_intersect, sb.rays_occluded), key


# -------------------------------------------------------------------- shading
@pytest.mark.parametrize("key", NAMED)
def test_shading_of_the_hits(gpu, key):
    r = leaf_shade_ref(gpu, key)
    got, rows = _logged(gpu, lambda: S.shade(gpu, r))
    S.check(gpu, r, got, key + " shade")
    print(f"  {key} rows {rows}")
    assert r.hit.sum() >= len(r) // 4
    assert got.tobytes() == S.shade(gpu, r, flags=gpu.RT_FLAG_NO_CULL).tobytes(), key


# ----------------------------------------- non-finite and overflowing rays
def _ordinary(gpu, name):
    """The scene's test_gpu_query.Case (or LeafCase): its scene handle and ordinary rays."""
    return leaf_case(gpu, name[5:]) if name.startswith("leaf/") else case(gpu, name)


def _interleave(a, b):
    m = min(len(a), len(b))
    mix = np.empty(2 * m, dtype=a.dtype)
    mix[0::2], mix[1::2] = a[:m], b[:m]
    return mix, m


@pytest.mark.parametrize("name", scenes.ODD_RAY_SCENES)
def test_odd_rays_intersect_and_occluded(gpu, name):
    c = _ordinary(gpu, name)
    sc = c.scene
    plain_hits, plain_occ = q_isect(gpu, sc, c.rays), q_occl(gpu, sc, c.seg_rays)
    nonfinite = 0
    for tag, rays in odd_groups(gpu, name).items():
        what = f"{name} {tag}"
        ref_hit, ref_rec = gpu.oracle_scene_intersect(odd_scene(gpu, name), rays)
        ref_occ = gpu.oracle_occluded(odd_scene(gpu, name), rays["o"], rays["d"], rays["tmin"], rays["tmax"])
        (got, occ), rows = _logged(gpu, lambda: (q_isect(gpu, sc, rays), q_occl(gpu, sc, rays)))
        check_hits_every_ray(rays, got, ref_hit, ref_rec, what)
        nonfinite += int((ref_hit & ~np.isfinite(ref_rec["t"])).sum())
        print(f"  {what}: {int(ref_occ.sum())} occluded, rows {rows}")
        assert np.array_equal(occ, ref_occ), (what, np.flatnonzero(occ != ref_occ)[:8])
        for f in (gpu.RT_FLAG_NO_CULL,) + ((gpu.RT_FLAG_NO_BVH, gpu.RT_FLAG_FORCE_BVH) if name == "bvh/ties" else ()):
            assert _same_hits(got, q_isect(gpu, sc, rays, flags=f)), (what, f)
            assert np.array_equal(occ, q_occl(gpu, sc, rays, flags=f)), (what, f)
        # interleaved with ordinary rays, lane by lane
        mix, m = _interleave(rays, c.rays)
        mix_seg, _ = _interleave(rays, c.seg_rays)
        both, both_occ = q_isect(gpu, sc, mix), q_occl(gpu, sc, mix_seg)
        assert both.records[0::2].tobytes() == got.records[:m].tobytes() and np.array_equal(both.hit[0::2], got.hit[:m]), what
        assert both.records[1::2].tobytes() == plain_hits.records[:m].tobytes(), what
        assert np.array_equal(both.hit[1::2], plain_hits.hit[:m]), what
        assert np.array_equal(both_occ[0::2], occ[:m]) and np.array_equal(both_occ[1::2], plain_occ[:m]), what
    # hits with t = NaN do come back, where the scene's last objects are leaves (a CSG rejects a NaN range)
    assert nonfinite >= 64 or name == "torture/halfspace_in_csg"


def _odd_radiance_groups(gpu, name):
    """The groups that differ for a radiance query (tmin / tmax play no part in it)."""
    return {tag: rays for tag, rays in odd_groups(gpu, name).items() if not tag.startswith(("tmin", "tmax", "both"))}


@pytest.mark.parametrize("name", scenes.ODD_RAY_SCENES)
def test_odd_rays_radiance(gpu, name):
    """Against rtamd.oracle_trace_rays: Tracer::trace(Ray(o, d)) with the ray
    built once (through oracle_trace's camera an infinite direction would be
    normalised twice, into (0, 1, 0))."""
    c = _ordinary(gpu, name)
    sc = c.scene
    plain_o, plain_d = np.ascontiguousarray(c.rays["o"]), np.ascontiguousarray(c.rays["d"])
    plain = gpu.query_radiance(sc, plain_o, plain_d)
    for tag, rays in _odd_radiance_groups(gpu, name).items():
        what = f"{name} {tag} radiance"
        o, d = np.ascontiguousarray(rays["o"]), np.ascontiguousarray(rays["d"])
        rgb, ni, no = gpu.oracle_trace_rays(odd_scene(gpu, name), o, d)
        st, st_nc = gpu.Stats(), gpu.Stats()
        got, rows = _logged(gpu, lambda: gpu.query_radiance(sc, o, d, stats=st))
        ok = same_value(got, rgb, TOL, relative=False).all(axis=1)
        fin = np.isfinite(rgb).all(axis=1)
        mx = float(np.abs(got[fin] - rgb[fin]).max(initial=0.0))
        print(f"  {what}: {len(o)} rays, {int((~fin).sum())} non-finite, max|d|={mx:.3g}, left out 0, oracle counts "
              f"({int(ni.sum())}, {int(no.sum())}) rows {rows}")
        assert ok.all(), (what, np.flatnonzero(~ok)[:8], got[~ok][:2], rgb[~ok][:2])
        assert (st.rays_intersect, st.rays_occluded) == (int(ni.sum()), int(no.sum())), what
        nc = gpu.query_radiance(sc, o, d, gpu.RT_FLAG_NO_CULL, st_nc)
        assert got.tobytes() == nc.tobytes(), what
        assert (st_nc.rays_intersect, st_nc.rays_occluded) == (st.rays_intersect, st.rays_occluded), what
        m = len(o)
        mo, md = np.empty((2 * m, 3)), np.empty((2 * m, 3))
        mo[0::2], mo[1::2], md[0::2], md[1::2] = o, plain_o[:m], d, plain_d[:m]
        both = gpu.query_radiance(sc, mo, md)
        assert both[0::2].tobytes() == got.tobytes() and both[1::2].tobytes() == plain[:m].tobytes(), what


@pytest.mark.parametrize("name", scenes.ODD_RAY_SCENES)
def test_odd_hits_shade(gpu, name):
    """rt_query_shade of hits with non-finite (and overflowing) fields under
    hit_mask = 1: scenes.odd_hit_groups of the hits of the scene's 64 base
    rays, which tests/test_leaf_scenes.py holds to the reference's own
    shade_lambert_phong."""
    sc = _ordinary(gpu, name).scene
    osc, groups = odd_hits(gpu, name)
    H0, wo0 = groups["wo 1e200"][0], groups["wo 1e200"][1] / 1e200   # (the ordinary hits themselves)
    n = len(H0)
    plain = gpu.query_shade(sc, H0, wo0)
    for tag, (H, wo) in groups.items():
        what = f"{name} hits with {tag}"
        rgb, no = gpu.oracle_shade(osc, H, wo)
        st = gpu.Stats()
        got, rows = _logged(gpu, lambda: gpu.query_shade(sc, H, wo, np.ones(n, dtype=np.uint8), stats=st))
        # 1e-5 absolute, as everywhere; a colour beyond shading's own cap of 1.5 (a finite power above 1: wo x10
        # reaches -1e290) is judged relative to its size, as this suite judges t and p
        with np.errstate(invalid="ignore"):
            size = np.where(np.isfinite(rgb) & (np.abs(rgb) > 1.5), np.abs(rgb), 1.0)
        ok = same_value(got / size, rgb / size, TOL, relative=False).all(axis=1)
        fin = np.isfinite(rgb).all(axis=1)
        mx = float((np.abs(got[fin] - rgb[fin]) / size[fin]).max(initial=0.0))
        print(f"  {what}: {n} hits, {int((~fin).sum())} non-finite, max|d|={mx:.3g}, left out 0, oracle count "
              f"{int(no.sum())} rows {rows}")
        assert ok.all(), (what, np.flatnonzero(~ok)[:8], got[~ok][:2], rgb[~ok][:2])
        assert (st.rays_intersect, st.rays_occluded) == (0, int(no.sum())), what
        assert got.tobytes() == gpu.query_shade(sc, H, wo, flags=gpu.RT_FLAG_NO_CULL).tobytes(), what
        mixH, m = _interleave(H, H0)
        mixw = np.empty((2 * m, 3))
        mixw[0::2], mixw[1::2] = wo, wo0
        both = gpu.query_shade(sc, mixH, mixw)
        assert both[0::2].tobytes() == got.tobytes() and both[1::2].tobytes() == plain.tobytes(), what


def test_zero_radius_centre_hits_are_shaded_as_the_oracle_shades_them(gpu):
    """Finite rays whose hit has a NaN normal (through the centre of the
    radius-0 sphere): intersect on the device, then shade its own output."""
    name = "leaf/radius_edges_wave"
    c = _ordinary(gpu, name)
    rays = odd_groups(gpu, name)["zero radius centre"]
    got = q_isect(gpu, c.scene, rays)
    assert got.hit.all() and np.isnan(got.records["n"]).any(axis=1).all() and np.isfinite(got.records["p"]).all()
    wo = -rays["d"]
    rgb, no = gpu.oracle_shade(c.scene, got.records, wo)
    st = gpu.Stats()
    out = gpu.query_shade(c.scene, got.records, wo, got.hit.astype(np.uint8), stats=st)
    ok = same_value(out, rgb, TOL, relative=False).all(axis=1)
    print(f"  {name} zero radius centre shade: {len(rays)} hits, {int((~np.isfinite(rgb)).any(axis=1).sum())} non-finite, "
          f"oracle count {int(no.sum())}, left out 0")
    assert ok.all(), (out[~ok][:2], rgb[~ok][:2])
    assert st.rays_occluded == int(no.sum())
    assert out.tobytes() == gpu.query_shade(c.scene, got.records, wo, flags=gpu.RT_FLAG_NO_CULL).tobytes()
