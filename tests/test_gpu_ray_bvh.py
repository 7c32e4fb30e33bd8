"""Ray queries on the per-ray BVH (RT_FLAG_RAY_BVH, rt_query_bvh_kernels.hpp)
on the GPU: each of the six rows launches, and its hits, masks, occluded bytes
and stats counts are the bytes of the same call without the flag - on exact
ties, deep trees, odd leaves, placed scenes, negative and finite ranges,
non-finite rays and wave tails - and pass tests/test_gpu_query.py's bar
against the oracle.  tests/test_ray_bvh_plan.py holds the tree and the culls
to the oracle on the CPU."""
import ctypes as C
import json

import numpy as np
import pytest

import scenes
from test_gpu_node_query import logged
from test_gpu_query import Case, case, check_hits, check_occluded, q_isect, q_occl
from test_leaf_scenes import odd_base_rays
from test_placed_scenes import PL, load, map_rays, placed_any_scale
from test_ray_bvh_plan import LEAF_BVH, PLACEMENTS, SEED, scene, scene_dict

pytestmark = pytest.mark.gpu

INF = float("inf")
SUN = [([-0.4, -1.0, -0.3], [0.9, 0.85, 0.8])]
ROW_SCENES = {"bvh/ties": "false, false", "bvh/ties+sun": "true, false", "bvh/perf300": "false, true"}
_cases = {}


def F(rt):
    return rt.RT_FLAG_RAY_BVH


def ray_case(rt, name):
    """test_gpu_query.Case (768 incoherent rays, the oracle's answers) of a scene of this file, once."""
    if name == "bvh/ties":
        return case(rt, name)
    if name not in _cases:
        sc = rt.with_dir_lights(scene(rt, "bvh/ties"), SUN) if name == "bvh/ties+sun" else scene(rt, name)
        c = Case.__new__(Case)
        c._build(rt, sc, SEED + 17 + len(_cases), name)
        _cases[name] = c
    return _cases[name]


def both(rt, sc, rays, segs=None, want_row=None):
    """The closest-hit query of `rays` and the occluded query of `segs` (default:
    rays), flat and flagged: asserts equal bytes and stats counts, and the
    flagged launches' rows; returns the flagged (hits, occluded)."""
    segs = rays if segs is None else segs
    s0, s1, t0, t1 = rt.Stats(), rt.Stats(), rt.Stats(), rt.Stats()
    flat_h, flat_o = q_isect(rt, sc, rays, 0, s0), q_occl(rt, sc, segs, 0, t0)
    (h, o), rows = logged(rt, lambda: (q_isect(rt, sc, rays, F(rt), s1), q_occl(rt, sc, segs, F(rt), t1)))
    if want_row is not None:
        assert rows == [f"rtd::k_query_isect_bvh<{want_row}>", f"rtd::k_query_occl_bvh<{want_row}>"], rows
    assert h.records.tobytes() == flat_h.records.tobytes() and np.array_equal(h.hit, flat_h.hit)
    assert np.array_equal(o, flat_o)
    for a, b in ((s0, s1), (t0, t1)):
        assert (a.rays_intersect, a.rays_occluded, a.rays_traced, a.n_gpus) == \
               (b.rays_intersect, b.rays_occluded, b.rays_traced, b.n_gpus)
    assert (s1.rays_intersect, t1.rays_occluded) == (len(rays), len(segs))
    return h, o


# ----------------------------------------------------------------- the rows
@pytest.mark.parametrize("name", sorted(ROW_SCENES))
def test_each_row_launches_and_is_exact(gpu, name):
    c = ray_case(gpu, name)
    rc, kname = gpu.ray_bvh_kernel_name(c.scene, 0, F(gpu))
    assert rc == 0 and kname == f"rtd::k_query_isect_bvh<{ROW_SCENES[name]}>"
    h, o = both(gpu, c.scene, c.rays, c.seg_rays, want_row=ROW_SCENES[name])
    check_hits(c, c.rays, h, c.ref_hit, c.ref_rec, name + " ray-bvh intersect")
    check_occluded(c, c.seg_rays, o, c.ref_occ, name + " ray-bvh occluded")
    assert c.ref_hit.sum() >= len(c.rays) // 4 and c.ref_occ.any()


# --------------------------------------------------------------------- ties
def test_exact_ties(gpu):
    """The centre ray of every pair of bvh/ties, as it is and with tmax at exactly
    the hit's t and one ulp below it: all three pair kinds among the winners."""
    sc = scene(gpu, "bvh/ties")
    objs = scene_dict("bvh/ties")["objects"]
    centres, kinds = [], []
    for k in range(150):
        a = objs[1 + 2 * k]
        s = (a["union"][0] if "union" in a else a)["sphere"]
        centres.append(s["position"])
        kinds.append(k % 3)
    centres, kinds = np.array(centres, dtype=np.float64), np.array(kinds)
    eye = np.array(scene_dict("bvh/ties")["screen"]["observer"], dtype=np.float64)
    o = np.tile(eye, (150, 1))
    d = centres - eye
    rays = gpu.make_rays(o, d, 1e-4, INF)
    h0, _ = both(gpu, sc, rays, want_row="false, false")
    assert h0.hit.all()
    at = gpu.make_rays(o, d, 1e-4, h0.t)
    below = gpu.make_rays(o, d, 1e-4, np.nextafter(h0.t, -INF))
    h1, _ = both(gpu, sc, at)
    h2, _ = both(gpu, sc, below)
    # all three pair kinds among the winners: rays whose hit lies on their own pair (some pairs hide behind others)
    own = np.abs(h0.p - centres).max(axis=1) < 0.3
    assert {int(kd) for kd in kinds[own]} == {0, 1, 2}
    # a bare sphere accepts a hit at exactly tmax, a union does not (strict t < tmax): where the winner is a
    # sphere (sphere vs union, sphere vs sphere) the record stays, a pair of unions is lost
    keeps = own & (kinds != 1)
    assert keeps.any() and h1.records[keeps].tobytes() == h0.records[keeps].tobytes()
    lost = own & (kinds == 1)
    assert lost.any() and not np.any(h1.hit[lost] & (h1.t[lost] == h0.t[lost]))
    # ... and one ulp below, the pair's front surface is out of range for both of its members
    assert not np.any(h2.hit[own] & (h2.t[own] == h0.t[own]))
    # the reference's rule, through the oracle: every winner is the oracle's
    c = case(gpu, "bvh/ties")
    for rr, h in ((rays, h0), (at, h1), (below, h2)):
        ref_hit, ref_rec = c.oracle_intersect(rr)
        assert np.array_equal(ref_hit, h.hit) and np.array_equal(ref_rec["mat"][ref_hit], h.mat[ref_hit])


# --------------------------------------------------- more scenes and ranges
def test_deep_tree_4096(gpu):
    sc = scene(gpu, "perf4096")
    c = Case.__new__(Case)
    c._build(gpu, sc, SEED + 3, "perf4096")
    h, o = both(gpu, sc, c.rays, c.seg_rays, want_row="false, true")
    check_hits(c, c.rays, h, c.ref_hit, c.ref_rec, "perf4096 ray-bvh intersect")
    check_occluded(c, c.seg_rays, o, c.ref_occ, "perf4096 ray-bvh occluded")


@pytest.mark.parametrize("name", LEAF_BVH)
def test_leaf_cases(gpu, name):
    sc = scene(gpu, name)
    base = ray_case(gpu, "bvh/ties")
    rc, kname = gpu.ray_bvh_kernel_name(sc, 0, F(gpu))
    assert rc == 0 and "_bvh<" in kname
    # the case's own camera rays (the odd leaf is what the camera looks at) and the ties batch's incoherent ones
    o, d = odd_base_rays(gpu, sc)
    both(gpu, sc, gpu.make_rays(o, d, 1e-4, INF))
    both(gpu, sc, base.rays, base.seg_rays)


@pytest.mark.parametrize("pl", PLACEMENTS)
@pytest.mark.parametrize("name", ("bvh/ties", "bvh/grid"))
def test_placements(gpu, name, pl):
    base = ray_case(gpu, "bvh/ties")
    scale, offset = PL[pl]
    sc = load(gpu, placed_any_scale(scene_dict(name), scale, offset))
    h, o = both(gpu, sc, map_rays(base.rays, scale, offset), map_rays(base.seg_rays, scale, offset))
    assert h.hit.any()


@pytest.mark.parametrize("name", ("bvh/ties", "bvh/perf300"))
def test_ranges(gpu, name):
    """Negative tmin (hits behind the origin), tmax = +inf, finite segments, empty and reversed ranges."""
    c = ray_case(gpu, name)
    n = len(c.rays)
    rng = np.random.default_rng(SEED + 5)
    for tmin, tmax in ((-INF, INF), (-5.0, INF), (-5.0, -1e-3), (-3.0, 2.0), (1e-4, rng.uniform(0.5, 8.0, n)),
                       (rng.uniform(-4.0, 4.0, n), rng.uniform(-4.0, 8.0, n)), (2.0, 2.0), (0.0, 0.0), (-0.0, 0.0)):
        rays = gpu.make_rays(c.rays["o"], c.rays["d"], tmin, tmax)
        both(gpu, c.scene, rays)
    # hits at negative t do occur in these batches
    h = q_isect(gpu, c.scene, gpu.make_rays(c.rays["o"], c.rays["d"], -5.0, -1e-3), F(gpu))
    assert (h.t[h.hit] < 0).any()


# ----------------------------------------------------------------- odd rays
@pytest.mark.parametrize("name", ("bvh/ties", "bvh/grid"))
def test_odd_rays(gpu, name):
    """Every group of scenes.odd_ray_groups alone and interleaved one in eight
    with ordinary rays: the unflagged call's bytes, and the ordinary rays'
    bytes are theirs in a batch without the odd ones."""
    sc = scene(gpu, name)
    base = ray_case(gpu, "bvh/ties")
    ob, db = odd_base_rays(gpu, sc)
    plain = base.rays[:448].copy()          # 7 ordinary rays per odd one
    h_plain, o_plain = both(gpu, sc, plain)
    for tag, (o, d, tmin, tmax) in scenes.odd_ray_groups(ob, db).items():
        odd = gpu.make_rays(o, d, tmin, tmax)
        both(gpu, sc, odd)
        mixed = np.empty(512, dtype=plain.dtype)
        is_odd = np.arange(512) % 8 == 3
        mixed[is_odd], mixed[~is_odd] = odd, plain
        h, oc = both(gpu, sc, mixed)
        assert h.records[~is_odd].tobytes() == h_plain.records.tobytes(), tag
        assert np.array_equal(h.hit[~is_odd], h_plain.hit) and np.array_equal(oc[~is_odd], o_plain), tag


# --------------------------------------------------------------- wave tails
def _dev(rt, sc, rays, n, cap, flags):
    lib = rt.amd_lib()
    d_rays = rt.DeviceBuffer(max(1, len(rays)) * 64)
    d_rays.from_host(rays)
    d_hits, d_mask, d_occ = rt.DeviceBuffer(cap * 64), rt.DeviceBuffer(cap), rt.DeviceBuffer(cap)
    for b in (d_hits, d_mask, d_occ):
        b.from_host(np.full(b.nbytes, 0xAB, dtype=np.uint8))
    st, so = rt.Stats(), rt.Stats()
    assert lib.rt_query_intersect_device(sc.handle, d_rays.ptr, n, flags, d_hits.ptr, d_mask.ptr, None, C.byref(st)) == 0
    assert lib.rt_query_occluded_device(sc.handle, d_rays.ptr, n, flags, d_occ.ptr, None, C.byref(so)) == 0
    return d_hits.to_host(np.uint8), d_mask.to_host(np.uint8), d_occ.to_host(np.uint8), st, so


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
def test_wave_tails(gpu, n):
    c = ray_case(gpu, "bvh/ties")
    cap = n + 70
    (hb, mb, ob, st, so), rows = logged(gpu, lambda: _dev(gpu, c.scene, c.rays, n, cap, F(gpu)))
    assert len(rows) == (2 if n else 0) and all("_bvh<" in r for r in rows)
    assert (st.rays_intersect, so.rays_occluded) == (n, n)
    h0, m0, o0, _, _ = _dev(gpu, c.scene, c.rays, n, cap, 0)
    assert hb.tobytes() == h0.tobytes() and mb.tobytes() == m0.tobytes() and ob.tobytes() == o0.tobytes()
    assert np.all(hb[n * 64:] == 0xAB) and np.all(mb[n:] == 0xAB) and np.all(ob[n:] == 0xAB)
    if n:
        want = q_isect(gpu, c.scene, c.rays[:n])
        assert hb[:n * 64].tobytes() == want.records.tobytes()


# ------------------------------------------------------------- flag hygiene
def test_flag_is_accepted_where_it_changes_nothing(gpu):
    c4 = case(gpu, "config4")
    (h, o), rows = logged(gpu, lambda: (q_isect(gpu, c4.scene, c4.rays, F(gpu)), q_occl(gpu, c4.scene, c4.seg_rays, F(gpu))))
    assert rows == [gpu.query_kernel_name(c4.scene, 0)[1], gpu.query_kernel_name(c4.scene, 1)[1]]
    assert h.records.tobytes() == q_isect(gpu, c4.scene, c4.rays).records.tobytes()
    assert np.array_equal(o, q_occl(gpu, c4.scene, c4.seg_rays))
    c = ray_case(gpu, "bvh/ties")
    fl = F(gpu) | gpu.RT_FLAG_NO_CULL
    (h, o), rows = logged(gpu, lambda: (q_isect(gpu, c.scene, c.rays, fl), q_occl(gpu, c.scene, c.seg_rays, fl)))
    assert rows == [gpu.query_kernel_name(c.scene, 0)[1], gpu.query_kernel_name(c.scene, 1)[1]]
    assert h.records.tobytes() == q_isect(gpu, c.scene, c.rays).records.tobytes()
    assert np.array_equal(o, q_occl(gpu, c.scene, c.seg_rays))
    for bad in (gpu.RT_FLAG_FP32, gpu.RT_FLAG_COUNT_OPS):
        with pytest.raises(gpu.RTError) as e:
            q_isect(gpu, c.scene, c.rays, F(gpu) | bad)
        assert e.value.code == -6


def test_other_queries_ignore_the_flag(gpu):
    c = ray_case(gpu, "bvh/ties")
    o, d = c.rays["o"][:256], c.rays["d"][:256]
    a, rows_a = logged(gpu, lambda: gpu.query_radiance(c.scene, o, d))
    b, rows_b = logged(gpu, lambda: gpu.query_radiance(c.scene, o, d, F(gpu)))
    assert a.tobytes() == b.tobytes() and rows_a == rows_b and rows_a and not any("_bvh" in r for r in rows_b)
    hits = q_isect(gpu, c.scene, c.rays[:256])
    wo = -d / np.linalg.norm(d, axis=1, keepdims=True)
    a, rows_a = logged(gpu, lambda: gpu.query_shade(c.scene, hits.records, wo, hits.hit))
    b, rows_b = logged(gpu, lambda: gpu.query_shade(c.scene, hits.records, wo, hits.hit, flags=F(gpu)))
    assert a.tobytes() == b.tobytes() and rows_a == rows_b and rows_a


# ---------------------------------------------------------------- residency
def test_the_tree_is_uploaded_once_and_goes_with_the_scene(gpu):
    lib = gpu.amd_lib()
    t = (C.c_double * 4)()

    def scene_ms():
        assert lib.rt_setup_times(t, 4) == 0
        return t[0]

    base = ray_case(gpu, "bvh/ties")
    sc = gpu.load_scene_from_json_text(json.dumps(scene_dict("bvh/ties")))   # a handle no query has seen
    flat = q_isect(gpu, sc, base.rays)
    ms0 = scene_ms()
    first = q_isect(gpu, sc, base.rays, F(gpu))
    ms1 = scene_ms()
    assert ms1 > ms0                                   # the first flagged query uploads the tree
    fb = gpu.Tracer(sc, sc.width, sc.height, 0).render()
    again = q_isect(gpu, sc, base.rays)
    second = q_isect(gpu, sc, base.rays, F(gpu))
    occ = q_occl(gpu, sc, base.seg_rays, F(gpu))
    assert scene_ms() == ms1                           # a frame, an unflagged and a second flagged query: nothing
    assert first.records.tobytes() == flat.records.tobytes() == again.records.tobytes() == second.records.tobytes()
    assert np.array_equal(occ, q_occl(gpu, sc, base.seg_rays))
    assert np.isfinite(fb).all()
    gpu.shutdown()
    (third, rows) = logged(gpu, lambda: q_isect(gpu, sc, base.rays, F(gpu)))
    assert rows == ["rtd::k_query_isect_bvh<false, false>"]
    assert third.records.tobytes() == flat.records.tobytes()
    assert scene_ms() > ms1
