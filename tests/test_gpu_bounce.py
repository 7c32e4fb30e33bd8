"""Bounce-by-bounce tracing on the device: rt_scatter_rays_device and
rt_combine_bounce_device against their host forms byte for byte,
rtamd.radiance_bounces_device (the loop, every buffer on the device) against
rt_query_radiance_device byte for byte with equal ray counts, and
rt_query_radiance_depth_device.  Every comparison is equality of bytes (two
NaN colours count as equal); tests/test_bounce_plan.py holds the host forms to
the reference's rules on the CPU."""
import ctypes as C
import json

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

# The scan's first level is one workgroup over 256 workgroup counts of 256
# parents each (rt_bounce.hpp kScatterTile x kScatterThreads): one parent more
# takes the second level.
SCAN_LEVEL1_PARENTS = 256 * 256
SIZES = [1, 63, 64, 65, 255, 256, 257, 1025, SCAN_LEVEL1_PARENTS + 1]


def _beq(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _differing(got, want):
    g, w = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    eq = (g.view(np.uint64) == w.view(np.uint64)) | (np.isnan(g) & np.isnan(w))
    return int((~eq.all(axis=1)).sum())


class _At:
    """A device buffer seen from `shift` bytes in."""

    def __init__(self, buf, shift):
        self.ptr = C.c_void_p(buf.ptr.value + shift)
        self.nbytes = buf.nbytes - shift


def _dev(rt, arr, pad=0):
    arr = np.ascontiguousarray(arr)
    b = rt.DeviceBuffer(max(arr.nbytes + pad, 16))
    if arr.nbytes:
        b.from_host(arr)
    return b


# ----------------------------------------------------------------- 1. scatter
_mat_scene = {}


def _material_scene(rt):
    """Four materials: 0 plain, 1 mirror, 2 glass, 3 both; recursion 4."""
    if "sc" not in _mat_scene:
        objs = [scenes._sph([k, 0, -3], 0.4, scenes._mat([0.5, 0.5, 0.5])) for k in range(4)]
        sc = rt.load_scene_from_json_text(json.dumps(scenes._base(objs, recursion=4, dpi=4)))
        _mat_scene["sc"] = rt.with_material_fields(sc, {
            0: {"kr": 0.0, "kt": 0.0}, 1: {"kr": 0.6, "kt": 0.0},
            2: {"kr": 0.0, "kt": 0.7, "refractive_index": 1.5}, 3: {"kr": 0.25, "kt": 0.5, "refractive_index": 1.3}})
    return _mat_scene["sc"]


PATTERNS = ["none", "both", "alternating", "last_lane_of_last_wave", "lane0", "random"]


def _parents(rt, n, pattern, seed=5):
    """n synthetic parents whose spawn pattern is `pattern` (front-face hits of
    the both-material spawn two children: 1.3 from outside has no TIR)."""
    rng = np.random.default_rng(seed + n)
    d = rng.normal(size=(n, 3))
    nn = rng.normal(size=(n, 3))
    nn /= np.linalg.norm(nn, axis=1)[:, None]
    d -= nn * (1.0 + np.abs(rng.normal(size=n)))[:, None]   # towards the surface
    rays = rt.make_rays(rng.normal(size=(n, 3)), d)
    hits = np.zeros(n, dtype=rt.HIT_DTYPE)
    hits["t"], hits["p"], hits["n"], hits["front_face"] = 1.0, rng.normal(size=(n, 3)), nn, 1
    mask = np.ones(n, dtype=np.uint8)
    i = np.arange(n)
    if pattern == "none":
        hits["mat"] = 0
    elif pattern == "both":
        hits["mat"] = 3
    elif pattern == "alternating":
        hits["mat"] = np.where(i % 2 == 0, 3, 0)
    elif pattern == "last_lane_of_last_wave":
        hits["mat"] = np.where(i == n - 1, 3, 0)
    elif pattern == "lane0":
        hits["mat"] = np.where(i == 0, 3, 0)
    else:
        hits["mat"] = rng.integers(-2, 6, n)          # null and out-of-range materials too
        hits["front_face"] = rng.integers(0, 2, n)     # back faces: total internal reflection happens
        mask = (rng.random(n) < 0.8).astype(np.uint8)
        odd = rng.random(n) < 0.02
        rays["d"][odd, 0] = np.nan
        hits["n"][rng.random(n) < 0.02] *= 3.0
    return rays, hits, mask


def _device_scatter(rt, sc, rays, hits, mask, depth, cap=None, shift=0, guard=0):
    n = len(rays)
    cap = 2 * n if cap is None else cap
    d_rays, d_hits = _dev(rt, rays), _dev(rt, hits)
    d_mask = _dev(rt, mask) if mask is not None else None
    d_spawn, d_first = rt.DeviceBuffer(max(n, 16)), rt.DeviceBuffer(max(8 * n, 16))
    g_rays = np.full(((cap + guard) * 64 + shift) // 8 + 2, -7.0)
    g_w = np.full(cap + guard + 2, -7.0)
    d_cr, d_cw = _dev(rt, g_rays), _dev(rt, g_w)
    st = rt.Stats()
    err = None
    try:
        m = rt.scatter_rays_device(sc, d_rays, d_hits, d_mask, n, depth, d_spawn, d_first, _At(d_cr, shift), d_cw, cap,
                                   stats=st)
    except rt.RTError as e:
        err, m = e, e.needed
    spawn = d_spawn.to_host(np.uint8)[:n]
    first = d_first.to_host(np.uint64)[:n]
    raw = d_cr.to_host(np.uint8)
    k = min(m, cap)
    child = raw[shift:shift + k * 64].view(rt.RAY_DTYPE)
    w = d_cw.to_host(np.float64)
    behind = (raw[shift + k * 64:shift + (cap + guard) * 64].view(np.float64), w[k:cap + guard])
    return (spawn, first, child, w[:k]), m, err, behind, st


@pytest.mark.parametrize("n", SIZES)
def test_device_scatter_is_the_host_scatter(gpu, n):
    sc = _material_scene(gpu)
    for pattern in PATTERNS:
        rays, hits, mask = _parents(gpu, n, pattern)
        want = gpu.scatter_rays(sc, rays, hits, mask, 1)
        for items in (0, 192):
            gpu.scatter_launch_items(items)
            try:
                got, m, err, _, st = _device_scatter(gpu, sc, rays, hits, mask, 1)
            finally:
                gpu.scatter_launch_items(0)
            assert err is None and m == len(want[2]), (pattern, items)
            for g, w in zip(got, want):
                assert _beq(g, w), (n, pattern, items)
            assert (st.rays_intersect, st.rays_occluded, st.rays_traced, st.pixels, st.n_gpus) == (0, 0, 0, 0, 1)
        if pattern == "both":
            assert m == 2 * n
        if pattern == "none":
            assert m == 0
    # the same bytes on a second run, at a depth that spawns nothing, and into a
    # child buffer that is not 16-byte aligned
    rays, hits, mask = _parents(gpu, n, "random")
    want = gpu.scatter_rays(sc, rays, hits, None, 0)
    a = _device_scatter(gpu, sc, rays, hits, None, 0)[0]
    b = _device_scatter(gpu, sc, rays, hits, None, 0, shift=8)[0]
    for g, h, w in zip(a, b, want):
        assert _beq(g, w) and _beq(h, w)
    got, m, err, _, _ = _device_scatter(gpu, sc, rays, hits, mask, 3)   # depth = limit - 1
    assert err is None and m == 0 and not got[0].any() and not got[1].any()


@pytest.mark.parametrize("n,items", [(257, 0), (1025, 192)])
def test_child_cap(gpu, n, items):
    sc = _material_scene(gpu)
    rays, hits, mask = _parents(gpu, n, "random")
    want = gpu.scatter_rays(sc, rays, hits, mask, 0)
    m = len(want[2])
    assert m > 2
    gpu.scatter_launch_items(items)
    try:
        got, gm, err, behind, _ = _device_scatter(gpu, sc, rays, hits, mask, 0, cap=m, guard=8)
        assert err is None and gm == m
        assert all(_beq(g, w) for g, w in zip(got, want))
        assert (behind[0] == -7.0).all() and (behind[1] == -7.0).all()
        got, gm, err, behind, _ = _device_scatter(gpu, sc, rays, hits, mask, 0, cap=m - 1, guard=8)
        assert err is not None and err.code == gpu.RT_ERR_INVALID_ARG and gm == m
        assert _beq(got[0], want[0]) and _beq(got[1], want[1])
        assert _beq(got[2], want[2][:m - 1]) and _beq(got[3], want[3][:m - 1])
        assert (behind[0] == -7.0).all() and (behind[1] == -7.0).all()   # nothing behind the cap was written
        got, gm, err, behind, _ = _device_scatter(gpu, sc, rays, hits, mask, 0, cap=0, guard=8)
        assert err is not None and gm == m and (behind[0] == -7.0).all() and (behind[1] == -7.0).all()
    finally:
        gpu.scatter_launch_items(0)


# ----------------------------------------------------------------- 2. combine
@pytest.mark.parametrize("n", [1, 255, 257, 4099])
def test_device_combine_is_the_host_combine(gpu, n):
    rng = np.random.default_rng(n)
    spawn = rng.integers(0, 4, n).astype(np.uint8)
    spawn[rng.random(n) < 0.05] |= 0xF0   # (bits beyond the two are ignored)
    cnt = (spawn & 1) + ((spawn >> 1) & 1)
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.uint64)
    m = int(cnt.sum())
    wild = rng.random(n) < 0.1
    first[wild] = rng.choice(np.array([m, m + 1, 2**63, 2**64 - 1, 2**64 - 2, m - 1 if m else 0], dtype=np.uint64), int(wild.sum()))
    crgb = rng.uniform(-0.5, 1.5, (max(m, 1), 3))[:m]
    cw = rng.uniform(-1.0, 2.0, max(m, 1))[:m]
    rgb = rng.uniform(0.0, 1.2, (n, 3))
    for arr in (crgb.reshape(-1), cw, rgb.reshape(-1)):
        if arr.size >= 8:
            arr[rng.integers(0, arr.size, 6)] = [np.nan, np.inf, -np.inf, 5e-324, -2e-310, 0.0]
    want = gpu.combine_bounce(rgb, spawn, first, crgb, cw)
    d_rgb, d_spawn, d_first = _dev(gpu, rgb), _dev(gpu, spawn), _dev(gpu, first)
    d_crgb, d_cw = _dev(gpu, crgb), _dev(gpu, cw)
    gpu.combine_bounce_device(d_rgb, d_spawn, d_first, n, d_crgb, d_cw, m)
    got = d_rgb.to_host()[:3 * n].reshape(n, 3)
    assert _beq(got, want)
    # no children at all: every index is out of range and the colours stay
    d_rgb.from_host(rgb)
    gpu.combine_bounce_device(d_rgb, d_spawn, d_first, n, None, None, 0)
    assert _beq(d_rgb.to_host()[:3 * n].reshape(n, 3), rgb)


# -------------------------------------------------------------------- 3. loop
LOOP_SCENES = ["cfg5", "deep6", "torture/reflect_refract", "torture/recursion0", "leaf/neg_radius_glass",
               "leaf/index_edges", "leaf/index_huge", "leaf/index_medium0", "leaf/coeff_edges", "leaf/neg_radius_eager"]
_loop_cache = {}


def _loop_scene_json(name):
    if name == "cfg5":
        return json.loads(scenes.config_json(5, dpi=6)[0])
    if name == "deep6":
        return scenes.deep_recursion_scene(6, dpi=8)
    group, key = name.split("/")
    return (scenes.torture_scenes(dpi=10) if group == "torture" else scenes.leaf_cases(dpi=8))[key]


def _loop_case(rt, name):
    """(scene, pixel-centre rays, their device buffer), once per scene."""
    if name not in _loop_cache:
        sc = rt.load_scene_from_json_text(json.dumps(_loop_scene_json(name)))
        rays = rt.camera_rays(sc, sc.width, sc.height, rt.RT_RAYS_CENTRE).reshape(-1)
        _loop_cache[name] = (sc, rays, _dev(rt, rays))
    return _loop_cache[name]


def _full_trace(rt, sc, d_rays, n, flags=0):
    d_rgb = rt.DeviceBuffer(24 * n)
    st = rt.Stats()
    rt.query_radiance_device(sc, d_rays, n, d_rgb, flags, stats=st)
    return d_rgb.to_host()[:3 * n].reshape(n, 3), st


@pytest.mark.parametrize("name", LOOP_SCENES)
def test_bounce_loop_is_the_radiance_query(gpu, name):
    sc, rays, d_rays = _loop_case(gpu, name)
    n = len(rays)
    for flags in (0, gpu.RT_FLAG_NO_CULL):
        want, wst = _full_trace(gpu, sc, d_rays, n, flags)
        d_rgb, sizes, st = gpu.radiance_bounces_device(sc, d_rays, n, flags)
        got = d_rgb.to_host()[:3 * n].reshape(n, 3)
        print(f"  {name} flags {flags}: levels {sizes}, rays ({st.rays_intersect}, {st.rays_occluded})")
        assert _differing(got, want) == 0
        assert (st.rays_intersect, st.rays_occluded) == (wst.rays_intersect, wst.rays_occluded)
        assert st.rays_traced == st.rays_intersect + st.rays_occluded
    # every shininess of these scenes is an integer below 1024, so both paths
    # take pow_spec: the oracle's Tracer::trace under the device's power
    d = sc.desc
    assert all(float(d.materials[i].shininess).is_integer() and 0 <= d.materials[i].shininess < 1024
               for i in range(d.n_materials))
    with gpu.oracle_pow(1):
        ref, ni, no = gpu.oracle_trace_rays(sc, rays["o"], rays["d"])
    assert _differing(got, ref) == 0
    assert (st.rays_intersect, st.rays_occluded) == (int(ni.sum()), int(no.sum()))
    if name == "torture/recursion0":
        assert sizes == [] and not got.any() and st.rays_traced == 0
    if name in ("deep6", "torture/reflect_refract"):
        assert len(sizes) == 6


# ------------------------------------------------------------------- 4. depth
@pytest.mark.parametrize("name", ["torture/reflect_refract", "deep6", "leaf/index_edges"])
def test_radiance_depth(gpu, name):
    sc, rays, d_rays = _loop_case(gpu, name)
    n, limit = len(rays), sc.desc.recursion_limit
    want, wst = _full_trace(gpu, sc, d_rays, n)
    d_rgb = gpu.DeviceBuffer(24 * n)
    st = gpu.Stats()
    gpu.query_radiance_depth_device(sc, d_rays, n, 0, d_rgb, stats=st)   # depth 0: rt_query_radiance
    assert _beq(d_rgb.to_host()[:3 * n].reshape(n, 3), want)
    assert (st.rays_intersect, st.rays_occluded, st.rays_traced) == (wst.rays_intersect, wst.rays_occluded, wst.rays_traced)
    host = gpu.query_radiance_depth(sc, rays["o"], rays["d"], 0)
    assert _beq(host, want)
    # level 0 by hand, its children traced at depth 1, combined: the full trace
    d_hits, d_mask, d_wo = gpu.DeviceBuffer(64 * n), gpu.DeviceBuffer(max(n, 16)), gpu.DeviceBuffer(24 * n)
    d_direct = gpu.DeviceBuffer(24 * n)
    s0, s1, s2 = gpu.Stats(), gpu.Stats(), gpu.Stats()
    gpu.query_intersect_device(sc, d_rays, n, d_hits, d_mask, stats=s0)
    gpu.rays_wo_device(d_rays, n, d_wo)
    gpu.query_shade_device(sc, d_hits, d_wo, d_mask, n, d_direct, stats=s1)
    d_spawn, d_first = gpu.DeviceBuffer(max(n, 16)), gpu.DeviceBuffer(8 * n)
    d_child, d_w = gpu.DeviceBuffer(128 * n), gpu.DeviceBuffer(16 * n)
    m = gpu.scatter_rays_device(sc, d_rays, d_hits, d_mask, n, 0, d_spawn, d_first, d_child, d_w, 2 * n)
    assert m > 0
    d_crgb = gpu.DeviceBuffer(24 * m)
    gpu.query_radiance_depth_device(sc, d_child, m, 1, d_crgb, stats=s2)
    gpu.combine_bounce_device(d_direct, d_spawn, d_first, n, d_crgb, d_w, m)
    assert _differing(d_direct.to_host()[:3 * n].reshape(n, 3), want) == 0
    assert s0.rays_intersect + s2.rays_intersect == wst.rays_intersect
    assert s1.rays_occluded + s2.rays_occluded == wst.rays_occluded
    # the children at depth 1 are the trace of the scene with one level less
    sub = gpu.with_recursion_limit(sc, limit - 1)
    sub_rgb, _ = _full_trace(gpu, sub, d_child, m)
    assert _beq(sub_rgb, d_crgb.to_host()[:3 * m].reshape(m, 3))
    # depth = limit, and beyond: black, nothing traced
    for depth in (limit, limit + 5, 2**31 - 1):
        d_crgb.from_host(np.full(3 * m, 0.5))
        st = gpu.Stats()
        gpu.query_radiance_depth_device(sc, d_child, m, depth, d_crgb, stats=st)
        assert not d_crgb.to_host()[:3 * m].any() and (st.rays_intersect, st.rays_occluded, st.rays_traced) == (0, 0, 0)
    # a frame after it is the frame it was before: the resident scene is left alone
    t = (C.c_double * 4)()
    lib = gpu.amd_lib()
    W, H = sc.width, sc.height
    before = gpu.Tracer(sc, W, H, gpu.RT_MODE_STANDARD).render()
    assert lib.rt_setup_times(t, 4) == 0
    ms0 = t[0]
    gpu.query_radiance_depth_device(sc, d_child, m, 2, d_crgb)
    after = gpu.Tracer(sc, W, H, gpu.RT_MODE_STANDARD).render()
    assert lib.rt_setup_times(t, 4) == 0
    assert t[0] == ms0 and _beq(before, after)


# -------------------------------------------------------------- 5. launch log
def test_launch_log_and_residency(gpu):
    sc, rays, d_rays = _loop_case(gpu, "torture/reflect_refract")
    n = len(rays)
    lib = gpu.amd_lib()
    t = (C.c_double * 4)()
    _full_trace(gpu, sc, d_rays, n)   # (the scene is resident from here on)
    assert lib.rt_setup_times(t, 4) == 0
    ms0 = t[0]
    d_hits, d_mask = gpu.DeviceBuffer(64 * n), gpu.DeviceBuffer(max(n, 16))
    gpu.query_intersect_device(sc, d_rays, n, d_hits, d_mask)
    d_spawn, d_first = gpu.DeviceBuffer(max(n, 16)), gpu.DeviceBuffer(8 * n)
    d_child, d_w = gpu.DeviceBuffer(128 * n), gpu.DeviceBuffer(16 * n)
    d_rgb = gpu.DeviceBuffer(24 * n)
    gpu.launch_log(True)
    try:
        m = gpu.scatter_rays_device(sc, d_rays, d_hits, d_mask, n, 0, d_spawn, d_first, d_child, d_w, 2 * n)
        d_crgb = gpu.DeviceBuffer(24 * max(m, 1))
        gpu.combine_bounce_device(d_rgb, d_spawn, d_first, n, d_crgb, d_w, m)
        log = gpu.launch_log_get()
    finally:
        gpu.launch_log(False)
    assert log == ["rtd::k_scatter_count", "rtd::k_scan_tile<true>", "rtd::k_scatter_emit<true>", "rtd::k_combine_bounce"]
    assert lib.rt_setup_times(t, 4) == 0 and t[0] == ms0   # no scene was compiled or uploaded
    # past the scan's first level: two levels of tiles and the add
    big = SCAN_LEVEL1_PARENTS + 1
    rays2, hits2, mask2 = _parents(gpu, big, "alternating")
    gpu.launch_log(True)
    try:
        _device_scatter(gpu, _material_scene(gpu), rays2, hits2, mask2, 0)
        log = gpu.launch_log_get()
    finally:
        gpu.launch_log(False)
    assert log == ["rtd::k_scatter_count", "rtd::k_scan_tile<false>", "rtd::k_scan_tile<true>", "rtd::k_scan_add",
                   "rtd::k_scatter_emit<true>"]
