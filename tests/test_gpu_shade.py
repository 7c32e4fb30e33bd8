"""Batched shading queries on the GPU (rt_query_shade / rt_query_shade_device:
shade_lambert_phong for caller-given hits, shading.cpp:31-138) against
rtamd.oracle_shade, the numpy restatement that tests/test_shade_plan.py holds
to the pinned oracle's own shading (within 3.3e-11 there).

Hits: the oracle's closest hits of the rays of tests/test_gpu_query.py (per
scene 768 rays), or of the same recipe on other scenes, with wo = -d unless a
test says otherwise; the rays that miss ride along as masked-out entries.  The
expected values are test_shade_plan.shade_ref's, computed once.

Bar: every channel |gpu - oracle| <= 1e-5, the project's parity bar (where the
oracle is not finite - pow(0, -2) - the GPU must be non-finite of the same
kind), and a batch's rays_occluded exactly the sum of the oracle's per-hit
counts.  A hit may be left out only if the ORACLE alone is unstable on it (its
colour moves by more than 1e-5, or its occluded count changes, when p moves
+-1e-7 along an axis): at most 1 % of a scene's shaded hits.  On the CPU that
rule leaves out no hit of any scene here, so the cap is a safeguard.  The kept
hits are queried once more as their own batch for the count assertion.

Measured on an MI355X: the largest difference over all of this file's entries
is 1.46e-11 (shading/exponents_wave with a random wo; 3.6e-15 with wo = -d, at
most 1.2e-16 on the 18 scenes), no hit had to be left out, and intersect ->
shade on the device differs from rt_query_radiance at recursion limit 1 by 0.
Every test prints its largest difference."""
import ctypes as C
import json

import numpy as np
import pytest

import scenes
from test_gpu_query import SCENES, case
from test_shade_plan import override_lights, shade_ref

pytestmark = pytest.mark.gpu

TOL = 1e-5
MAGENTA = np.array([1.0, 0.0, 1.0])
_vp = C.c_void_p


# ------------------------------------------------------------------ helpers
def shade(rt, r, sel=slice(None), flags=0, stats=None, wo=None, lights="ref"):
    """rt_query_shade of r's entries `sel`: hits and misses, the misses masked
    out; under r's lights unless `lights` is given."""
    return rt.query_shade(r.sc, r.H[sel], (r.wo if wo is None else wo)[sel], r.hit[sel].astype(np.uint8),
                          r.lights if isinstance(lights, str) else lights, None, flags, stats)


def oracle_unstable(rt, r, k, wo, rgb_k, no_k, step=1e-7):
    """oracle_shade of hit k moves under a +-step shift of p."""
    for ax in range(3):
        for sgn in (1.0, -1.0):
            h = r.H[k:k + 1].copy()
            h["p"][0, ax] += sgn * step
            rgb, no = rt.oracle_shade(r.sc, h, wo[k:k + 1], r.lights)
            with np.errstate(invalid="ignore"):
                moved = not np.all(np.abs(rgb[0] - rgb_k) <= TOL) if np.isfinite(rgb_k).all() else \
                    not np.array_equal(rgb[0], rgb_k, equal_nan=True)
            if moved or no[0] != no_k:
                return True
    return False


def check(rt, r, got, what, flags=0, wo=None, ref=None, step=1e-7):
    """got (n, 3) against the oracle at this file's bar; then the hits not left
    out once more as their own unmasked batch: the same colours, the oracle's
    count.  ref: (rgb, no) over all entries when not r's own (another wo);
    step: the instability probe's shift of p."""
    n = len(r)
    wo = r.wo if wo is None else wo
    ref_rgb, ref_no = (r.rgb, r.no) if ref is None else ref
    assert got.shape == (n, 3) and got.dtype == np.float64
    # masked-out entries: the background, bit for bit
    assert got[~r.hit].tobytes() == np.tile(r.background, (int((~r.hit).sum()), 1)).tobytes(), what
    fin = np.isfinite(ref_rgb)
    with np.errstate(invalid="ignore"):
        diff = np.where(fin, np.abs(got - ref_rgb), 0.0).max(axis=1)
        same_kind = (fin | ((got == ref_rgb) | (np.isnan(got) & np.isnan(ref_rgb)))).all(axis=1)
        bad = np.flatnonzero(r.hit & ~((diff <= TOL) & same_kind))
    left_out = [int(k) for k in bad if oracle_unstable(rt, r, k, wo, ref_rgb[k], ref_no[k], step)]
    wrong = sorted(set(bad.tolist()) - set(left_out))
    keep = r.hit.copy()
    keep[left_out] = False
    mx = float(diff[keep].max(initial=0.0))
    print(f"  {what}: {n} entries, {int(r.hit.sum())} shaded, max|d|={mx:.3g}, non-finite hits "
          f"{int((~fin).any(axis=1).sum())}, left out {len(left_out)} (oracle unstable), oracle count "
          f"{int(ref_no[keep].sum())}")
    assert not wrong, (what, wrong[:8], [(got[k], ref_rgb[k]) for k in wrong[:3]])
    assert len(left_out) <= int(r.hit.sum()) // 100, (what, left_out)
    st = rt.Stats()
    again = rt.query_shade(r.sc, r.H[keep], wo[keep], None, r.lights, None, flags, st)
    assert again.tobytes() == got[keep].tobytes(), what
    assert (st.rays_intersect, st.rays_occluded, st.rays_traced) == (0, int(ref_no[keep].sum()), int(ref_no[keep].sum())), what
    assert st.pixels == 0 and st.n_gpus == 1
    return mx


# ------------------------------------------------------------ 1. every scene
@pytest.mark.parametrize("name", sorted(SCENES))
def test_shade_matches_oracle(gpu, name):
    r = shade_ref(gpu, name)
    assert len(r) == 768
    st = gpu.Stats()
    got = shade(gpu, r, stats=st)
    assert st.ms_kernel > 0.0 and st.ms_total >= st.ms_kernel and st.n_gpus == 1 and st.pixels == 0
    check(gpu, r, got, name)
    print(f"  {name}: {int((r.H['t'][r.hit] > 10).sum())} hits at t > 10")
    assert r.hit.sum() >= len(r) // 4   # (the batch does exercise the objects)


def test_far_hits_are_present(gpu):
    """Hits at t > 10 (where the shadow epsilon is 1e-4 t, not 1e-3) are shaded in 16 of the 18 scenes."""
    assert sum(bool((shade_ref(gpu, n).H["t"][shade_ref(gpu, n).hit] > 10).any()) for n in SCENES) == 16


# --------------------------------------------------------- 2. shading inputs
@pytest.mark.parametrize("name", ["lights65_csg", "near_light_wave", "far_skip_few", "null_mat_csg", "exponents_wave",
                                  "extremes_csg"])
def test_shading_inputs(gpu, name):
    """More than 32 lights, a light nearer than the shadow epsilon / skipped
    lights, null materials, exponents whose pow is not finite, extreme
    material values."""
    r = shade_ref(gpu, "shading/" + name)
    got = shade(gpu, r)
    check(gpu, r, got, "shading/" + name)
    if name == "lights65_csg":
        assert r.sc.desc.n_lights > 32
    if name == "exponents_wave":
        assert not np.isfinite(r.rgb).all()
    if name == "null_mat_csg":
        null = r.hit & (r.H["mat"] == -1)
        assert null.any() and not r.no[null].any()
        assert got[null].tobytes() == np.tile(MAGENTA, (int(null.sum()), 1)).tobytes()
        st = gpu.Stats()
        gpu.query_shade(r.sc, r.H[null], r.wo[null], stats=st)
        assert st.rays_occluded == 0


# ------------------------------------------------------ 3. any view direction
@pytest.mark.parametrize("name", ["exponents_wave", "extremes_few"])
def test_any_view_direction(gpu, name):
    r = shade_ref(gpu, "shading/" + name)
    rng = np.random.default_rng(515 + len(name))
    v = rng.normal(size=(len(r), 3))
    v /= np.sqrt((v * v).sum(axis=1))[:, None]
    v = np.where(((v * r.H["n"]).sum(axis=1) < 0)[:, None], -v, v)   # (into the normal's hemisphere)
    rgb, no = r.rgb.copy(), r.no.copy()
    rgb[r.hit], no[r.hit] = gpu.oracle_shade(r.sc, r.H[r.hit], v[r.hit])
    got = shade(gpu, r, wo=v)
    check(gpu, r, got, f"shading/{name} with a random wo", wo=v, ref=(rgb, no))
    base = shade(gpu, r)
    assert not np.array_equal(got, base, equal_nan=True)   # wo is read
    assert not np.array_equal(rgb, r.rgb, equal_nan=True)


# ----------------------------------------------------------- 4. light override
@pytest.mark.parametrize("name,n", [("config4", 0), ("config4", 1), ("config4", 32), ("config4", 33), ("config4", 65),
                                    ("dir/pokeball_csg_sun", 2)])
def test_light_override(gpu, name, n):
    r = shade_ref(gpu, f"override/{name}/{n}")
    assert r.lights is not None and len(r.lights) == n
    got = shade(gpu, r)
    check(gpu, r, got, f"{name} with {n} lights of the call")
    own = shade(gpu, r, lights=None)
    assert own.tobytes() != got.tobytes()   # (the call's lights, not the scene's)
    if name.startswith("dir/"):
        # the directional light still shades: without it the oracle's colours differ
        dark, _ = gpu.oracle_shade(gpu.with_dir_lights(r.sc, []), r.H[r.hit], r.wo[r.hit], r.lights)
        assert r.sc.desc.n_dir_lights > 0 and float(np.abs(dark - r.rgb[r.hit]).max()) > 100 * TOL


def test_no_override_is_the_scenes_own_lights(gpu):
    r = shade_ref(gpu, "config4")
    d = r.sc.desc
    own = [(list(d.lights[i].pos), list(d.lights[i].intensity)) for i in range(d.n_lights)]
    sa, sb = gpu.Stats(), gpu.Stats()
    a = shade(gpu, r, stats=sa)
    b = shade(gpu, r, lights=own, stats=sb)
    assert a.tobytes() == b.tobytes() and sa.rays_occluded == sb.rays_occluded > 0
    # lights is ignored when n_lights < 0
    junk = (gpu.Light * 1)()
    rgb = np.zeros((len(r), 3))
    assert gpu.amd_lib().rt_query_shade(r.sc.handle, r.H.ctypes.data_as(_vp), r.wo.ctypes.data_as(_vp),
                                        r.hit.astype(np.uint8).ctypes.data_as(_vp), len(r), C.cast(junk, _vp), -7, None,
                                        0, rgb.ctypes.data_as(_vp), None) == 0
    assert rgb.tobytes() == a.tobytes()


def test_override_leaves_the_resident_scene_alone(gpu):
    lib = gpu.amd_lib()
    r = shade_ref(gpu, "config4")
    sc = r.sc
    t = (C.c_double * 4)()

    def scene_ms():
        assert lib.rt_setup_times(t, 4) == 0
        return t[0]

    W, H = sc.width, sc.height
    fb = gpu.Tracer(sc, W, H, 0).render()
    plain = shade(gpu, r)
    ms = scene_ms()
    for n in (0, 3, 65):
        shade(gpu, r, lights=override_lights("config4", n))
    assert np.array_equal(gpu.Tracer(sc, W, H, 0).render(), fb)
    assert shade(gpu, r).tobytes() == plain.tobytes()
    assert gpu.query_radiance(sc, r.o[:64], r.d[:64]).shape == (64, 3)
    assert scene_ms() == ms


# ----------------------------------------- 5. the deferred pipeline on the device
@pytest.mark.parametrize("name", ["config4", "torture/xform_in_csg", "deep/xform_nest12"])
def test_deferred_pipeline_on_the_device(gpu, name):
    """rt_query_intersect_device, then rt_query_shade_device on its (hits, mask)
    buffers in place, on one stream: Tracer::trace at recursion depth 1."""
    lib = gpu.amd_lib()
    r = shade_ref(gpu, name)
    n = len(r)
    rec1 = gpu.with_recursion_limit(r.sc, 1)
    rs = gpu.Stats()
    want = gpu.query_radiance(rec1, r.o, r.d, stats=rs)
    d_rays, d_hits, d_mask = gpu.DeviceBuffer(n * 64), gpu.DeviceBuffer(n * 64), gpu.DeviceBuffer(n)
    d_wo, d_rgb = gpu.DeviceBuffer(n * 24), gpu.DeviceBuffer(n * 24)
    d_rays.from_host(gpu.make_rays(r.o, r.d))
    d_wo.from_host(r.wo)
    stream = gpu.Stream()
    try:
        assert lib.rt_query_intersect_device(r.sc.handle, d_rays.ptr, n, 0, d_hits.ptr, d_mask.ptr, stream.handle,
                                             None) == 0, gpu.last_error()
        st = gpu.Stats()
        gpu.query_shade_device(r.sc, d_hits, d_wo, d_mask, n, d_rgb, stream=stream, stats=st)
        got = d_rgb.to_host(np.float64, (n, 3))
        gpu.query_shade_device(r.sc, d_hits, d_wo, d_mask, n, d_rgb, miss_rgb=(1.0, 1.0, 1.0), stream=stream)
        white = d_rgb.to_host(np.float64, (n, 3))
    finally:
        stream.destroy()
    hits, mask = d_hits.to_host(gpu.HIT_DTYPE), d_mask.to_host(np.uint8)
    err = float(np.abs(got - want).max())
    print(f"  {name}: intersect -> shade on the device, {int(mask.sum())} of {n} hit, max|d| to rt_query_radiance at "
          f"recursion limit 1: {err:.3g}, occluded {st.rays_occluded}")
    assert err <= TOL
    assert (st.rays_intersect, st.rays_occluded) == (0, rs.rays_occluded) and rs.rays_intersect == n
    miss = mask == 0
    assert miss.any()
    assert np.all(white[miss] == 1.0) and white[~miss].tobytes() == got[~miss].tobytes()
    assert got[miss].tobytes() == np.tile(r.background, (int(miss.sum()), 1)).tobytes()
    # the host form: the same bytes
    hs = gpu.Stats()
    host = gpu.query_shade(r.sc, hits, r.wo, mask, stats=hs)
    assert host.tobytes() == got.tobytes() and hs.rays_occluded == st.rays_occluded
    with pytest.raises(ValueError):
        gpu.query_shade_device(r.sc, gpu.DeviceBuffer(64), gpu.DeviceBuffer(24), None, 2, gpu.DeviceBuffer(48))


# ------------------------------------------------------ 6. wave tails and masks
def _dev_shade(rt, r, H, wo, mask, n, cap):
    """rt_query_shade_device on the first n entries into a buffer of cap colours filled with 0xAB."""
    d_hits, d_wo = rt.DeviceBuffer(max(1, len(H)) * 64), rt.DeviceBuffer(max(1, len(H)) * 24)
    d_hits.from_host(H)
    d_wo.from_host(wo)
    d_mask = None
    if mask is not None:
        d_mask = rt.DeviceBuffer(max(1, len(H)))
        d_mask.from_host(mask)
    d_rgb = rt.DeviceBuffer(cap * 24)
    d_rgb.from_host(np.full(cap * 24, 0xAB, dtype=np.uint8))
    st = rt.Stats()
    rt.query_shade_device(r.sc, d_hits, d_wo, d_mask, n, d_rgb, stats=st)
    return d_rgb.to_host(np.uint8), st


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("name", ["config4", "torture/csg_groups"])
def test_wave_tails(gpu, name, n):
    """The first n entries: the full batch's colours bit for bit, the oracle's
    count over those n entries (lanes past the end count nothing), and nothing
    written past 3n doubles."""
    r = shade_ref(gpu, name)
    full = shade(gpu, r)
    want = int(r.no[:n].sum())
    st = gpu.Stats()
    got = shade(gpu, r, slice(0, n), stats=st)
    assert got.tobytes() == full[:n].tobytes()
    assert (st.rays_intersect, st.rays_occluded, st.rays_traced) == (0, want, want)
    cap = n + 50
    raw, st = _dev_shade(gpu, r, r.H, r.wo, r.hit.astype(np.uint8), n, cap)
    assert raw[:n * 24].tobytes() == full[:n].tobytes()
    assert np.all(raw[n * 24:] == 0xAB)
    assert (st.rays_intersect, st.rays_occluded, st.rays_traced) == (0, want, want)


@pytest.mark.parametrize("pattern", ["wave", "alternating", "all"])
def test_mask_patterns(gpu, pattern):
    """A whole wave of masked entries, alternating entries, everything masked:
    the unmasked entries are bit-identical to the compacted batch, the masked
    ones the miss colour, and only the unmasked ones count."""
    r = shade_ref(gpu, "config4")
    n = 320
    H, wo = r.H[:n].copy(), r.wo[:n]
    m = r.hit[:n].copy()
    if pattern == "wave":
        m[64:128] = False
    elif pattern == "alternating":
        m[1::2] = False
    else:
        m[:] = False
    # masked entries hold garbage: nothing of them is interpreted
    H["mat"][~m] = 10**6
    H["p"][~m] = np.nan
    H["t"][~m] = -np.inf
    wo = np.where(m[:, None], wo, np.nan)
    miss = (0.25, 0.5, 0.125)
    st, sc_ = gpu.Stats(), gpu.Stats()
    got = gpu.query_shade(r.sc, H, wo, m.astype(np.uint8), None, miss, 0, st)
    assert got[~m].tobytes() == np.tile(np.array(miss), (int((~m).sum()), 1)).tobytes()
    if m.any():
        compact = gpu.query_shade(r.sc, H[m], wo[m], stats=sc_)
        assert got[m].tobytes() == compact.tobytes()
        assert got[m].tobytes() == shade(gpu, r, slice(0, n))[m].tobytes()
    assert st.rays_occluded == sc_.rays_occluded == int(r.no[:n][m].sum())
    assert (pattern == "all") == (st.rays_occluded == 0)


# --------------------------------------------------------- 7. material indices
def test_material_indices_outside_the_table_are_null_materials(gpu):
    r = shade_ref(gpu, "config4")
    k = np.flatnonzero(r.hit)[:128]
    H, wo = r.H[k].copy(), r.wo[k]
    base = gpu.query_shade(r.sc, H, wo)
    at = np.array([5, 17, 30, 63, 64, 100])
    H["mat"][at] = [-1, -2, r.sc.desc.n_materials, 2**31 - 1, -(2**31), r.sc.desc.n_materials + 1]
    other = np.ones(len(k), dtype=bool)
    other[at] = False
    for host in (True, False):
        st = gpu.Stats()
        if host:
            got = gpu.query_shade(r.sc, H, wo, stats=st)
        else:
            raw, st = _dev_shade(gpu, r, H, wo, None, len(k), len(k))
            got = raw.view(np.float64).reshape(-1, 3)
        assert got[at].tobytes() == np.tile(MAGENTA, (len(at), 1)).tobytes()
        assert got[other].tobytes() == base[other].tobytes()   # the neighbouring lanes are unaffected
        assert st.rays_occluded == int(r.no[k][other].sum())


# ---------------------------------------------------------- 8. flags and errors
@pytest.mark.parametrize("name", ["config3", "config4", "dir/pokeball_csg_sun", "torture/xform_in_csg", "deep/xform_nest12"])
def test_no_cull_is_byte_identical(gpu, name):
    r = shade_ref(gpu, name)
    sa, sb = gpu.Stats(), gpu.Stats()
    a = shade(gpu, r, stats=sa)
    b = shade(gpu, r, flags=gpu.RT_FLAG_NO_CULL, stats=sb)
    assert a.tobytes() == b.tobytes() and sa.rays_occluded == sb.rays_occluded
    for f in (gpu.RT_FLAG_NO_BVH, gpu.RT_FLAG_FORCE_BVH):   # no effect
        assert shade(gpu, r, flags=f).tobytes() == a.tobytes()


def test_errors(gpu):
    lib = gpu.amd_lib()
    r = shade_ref(gpu, "config3")
    sc, n = r.sc, len(r)
    rgb, mask = np.zeros((n, 3)), r.hit.astype(np.uint8)
    hp, wp, mp, cp = (a.ctypes.data_as(_vp) for a in (r.H, r.wo, mask, rgb))
    st = gpu.Stats()
    # n == 0: RT_OK without a launch, whatever the pointers
    st.rays_traced = 123
    gpu.launch_log(True)
    try:
        assert lib.rt_query_shade(sc.handle, None, None, None, 0, None, 5, None, 0, None, C.byref(st)) == 0
        assert lib.rt_query_shade_device(sc.handle, None, None, None, 0, None, -1, None, 0, None, None, None) == 0
        assert gpu.query_shade(sc, np.zeros(0, dtype=gpu.HIT_DTYPE), np.zeros((0, 3))).shape == (0, 3)
        assert gpu.launch_log_get() == []
    finally:
        gpu.launch_log(False)
    assert (st.rays_intersect, st.rays_occluded, st.rays_traced, st.ms_kernel, st.n_gpus) == (0, 0, 0, 0.0, 1)
    # NULL arguments
    for rc in (lib.rt_query_shade(None, hp, wp, mp, n, None, -1, None, 0, cp, None),
               lib.rt_query_shade(sc.handle, None, wp, mp, n, None, -1, None, 0, cp, None),
               lib.rt_query_shade(sc.handle, hp, None, mp, n, None, -1, None, 0, cp, None),
               lib.rt_query_shade(sc.handle, hp, wp, mp, n, None, -1, None, 0, None, None),
               lib.rt_query_shade(sc.handle, hp, wp, mp, n, None, 2, None, 0, cp, None),
               lib.rt_query_shade_device(None, hp, wp, mp, n, None, -1, None, 0, cp, None, None),
               lib.rt_query_shade_device(sc.handle, None, wp, mp, n, None, -1, None, 0, cp, None, None),
               lib.rt_query_shade_device(sc.handle, hp, None, mp, n, None, -1, None, 0, cp, None, None),
               lib.rt_query_shade_device(sc.handle, hp, wp, mp, n, None, -1, None, 0, None, None, None),
               lib.rt_query_shade_device(sc.handle, hp, wp, mp, n, None, 1, None, 0, cp, None, None)):
        assert rc == gpu.RT_ERR_INVALID_ARG
        assert "NULL" in gpu.last_error()
    # refused flags, with a message (also at n == 0); NULL stats are fine
    for flag, word in ((gpu.RT_FLAG_FP32, "FP32"), (gpu.RT_FLAG_COUNT_OPS, "COUNT_OPS")):
        assert lib.rt_query_shade(sc.handle, hp, wp, mp, n, None, -1, None, flag, cp, None) == gpu.RT_ERR_UNSUPPORTED
        assert word in gpu.last_error()
        assert lib.rt_query_shade(sc.handle, None, None, None, 0, None, -1, None, flag, None, None) == gpu.RT_ERR_UNSUPPORTED
        with pytest.raises(gpu.RTError) as e:
            shade(gpu, r, flags=flag)
        assert e.value.code == gpu.RT_ERR_UNSUPPORTED
    assert lib.rt_query_shade(sc.handle, hp, wp, mp, n, None, -1, None, 1 << 20, cp, None) == gpu.RT_ERR_INVALID_ARG
    assert lib.rt_query_shade(sc.handle, hp, wp, mp, n, None, -1, None, 0, cp, None) == 0
    assert rgb.tobytes() == shade(gpu, r).tobytes()


def test_scene_beyond_the_big_stacks_is_refused(gpu):
    leaves = [{"sphere": {"position": [0.01 * i, 0, -2], "radius": 0.5, "color": {"diffuse": [1, 1, 1]}}}
              for i in range(80)]
    node = leaves[-1]
    for leaf in reversed(leaves[:-1]):
        node = {"csg": {"operator": "union", "left": leaf, "right": node}}
    sc = gpu.load_scene_from_json_text(json.dumps({"screen": {"dpi": 4, "dimensions": [2, 2], "position": [-1, -1, 0],
                                                              "observer": [0, 0, 3]}, "objects": [node]}))
    h = np.zeros(1, dtype=gpu.HIT_DTYPE)
    h["t"], h["p"], h["n"] = 2.5, [[0, 0, -1.5]], [[0, 0, 1]]
    with pytest.raises(gpu.RTError) as e:
        gpu.query_shade(sc, h, [[0, 0, 1]])
    assert e.value.code == gpu.RT_ERR_UNSUPPORTED and "CSG operand depth 80" in str(e.value)
    # and the next query works
    r = shade_ref(gpu, "config3")
    got = shade(gpu, r, slice(0, 64))
    assert float(np.abs(got - r.rgb[:64]).max()) <= TOL


# --------------------------------------- 9. a host batch larger than one chunk
def test_host_batch_larger_than_one_chunk(gpu):
    """More entries than one host chunk (2^20): the chunks' colours in order, the counts scaled."""
    r = shade_ref(gpu, "config3")
    n = (1 << 20) + 69
    reps, rest = divmod(n, len(r))
    s_all, s_rest = gpu.Stats(), gpu.Stats()
    small = shade(gpu, r, stats=s_all)
    shade(gpu, r, slice(0, rest), stats=s_rest)
    H, wo = np.tile(r.H, reps + 1)[:n], np.tile(r.wo, (reps + 1, 1))[:n]
    mask = np.tile(r.hit.astype(np.uint8), reps + 1)[:n]
    st = gpu.Stats()
    got = gpu.query_shade(r.sc, H, wo, mask, stats=st)
    assert got.tobytes() == np.tile(small, (reps + 1, 1))[:n].tobytes()
    assert st.rays_occluded == reps * s_all.rays_occluded + s_rest.rays_occluded > 0
    assert st.rays_intersect == 0 and st.rays_traced == st.rays_occluded


def test_small_host_chunks_are_the_default_chunk(gpu):
    """The host form's chunk forced to 100 hits (rt_test_camera_chunk_rays sets
    the one chunk size of every batched call): 1000 hits cross ten chunks, each
    ending in a partial wave.  Once with a mask that blanks a whole chunk, once
    with the call's own lights (their upload must outlive the first chunk),
    then without lights again (the scene's own still shade).  The same bytes
    and counts as at the default chunk."""
    r = shade_ref(gpu, "config4")
    n = 1000
    reps = -(-n // len(r))
    H, wo = np.tile(r.H, reps)[:n], np.tile(r.wo, (reps, 1))[:n]
    hit = np.tile(r.hit, reps)[:n]
    blank = hit.copy()
    blank[300:400] = False   # (the fourth chunk of 100)
    lights = override_lights("config4", 3)
    d = r.sc.desc
    assert len(lights) >= 2 and lights != [(list(d.lights[i].pos), list(d.lights[i].intensity)) for i in range(d.n_lights)]

    def run():
        out = []
        for mask, lg in ((blank, None), (hit, lights), (hit, None)):
            st = gpu.Stats()
            rgb = gpu.query_shade(r.sc, H, wo, mask.astype(np.uint8), lg, None, 0, st)
            out.append((rgb.tobytes(), (st.rays_intersect, st.rays_occluded, st.rays_traced)))
        return out

    want = run()
    gpu.camera_chunk_rays(100)
    try:
        gpu.launch_log(True)
        got = run()
        launches = gpu.launch_log_get()
    finally:
        gpu.launch_log(False)
        gpu.camera_chunk_rays(0)
    assert len(launches) == 3 * 10 and all("k_shade" in k for k in launches)   # (ten chunks a call)
    assert got == want
    rgb = [np.frombuffer(b, dtype=np.float64).reshape(n, 3) for b, _ in want]
    assert rgb[0][300:400].tobytes() == np.tile(r.background, (100, 1)).tobytes()
    assert rgb[1].tobytes() != rgb[2].tobytes()   # (the call's lights, then the scene's own)
    # the scene's own lights: this file's reference for them, and the oracle's count
    assert np.abs(rgb[2][hit] - np.tile(r.rgb, (reps, 1))[:n][hit]).max() <= TOL
    assert want[2][1] == (0, int(np.tile(r.no, reps)[:n][hit].sum()), int(np.tile(r.no, reps)[:n][hit].sum()))
    assert want[0][1][1] == int(np.tile(r.no, reps)[:n][blank].sum()) > 0


# ----------------------------------------------------------------- 10. residency
def test_frame_shade_query_frame_share_the_resident_scene(gpu):
    """Frame -> shade query -> intersect query -> frame of one scene: the
    scene is compiled and uploaded once (rt_setup_times[0] stops growing);
    then the reverse order on a second handle."""
    lib = gpu.amd_lib()
    r = shade_ref(gpu, "config4")
    c = case(gpu, "config4")
    sc = gpu.load_scene_from_json_text(SCENES["config4"][0])   # a scene handle no frame or query has seen
    t = (C.c_double * 4)()

    def scene_ms():
        assert lib.rt_setup_times(t, 4) == 0
        return t[0]

    def q(s):
        return gpu.query_shade(s, r.H, r.wo, r.hit.astype(np.uint8))

    ms0 = scene_ms()
    W, H = sc.width, sc.height
    fb = gpu.Tracer(sc, W, H, 0).render()
    ms1 = scene_ms()
    assert ms1 > ms0
    q1 = q(sc)
    h1 = gpu.query_intersect(sc, c.rays["o"], c.rays["d"])
    fb2 = gpu.Tracer(sc, W, H, 0).render()
    assert scene_ms() == ms1
    assert np.array_equal(fb, fb2) and q1.tobytes() == q(r.sc).tobytes()
    assert h1.records.tobytes() == gpu.query_intersect(c.scene, c.rays["o"], c.rays["d"]).records.tobytes()
    # the reverse: a fresh handle's intersect query, its shade query, then its frame
    sc2 = gpu.load_scene_from_json_text(SCENES["config4"][0])
    ms2 = scene_ms()
    h2 = gpu.query_intersect(sc2, c.rays["o"], c.rays["d"])
    ms3 = scene_ms()
    assert ms3 > ms2
    q2 = q(sc2)
    fb3 = gpu.Tracer(sc2, W, H, 0).render()
    assert scene_ms() == ms3
    assert np.array_equal(fb, fb3) and q2.tobytes() == q1.tobytes() and h2.records.tobytes() == h1.records.tobytes()


# -------------------------------------------------------------------- 11. census
@pytest.mark.parametrize("recipe", scenes.shade_recipes(), ids=lambda r: r.row)
def test_census(gpu, recipe):
    """Every row of the shade tables: a 256-entry query of its recipe's scene
    launches exactly that row, and its colours and counts are the oracle's."""
    r = shade_ref(gpu, "census/" + recipe.scene_name)
    assert len(r) == 256
    gpu.launch_log(True)
    try:
        got = shade(gpu, r, flags=recipe.flags)
        log = gpu.launch_log_get()
    finally:
        gpu.launch_log(False)
    assert log == [recipe.row]
    check(gpu, r, got, recipe.row, recipe.flags)
    assert r.hit.sum() >= len(r) // 4 and r.no.sum() > 0
