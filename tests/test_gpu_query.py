"""Batched ray queries on the GPU (rt_query_intersect / rt_query_occluded and
their *_device forms: Scene::intersect / Scene::occluded, scene.cpp:10-42)
against the CPU oracle's oracle_scene_intersect / oracle_scene_occluded.

Rays per scene (fixed seed): 384 pixel-centre camera rays at random pixels and
384 surface-to-surface rays (from p_a + 1e-3 n_a of one primary hit toward
p_b + N(0, 0.05^2) of another, direction unnormalised), shuffled together so
that every wave is incoherent.

Bar: hit flag, mat and front_face equal for every ray; t and p within 1e-5
relative to max(1, |value|), n within 1e-5 absolute (the project's parity
bar); occluded exactly equal.  A ray may be left out only if the ORACLE alone
is unstable on it (its hit flag or mat changes when the origin moves +-1e-7
along an axis), at most 1 % of a scene's rays; with this recipe that happens
for none of them, so the cap is a safeguard."""
import ctypes as C
import json

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

TOL = 1e-5
N_CAM = N_SURF = 384
SEED = 20240611
INF = float("inf")
_dp = C.POINTER(C.c_double)


# ------------------------------------------------------------------- scenes
def _scene_texts():
    out = {}
    for k, v in scenes.torture_scenes(dpi=24).items():
        out["torture/" + k] = (json.dumps(v), None)
    for k, v in scenes.deep_scenes().items():
        out["deep/" + k] = (json.dumps(v), None)
    for n in (3, 4, 5):
        out[f"config{n}"] = (scenes.config_json(n, dpi=24)[0], None)
    out["bvh/ties"] = (json.dumps(scenes.bvh_scenes(16)["ties"]), None)
    out["dir/pokeball_csg_sun"] = scenes.dir_light_cases()["pokeball_csg_sun"]
    return out


SCENES = _scene_texts()
_cache = {}


class Case:
    """One scene: its rays and the oracle's answers, computed once."""

    def __init__(self, rt, name):
        text, lights = SCENES[name]
        sc = rt.load_scene_from_json_text(text)
        self._build(rt, rt.with_dir_lights(sc, lights) if lights else sc, SEED + sorted(SCENES).index(name), name)

    def _build(self, rt, scene, seed, name=""):
        """The ray recipe on a loaded scene (for the scene families of other files)."""
        self.scene = scene
        self.rt, self.olib, self.desc = rt, rt.oracle_lib(), self.scene.desc_ptr
        rng = np.random.default_rng(seed)
        W, H = self.scene.width, self.scene.height
        # pixel-centre camera rays (Camera::generate_ray) at random pixels
        cam_o, cam_d = np.empty((N_CAM, 3)), np.empty((N_CAM, 3))
        px = np.stack([rng.integers(0, W, N_CAM), rng.integers(0, H, N_CAM)], axis=1)
        o3, d3 = (C.c_double * 3)(), (C.c_double * 3)()
        for k, (i, j) in enumerate(px):
            self.olib.oracle_camera_ray(self.desc, int(i), int(j), 0.0, 0.0, 0, o3, d3)
            cam_o[k], cam_d[k] = list(o3), list(d3)
        hit, rec = self.oracle_intersect(rt.make_rays(cam_o, cam_d))
        self.cam_rays, self.cam_hit, self.cam_rec = rt.make_rays(cam_o, cam_d), hit, rec
        prim_p, prim_n = rec["p"][hit], rec["n"][hit]
        assert len(prim_p) >= 2, name
        # surface-to-surface rays between primary hits
        a, b = rng.integers(0, len(prim_p), N_SURF), rng.integers(0, len(prim_p), N_SURF)
        so = prim_p[a] + 1e-3 * prim_n[a]
        target = prim_p[b] + rng.normal(0.0, 0.05, (N_SURF, 3))
        sd = target - so
        dist = np.sqrt((sd * sd).sum(axis=1))
        o, d = np.concatenate([cam_o, so]), np.concatenate([cam_d, sd])
        seg_tmax = np.concatenate([np.full(N_CAM, INF), dist])
        order = rng.permutation(N_CAM + N_SURF)
        self.rays = rt.make_rays(o[order], d[order], 1e-4, INF)             # closest hit
        self.seg_rays = rt.make_rays(o[order], d[order], 1e-4, seg_tmax[order])   # occluded: segments
        self.ref_hit, self.ref_rec = self.oracle_intersect(self.rays)
        self.ref_occ = self.oracle_occluded(self.seg_rays)

    # the oracle, ray by ray
    def _one(self, ray, occluded=False, shift=None):
        o = np.array(ray["o"], dtype=np.float64)
        if shift is not None:
            o = o + shift
        d = np.ascontiguousarray(ray["d"], dtype=np.float64)
        if occluded:
            return bool(self.olib.oracle_scene_occluded(self.desc, o.ctypes.data_as(_dp), d.ctypes.data_as(_dp),
                                                        float(ray["tmin"]), float(ray["tmax"]))), None
        h = self.rt.OracleHit()
        ok = self.olib.oracle_scene_intersect(self.desc, o.ctypes.data_as(_dp), d.ctypes.data_as(_dp),
                                              float(ray["tmin"]), float(ray["tmax"]), C.byref(h))
        return bool(ok), h

    def oracle_intersect(self, rays):
        hit = np.zeros(len(rays), dtype=bool)
        rec = np.zeros(len(rays), dtype=self.rt.HIT_DTYPE)
        for k, ray in enumerate(rays):
            hit[k], h = self._one(ray)
            if hit[k]:
                rec[k] = (h.t, tuple(h.p), tuple(h.n), h.mat, h.front_face)
        return hit, rec

    def oracle_occluded(self, rays):
        return np.array([self._one(ray, occluded=True)[0] for ray in rays], dtype=bool)

    def oracle_unstable(self, ray, occluded, step=1e-7):
        """The oracle's own answer (hit flag, mat) changes under a +-step shift of the origin."""
        def key(shift):
            ok, h = self._one(ray, occluded, shift)
            return (ok, h.mat if (h is not None and ok) else -1)
        base = key(None)
        for ax in range(3):
            for sgn in (1.0, -1.0):
                shift = np.zeros(3)
                shift[ax] = sgn * step
                if key(shift) != base:
                    return True
        return False


def case(rt, name):
    if name not in _cache:
        _cache[name] = Case(rt, name)
    return _cache[name]


# --------------------------------------------------------------------- bars
def _rel(a, b, floor=None):
    return np.abs(a - b) / (np.maximum(1.0, np.abs(b)) if floor is None else floor)


def check_hits(c, rays, got, ref_hit, ref_rec, what, step=1e-7, scale=None):
    """got (QueryHits) against the oracle's (ref_hit, ref_rec) at the bar of
    this file; returns the largest (t, p, n) differences over the compared hits.
    step: the instability probe's shift of the origin.  scale: for a scene of
    another size or place (tests/test_gpu_placed.py), t and p are judged
    relative to max(scale, |t_ref|): a far hit point's own magnitude would
    hide an error of the scene's size."""
    assert len(got) == len(rays)
    g = got.records
    bad = (got.hit != ref_hit)
    both = got.hit & ref_hit
    bad |= both & ((g["mat"] != ref_rec["mat"]) | (g["front_face"] != ref_rec["front_face"]))
    floor = None if scale is None else np.maximum(scale, np.abs(ref_rec["t"]))
    with np.errstate(invalid="ignore", divide="ignore"):
        dt = np.where(both, _rel(g["t"], ref_rec["t"], floor), 0.0)
        dp = np.where(both[:, None], _rel(g["p"], ref_rec["p"], None if floor is None else floor[:, None]), 0.0).max(axis=1)
    dn = np.where(both[:, None], np.abs(g["n"] - ref_rec["n"]), 0.0).max(axis=1)
    with np.errstate(invalid="ignore"):
        bad |= both & ~((dt <= TOL) & (dp <= TOL) & (dn <= TOL))
    # a miss is reported as mat -1 and zeros
    miss = g[~got.hit]
    assert np.all(miss["mat"] == -1) and not miss["t"].any() and not miss["p"].any() and not miss["n"].any() \
        and not miss["front_face"].any(), what
    left_out = [k for k in np.flatnonzero(bad) if c.oracle_unstable(rays[k], False, step)]
    wrong = sorted(set(np.flatnonzero(bad).tolist()) - set(left_out))
    keep = np.ones(len(rays), dtype=bool)
    keep[left_out] = False
    mx = (float(dt[keep].max(initial=0.0)), float(dp[keep].max(initial=0.0)), float(dn[keep].max(initial=0.0)))
    print(f"  {what}: {len(rays)} rays, {int(ref_hit.sum())} hits, max rel dt={mx[0]:.3g} dp={mx[1]:.3g} "
          f"abs dn={mx[2]:.3g}, left out {len(left_out)}")
    assert not wrong, (what, wrong[:8], [(g[k], ref_rec[k], bool(ref_hit[k])) for k in wrong[:2]])
    assert len(left_out) <= len(rays) // 100, (what, left_out)
    return mx


def same_value(got, ref, tol=TOL, relative=True):
    """Elementwise: NaN where ref is NaN, the same infinity where ref is
    infinite, within tol (relative to max(1, |ref|), or absolute) where ref is
    finite."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(ref)
        close = np.abs(got - ref) <= tol * (np.maximum(1.0, np.abs(ref)) if relative else 1.0)
        return np.where(fin, close & np.isfinite(got), (got == ref) | (np.isnan(got) & np.isnan(ref)))


def check_hits_every_ray(rays, got, ref_hit, ref_rec, what):
    """check_hits for rays whose oracle answer may be non-finite (a NaN or
    infinite ray component, tests/test_gpu_leaves.py): the same bar where the
    oracle is finite, NaN for NaN and the same infinity otherwise, and no ray
    left out - the reference's answer on such a ray is exact, not unstable.
    Returns the largest finite (t, p, n) differences."""
    assert len(got) == len(rays) == len(ref_hit)
    g = got.records
    bad = (got.hit != ref_hit)
    both = got.hit & ref_hit
    bad |= both & ((g["mat"] != ref_rec["mat"]) | (g["front_face"] != ref_rec["front_face"]))
    bad |= both & ~(same_value(g["t"], ref_rec["t"]) & same_value(g["p"], ref_rec["p"]).all(axis=1)
                    & same_value(g["n"], ref_rec["n"], relative=False).all(axis=1))
    miss = g[~got.hit]
    assert np.all(miss["mat"] == -1) and not miss["t"].any() and not miss["p"].any() and not miss["n"].any() \
        and not miss["front_face"].any(), what

    def largest(f, rel):
        a, b = g[f][both].reshape(-1), ref_rec[f][both].reshape(-1)
        k = np.isfinite(b) & np.isfinite(a)
        return float((np.abs(a[k] - b[k]) / (np.maximum(1.0, np.abs(b[k])) if rel else 1.0)).max(initial=0.0))

    mx = (largest("t", True), largest("p", True), largest("n", False))
    nonfinite = int((both & ~(np.isfinite(ref_rec["t"]) & np.isfinite(ref_rec["p"]).all(axis=1)
                              & np.isfinite(ref_rec["n"]).all(axis=1))).sum())
    print(f"  {what}: {len(rays)} rays, {int(ref_hit.sum())} hits ({nonfinite} non-finite), max rel dt={mx[0]:.3g} "
          f"dp={mx[1]:.3g} abs dn={mx[2]:.3g}, left out 0")
    wrong = np.flatnonzero(bad).tolist()
    assert not wrong, (what, wrong[:8], [(g[k], ref_rec[k], bool(ref_hit[k])) for k in wrong[:2]])
    return mx


def check_occluded(c, rays, got, ref, what, step=1e-7):
    assert got.dtype == bool and len(got) == len(rays)
    bad = np.flatnonzero(got != ref)
    left_out = [k for k in bad if c.oracle_unstable(rays[k], True, step)]
    wrong = sorted(set(bad.tolist()) - set(left_out))
    print(f"  {what}: {len(rays)} rays, {int(ref.sum())} occluded, left out {len(left_out)}")
    assert not wrong, (what, wrong[:8])
    assert len(left_out) <= len(rays) // 100, (what, left_out)


def q_isect(rt, sc, rays, flags=0, stats=None):
    return rt.query_intersect(sc, rays["o"], rays["d"], rays["tmin"], rays["tmax"], flags, stats)


def q_occl(rt, sc, rays, flags=0, stats=None):
    return rt.query_occluded(sc, rays["o"], rays["d"], rays["tmin"], rays["tmax"], flags, stats)


# ------------------------------------------------------------ every scene
@pytest.mark.parametrize("name", sorted(SCENES))
def test_intersect_matches_oracle(gpu, name):
    c = case(gpu, name)
    st = gpu.Stats()
    got = q_isect(gpu, c.scene, c.rays, stats=st)
    assert (st.rays_intersect, st.rays_occluded, st.rays_traced) == (len(c.rays), 0, len(c.rays))
    assert st.ms_kernel > 0.0 and st.ms_total >= st.ms_kernel and st.n_gpus == 1
    check_hits(c, c.rays, got, c.ref_hit, c.ref_rec, name + " intersect")
    assert c.ref_hit.sum() >= len(c.rays) // 4   # (the batch does exercise the objects)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_occluded_matches_oracle(gpu, name):
    c = case(gpu, name)
    st = gpu.Stats()
    got = q_occl(gpu, c.scene, c.seg_rays, stats=st)
    assert (st.rays_intersect, st.rays_occluded, st.rays_traced) == (0, len(c.rays), len(c.rays))
    check_occluded(c, c.seg_rays, got, c.ref_occ, name + " occluded")
    assert c.ref_occ.any()   # (the eye-inside scenes occlude every segment)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_no_cull_is_byte_identical(gpu, name):
    c = case(gpu, name)
    a, b = q_isect(gpu, c.scene, c.rays), q_isect(gpu, c.scene, c.rays, flags=gpu.RT_FLAG_NO_CULL)
    assert a.records.tobytes() == b.records.tobytes() and np.array_equal(a.hit, b.hit)
    assert np.array_equal(q_occl(gpu, c.scene, c.seg_rays), q_occl(gpu, c.scene, c.seg_rays, flags=gpu.RT_FLAG_NO_CULL))


# ------------------------------------------------------------------ ranges
@pytest.mark.parametrize("name", ["config5", "torture/csg_ops", "torture/rotation_scaling", "torture/xform_in_csg",
                                  "bvh/ties"])
def test_ranges_around_the_first_hit(gpu, name):
    """tmax just below the first hit's t: a miss or a farther object, as in the
    oracle; tmin just above it: the next surface (spheres, CSG, transforms,
    and the exact ties)."""
    c = case(gpu, name)
    rays = c.cam_rays[c.cam_hit]
    t0 = c.cam_rec["t"][c.cam_hit]
    assert len(rays) >= 64
    below, above = rays.copy(), rays.copy()
    below["tmax"] = t0 * (1.0 - 1e-9)
    above["tmin"] = t0 * (1.0 + 1e-9)
    for tag, r in (("tmax<t0", below), ("tmin>t0", above)):
        ref_hit, ref_rec = c.oracle_intersect(r)
        check_hits(c, r, q_isect(gpu, c.scene, r), ref_hit, ref_rec, f"{name} {tag}")
        check_occluded(c, r, q_occl(gpu, c.scene, r), c.oracle_occluded(r), f"{name} {tag} occluded")
        if tag == "tmin>t0":
            assert ref_hit.any() and np.all(ref_rec["t"][ref_hit] > t0[ref_hit])
        if tag == "tmax<t0":
            assert np.all(ref_rec["t"][ref_hit] < t0[ref_hit])


# -------------------------------------------------------------- wave tails
def _dev_intersect(rt, sc, rays, n, cap, stream=None, flags=0):
    """rt_query_intersect_device on the first n rays into buffers of cap records filled with 0xAB."""
    lib = rt.amd_lib()
    d_rays = rt.DeviceBuffer(max(1, len(rays)) * 64)
    d_rays.from_host(rays)
    d_hits, d_mask = rt.DeviceBuffer(cap * 64), rt.DeviceBuffer(cap)
    d_hits.from_host(np.full(cap * 64, 0xAB, dtype=np.uint8))
    d_mask.from_host(np.full(cap, 0xAB, dtype=np.uint8))
    st = rt.Stats()
    rc = lib.rt_query_intersect_device(sc.handle, d_rays.ptr, n, flags, d_hits.ptr, d_mask.ptr,
                                       stream.handle if stream else None, C.byref(st))
    assert rc == 0, rt.last_error()
    return d_hits.to_host(np.uint8), d_mask.to_host(np.uint8), st


def _dev_occluded(rt, sc, rays, n, cap, stream=None):
    lib = rt.amd_lib()
    d_rays = rt.DeviceBuffer(max(1, len(rays)) * 64)
    d_rays.from_host(rays)
    d_occ = rt.DeviceBuffer(cap)
    d_occ.from_host(np.full(cap, 0xAB, dtype=np.uint8))
    st = rt.Stats()
    rc = lib.rt_query_occluded_device(sc.handle, d_rays.ptr, n, 0, d_occ.ptr, stream.handle if stream else None,
                                      C.byref(st))
    assert rc == 0, rt.last_error()
    return d_occ.to_host(np.uint8), st


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_wave_tails(gpu, n):
    c = case(gpu, "config4")
    reps = -(-n // len(c.rays))
    rays, segs = np.tile(c.rays, reps)[:n], np.tile(c.seg_rays, reps)[:n]
    ref_hit, ref_rec = np.tile(c.ref_hit, reps)[:n], np.tile(c.ref_rec, reps)[:n]
    got = q_isect(gpu, c.scene, rays)
    check_hits(c, rays, got, ref_hit, ref_rec, f"config4 n={n}")
    occ = q_occl(gpu, c.scene, segs)
    check_occluded(c, segs, occ, np.tile(c.ref_occ, reps)[:n], f"config4 n={n} occluded")
    # the device entry points: the same bytes, and nothing written beyond n
    cap = n + 200
    hits_b, mask_b, st = _dev_intersect(gpu, c.scene, rays, n, cap)
    assert st.rays_intersect == n
    assert hits_b[:n * 64].tobytes() == got.records.tobytes()
    assert np.array_equal(mask_b[:n], got.hit.astype(np.uint8))
    assert np.all(hits_b[n * 64:] == 0xAB) and np.all(mask_b[n:] == 0xAB)
    occ_b, st = _dev_occluded(gpu, c.scene, segs, n, cap)
    assert st.rays_occluded == n
    assert np.array_equal(occ_b[:n], occ.astype(np.uint8)) and np.all(occ_b[n:] == 0xAB)


def test_device_entry_points_on_a_stream(gpu):
    c = case(gpu, "torture/xform_in_csg")
    n = len(c.rays)
    got, occ = q_isect(gpu, c.scene, c.rays), q_occl(gpu, c.scene, c.seg_rays)
    stream = gpu.Stream()
    try:
        hits_b, mask_b, _ = _dev_intersect(gpu, c.scene, c.rays, n, n, stream=stream)
        occ_b, _ = _dev_occluded(gpu, c.scene, c.seg_rays, n, n, stream=stream)
    finally:
        stream.destroy()
    assert hits_b.tobytes() == got.records.tobytes() and np.array_equal(mask_b, got.hit.astype(np.uint8))
    assert np.array_equal(occ_b, occ.astype(np.uint8))
    # the hit mask is optional
    lib = gpu.amd_lib()
    d_rays, d_hits = gpu.DeviceBuffer(n * 64), gpu.DeviceBuffer(n * 64)
    d_rays.from_host(c.rays)
    assert lib.rt_query_intersect_device(c.scene.handle, d_rays.ptr, n, 0, d_hits.ptr, None, None, None) == 0
    assert d_hits.to_host(np.uint8).tobytes() == got.records.tobytes()


def test_host_batch_larger_than_one_chunk(gpu):
    """More rays than one host chunk (2^20): the chunks' results in order."""
    c = case(gpu, "config5")
    n = (1 << 20) + 777
    reps = -(-n // len(c.rays))
    rays, segs = np.tile(c.rays, reps)[:n], np.tile(c.seg_rays, reps)[:n]
    small, small_occ = q_isect(gpu, c.scene, c.rays), q_occl(gpu, c.scene, c.seg_rays)
    st = gpu.Stats()
    got = q_isect(gpu, c.scene, rays, stats=st)
    assert st.rays_intersect == n
    assert got.records.tobytes() == np.tile(small.records, reps)[:n].tobytes()
    assert np.array_equal(got.hit, np.tile(small.hit, reps)[:n])
    assert np.array_equal(q_occl(gpu, c.scene, segs), np.tile(small_occ, reps)[:n])


def test_small_host_chunks_are_the_default_chunk(gpu):
    """The host forms' chunk forced to 100 rays (rt_test_camera_chunk_rays sets
    the one chunk size of every batched call): 1000 rays cross ten chunks, each
    ending in a partial wave (100 is no multiple of 64) whose tail lanes replay
    a ray and must not store.  The same bytes and stats as at the default chunk."""
    c = case(gpu, "config4")
    n = 1000
    reps = -(-n // len(c.rays))
    rays, segs = np.tile(c.rays, reps)[:n], np.tile(c.seg_rays, reps)[:n]

    def run():
        si, so = gpu.Stats(), gpu.Stats()
        hits, occ = q_isect(gpu, c.scene, rays, stats=si), q_occl(gpu, c.scene, segs, stats=so)
        return (hits.records.tobytes(), hits.hit.tobytes(), occ.tobytes(),
                [(s.rays_intersect, s.rays_occluded, s.rays_traced) for s in (si, so)])

    want = run()
    gpu.camera_chunk_rays(100)
    try:
        gpu.launch_log(True)
        got = run()
        launches = gpu.launch_log_get()
    finally:
        gpu.launch_log(False)
        gpu.camera_chunk_rays(0)
    assert len(launches) == 2 * 10   # (ten chunks a call)
    assert got == want
    assert want[3] == [(n, 0, n), (0, n, n)]
    hit = np.frombuffer(want[1], dtype=bool)
    assert hit.any() and not hit.all()   # (the optional mask says something)


# ---------------------------------------------------- degenerate directions
def test_zero_length_direction_is_plus_y(gpu):
    """Ray::Ray normalises through Dir3::normalized (core.h:95-101, 278): a
    direction of length <= 1e-6 becomes (0, 1, 0)."""
    c = case(gpu, "config5")
    # under three spheres of config 5 (the rays go up into them), at the eye, and under the floor
    origins = np.array([[-3.5, -1.55, -2.0], [0.5, -1.58, -2.0], [2.5, -1.0, -4.0], [0.0, 0.0, 5.0], [0.0, -3.0, -2.0]])
    for d in ([0.0, 0.0, 0.0], [1e-300, 0.0, 0.0], [0.0, -1e-300, 1e-300], [5e-7, 0.0, 0.0]):
        rays = gpu.make_rays(origins, np.tile(np.array(d), (len(origins), 1)))
        up = gpu.make_rays(origins, np.tile(np.array([0.0, 1.0, 0.0]), (len(origins), 1)))
        ref_hit, ref_rec = c.oracle_intersect(rays)
        got = q_isect(gpu, c.scene, rays)
        check_hits(c, rays, got, ref_hit, ref_rec, f"config5 d={d}")
        assert ref_hit[:3].all() and not ref_hit[3]
        assert got.records.tobytes() == q_isect(gpu, c.scene, up).records.tobytes()
        assert np.array_equal(q_occl(gpu, c.scene, rays), c.oracle_occluded(rays))


# ---------------------------------------------------------------- residency
def test_query_frame_query_share_the_resident_scene(gpu):
    """A query, a frame and a query of one scene: the scene is compiled and
    uploaded once (rt_setup_times[0] stops growing), the frame matches the
    oracle at the usual bar and both queries return the same bytes."""
    lib = gpu.amd_lib()
    c = case(gpu, "config4")
    sc = gpu.load_scene_from_json_text(SCENES["config4"][0])   # a scene handle no frame or query has seen
    t = (C.c_double * 4)()

    def scene_ms():
        assert lib.rt_setup_times(t, 4) == 0
        return t[0]

    ms0 = scene_ms()
    q1, o1 = q_isect(gpu, sc, c.rays), q_occl(gpu, sc, c.seg_rays)
    ms1 = scene_ms()
    assert ms1 > ms0
    W, H = sc.width, sc.height
    st = gpu.Stats()
    fb = gpu.Tracer(sc, W, H, 0).render(st)
    q2, o2 = q_isect(gpu, sc, c.rays), q_occl(gpu, sc, c.seg_rays)
    fb2 = gpu.Tracer(sc, W, H, 0).render()
    assert scene_ms() == ms1
    ref, ost = gpu.oracle_render(sc, W, H, 0, threads=8)
    assert float(np.abs(fb - ref).max()) <= TOL
    assert (st.rays_intersect, st.rays_occluded) == (ost.rays_intersect, ost.rays_occluded)
    assert np.array_equal(fb, fb2)
    assert q1.records.tobytes() == q2.records.tobytes() and np.array_equal(q1.hit, q2.hit) and np.array_equal(o1, o2)
    check_hits(c, c.rays, q1, c.ref_hit, c.ref_rec, "config4 (fresh handle)")


# ------------------------------------------------------------------- errors
def test_errors(gpu):
    lib = gpu.amd_lib()
    c = case(gpu, "config3")
    sc, rays, n = c.scene, c.rays, len(c.rays)
    hits, mask = np.zeros(n, dtype=gpu.HIT_DTYPE), np.zeros(n, dtype=np.uint8)
    rp, hp, mp = (x.ctypes.data_as(C.c_void_p) for x in (rays, hits, mask))
    st = gpu.Stats()
    # n == 0: RT_OK without a launch, whatever the pointers
    st.rays_traced = 123
    assert lib.rt_query_intersect(sc.handle, None, 0, 0, None, None, C.byref(st)) == 0
    assert (st.rays_intersect, st.rays_traced, st.ms_kernel) == (0, 0, 0.0)
    assert lib.rt_query_occluded(sc.handle, None, 0, 0, None, None) == 0
    assert lib.rt_query_intersect_device(sc.handle, None, 0, 0, None, None, None, None) == 0
    assert lib.rt_query_occluded_device(sc.handle, None, 0, 0, None, None, None) == 0
    assert len(gpu.query_intersect(sc, np.zeros((0, 3)), np.zeros((0, 3)))) == 0
    # NULL arguments
    for rc in (lib.rt_query_intersect(None, rp, n, 0, hp, mp, None),
               lib.rt_query_intersect(sc.handle, None, n, 0, hp, mp, None),
               lib.rt_query_intersect(sc.handle, rp, n, 0, None, mp, None),
               lib.rt_query_occluded(None, rp, n, 0, mp, None),
               lib.rt_query_occluded(sc.handle, None, n, 0, mp, None),
               lib.rt_query_occluded(sc.handle, rp, n, 0, None, None),
               lib.rt_query_intersect_device(sc.handle, None, n, 0, hp, None, None, None),
               lib.rt_query_occluded_device(sc.handle, rp, n, 0, None, None, None)):
        assert rc == gpu.RT_ERR_INVALID_ARG
        assert "NULL" in gpu.last_error()
    # refused flags, with a message; NULL stats and a NULL hit mask are fine
    for flag, word in ((gpu.RT_FLAG_FP32, "FP32"), (gpu.RT_FLAG_COUNT_OPS, "COUNT_OPS")):
        assert lib.rt_query_intersect(sc.handle, rp, n, flag, hp, mp, None) == gpu.RT_ERR_UNSUPPORTED
        assert word in gpu.last_error()
        assert lib.rt_query_occluded(sc.handle, rp, n, flag, mp, None) == gpu.RT_ERR_UNSUPPORTED
        # (also at n == 0)
        assert lib.rt_query_intersect(sc.handle, None, 0, flag, None, None, None) == gpu.RT_ERR_UNSUPPORTED
        with pytest.raises(gpu.RTError) as e:
            q_isect(gpu, sc, rays, flags=flag)
        assert e.value.code == gpu.RT_ERR_UNSUPPORTED
    assert lib.rt_query_intersect(sc.handle, rp, n, 1 << 20, hp, mp, None) == gpu.RT_ERR_INVALID_ARG
    assert lib.rt_query_intersect(sc.handle, rp, n, 0, hp, None, None) == 0
    assert hits.tobytes() == q_isect(gpu, sc, rays).records.tobytes()


def test_scene_beyond_the_big_stacks_is_refused(gpu):
    leaves = [{"sphere": {"position": [0.01 * i, 0, -2], "radius": 0.5, "color": {"diffuse": [1, 1, 1]}}}
              for i in range(80)]
    node = leaves[-1]
    for leaf in reversed(leaves[:-1]):
        node = {"csg": {"operator": "union", "left": leaf, "right": node}}
    sc = gpu.load_scene_from_json_text(json.dumps({"screen": {"dpi": 4, "dimensions": [2, 2], "position": [-1, -1, 0],
                                                              "observer": [0, 0, 3]}, "objects": [node]}))
    with pytest.raises(gpu.RTError) as e:
        gpu.query_intersect(sc, [[0, 0, 3]], [[0, 0, -1]])
    assert e.value.code == gpu.RT_ERR_UNSUPPORTED and "CSG operand depth 80" in str(e.value)
    with pytest.raises(gpu.RTError) as e:
        gpu.Tracer(sc, 8, 8, 0).render()
    assert e.value.code == gpu.RT_ERR_UNSUPPORTED
