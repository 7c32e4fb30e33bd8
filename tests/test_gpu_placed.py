"""The float32 culls on translated and scaled scenes (scenes.placed,
scenes.PLACEMENTS): frames, batched queries, radiance, coherent bundles with
an origin spread, the deferred shading pipeline and far origins / odd ranges,
each against the CPU oracle at the existing files' bars and against its own
RT_FLAG_NO_CULL run, bit for bit.

Every float32 cull (ball_touch, plane_touch, the bundle cone and capsule
tests, the shadow hull and light-relative records, the CSG leaf masks, the
wave BVH chunk records, the host's float_ball) claims to be conservative:
results unchanged.  Its margins were chosen at unit scale near the origin;
here the same scenes sit 3000 and 1e6 units away (frames), up to 3e8 away and
at scales 1e-3 to 1e39 (queries: at 1e25 the float32 squares overflow, at 1e39
the float32 copies are inf), and rays start 1e7 units off or carry empty and
unbounded ranges.

Bars (unchanged): frames |fb - oracle| <= 1e-5 with identical ray counts,
paper mode array_equal; hit flag, mat, front_face and occluded exact, t and p
within 1e-5 * max(scale, |t_ref|), n within 1e-5; radiance and shading within
1e-5 with the oracle's counts.  The instability probe moves the origin by
1e-7 * scale; the caps stay 1 % (intersect, occluded, shading) and 15 of 768
(radiance).

The oracle's own unstable rays by that probe (CPU, tests/test_placed_scenes.py):
intersect and occluded 0 of 768 on all 6 scenes x 7 placements; radiance
config 5: 2 (mid, far, big, huge_far, e25, e39), 0 (tiny); reflect_refract,
csg_ops, bvh/ties and dir/pokeball_csg_sun: 1 each under every placement but
tiny (0).  At e25 and e39 the radiance scenes run at recursion limit 1
(test_placed_scenes.placed_ref says why: at full depth 213 of config 5's 768
rays are oracle-unstable there).

Measured on an MI355X (profiles/placed_scenes/gpu_tests.txt): frames within
1.2e-16 of the oracle in standard mode and equal in paper mode; every hit
record of the 72 intersect batches (42 placed, 30 far-origin / odd-range)
equal to the oracle's, t, p and n included; radiance and bundles within
2.2e-11, shading within 1.2e-16; no ray had to be left out anywhere.  Before
the fix of the clamped-light-distance cull (Culling) 9 cases
failed: every radiance and shading case at `tiny` (up to 5.5e-5) and the
frames of bvh/grid and bvh/ties at `d100_mid` (up to 7.6e-3).

Every test prints its largest differences and left-out counts."""
import numpy as np
import pytest

import scenes
import test_gpu_radiance as R
import test_gpu_shade as S
from test_gpu_query import case, check_hits, check_occluded, q_isect, q_occl
from test_placed_scenes import (FRAME_SCENES, PL, QUERY_SCENES, RADIANCE_SCENES, UNPLACED, load, oracle_frame,
                                placed_case, placed_ref, scene_dict)
from test_shade_plan import ShadeRef

pytestmark = pytest.mark.gpu

TOL = 1e-5
INF = float("inf")
GPU_FRAME_SCENES = FRAME_SCENES + ("bvh/ties", "deep/xform_nest12")
_logs, _bundles, _shade = {}, {}, {}


# --------------------------------------------------------------------- frames
def _render(rt, sc, mode, flags=0, log=False):
    """A frame of a fresh handle's first Tracer: (fb, counts[, launch log])."""
    st = rt.Stats()
    if log:
        rt.launch_log(True)
    try:
        fb = rt.Tracer(sc, sc.width, sc.height, mode, flags=flags).render(st)
        rows = rt.launch_log_get() if log else None
    finally:
        if log:
            rt.launch_log(False)
    return fb, (int(st.rays_intersect), int(st.rays_occluded)), rows


def _unplaced_log(rt, name, mode):
    if (name, mode) not in _logs:
        scene, lights = scene_dict(name)
        _logs[name, mode] = _render(rt, load(rt, scene, lights), mode, log=True)[2]
    return _logs[name, mode]


@pytest.mark.parametrize("pl", scenes.FRAME_PLACEMENTS)
@pytest.mark.parametrize("name", GPU_FRAME_SCENES)
def test_frames(gpu, name, pl):
    """Both modes against the oracle's frame of the placed scene, culling on
    and off, the BVH on and off, and the launch log: the placed scene launches
    the unplaced scene's rows (the translations that conjugate a scaling or
    rotation fold into the transform they wrap, so no scene here changes its
    row)."""
    scene, lights = scene_dict(name)
    text = scenes.placed(scene, *PL[pl])
    for mode in (0, 1):
        _, ref, counts = oracle_frame(gpu, name, pl, mode)
        sc = load(gpu, text, lights)   # a handle no frame has seen: the same first frame as the unplaced log's
        fb, got_counts, rows = _render(gpu, sc, mode, log=True)
        with np.errstate(invalid="ignore"):
            err = float(np.nanmax(np.abs(fb - ref)))
        print(f"  {name} {pl} mode {mode}: {sc.width}x{sc.height} max|d|={err:.3g} rays {got_counts} oracle {counts} "
              f"rows {rows}")
        assert got_counts == counts
        if mode == 1:
            assert np.array_equal(fb, ref, equal_nan=True)
        else:
            assert np.isfinite(fb).all() and err <= TOL
        assert rows == _unplaced_log(gpu, name, mode)
        nc, nc_counts, _ = _render(gpu, load(gpu, text, lights), mode, gpu.RT_FLAG_NO_CULL)
        assert np.array_equal(fb, nc, equal_nan=True) and nc_counts == counts
        if name.startswith("bvh/"):
            for f in (gpu.RT_FLAG_FORCE_BVH, gpu.RT_FLAG_NO_BVH):
                b, b_counts, _ = _render(gpu, sc, mode, f)
                assert np.array_equal(fb, b, equal_nan=True) and b_counts == counts


# ------------------------------------------------------ intersect and occluded
def _same_hits(a, b):
    return a.records.tobytes() == b.records.tobytes() and np.array_equal(a.hit, b.hit)


@pytest.mark.parametrize("pl", scenes.QUERY_PLACEMENTS)
@pytest.mark.parametrize("name", QUERY_SCENES)
def test_intersect_and_occluded(gpu, name, pl):
    """At e39 (float)tmax of a finite segment is inf: that is the case under test."""
    c = placed_case(gpu, name, pl)
    what = f"{name} {pl}"
    got = q_isect(gpu, c.scene, c.rays)
    check_hits(c, c.rays, got, c.ref_hit, c.ref_rec, what + " intersect", step=c.step, scale=c.scale)
    occ = q_occl(gpu, c.scene, c.seg_rays)
    check_occluded(c, c.seg_rays, occ, c.ref_occ, what + " occluded", step=c.step)
    assert c.ref_hit.sum() >= len(c.rays) // 4 and c.ref_occ.any()
    assert _same_hits(got, q_isect(gpu, c.scene, c.rays, flags=gpu.RT_FLAG_NO_CULL))
    assert np.array_equal(occ, q_occl(gpu, c.scene, c.seg_rays, flags=gpu.RT_FLAG_NO_CULL))


# ------------------------------------------------------------------- radiance
def _radiance(rt, r, what, step):
    sa, sb = rt.Stats(), rt.Stats()
    got = rt.query_radiance(r.sc, r.o, r.d, stats=sa)
    R.check(rt, r, got, what, step=step)
    nc = rt.query_radiance(r.sc, r.o, r.d, rt.RT_FLAG_NO_CULL, sb)
    assert got.tobytes() == nc.tobytes(), what
    assert (sa.rays_intersect, sa.rays_occluded) == (sb.rays_intersect, sb.rays_occluded), what


@pytest.mark.parametrize("pl", scenes.QUERY_PLACEMENTS)
@pytest.mark.parametrize("name", RADIANCE_SCENES)
def test_radiance(gpu, name, pl):
    r = placed_ref(gpu, name, pl)
    _radiance(gpu, r, f"{name} {pl} radiance", placed_case(gpu, name, pl).step)
    assert (np.abs(r.rgb - r.background).max(axis=1) > 0).sum() >= len(r) // 4


# ------------------------------------------- coherent bundles with an origin spread
BW, BH = 64, 48


def _bundle(rt, name, pl, kind):
    """A 64 x 48 grid of rays in frame order over the placed scene's screen
    rectangle: "ortho" parallel rays from the rectangle along the direction
    from the observer to the screen centre; "pinhole" rays through the grid
    from a point 0.2 * scale beside the observer.  The query tests shuffle
    their rays (every wave wider than 90 degrees: the bundle cone never culls)
    and a frame's camera call has no origin spread; these waves are narrow and
    have one."""
    key = (name, pl, kind)
    if key not in _bundles:
        c = placed_case(rt, name, pl)
        cam = c.scene.desc.camera
        P, eye = np.array(list(cam.P)), np.array(list(cam.eye))
        x, y = np.meshgrid((np.arange(BW) + 0.5) / BW, 1.0 - (np.arange(BH) + 0.5) / BH)
        grid = P + np.stack([cam.Lx * x.ravel(), cam.Ly * y.ravel(), np.zeros(BW * BH)], axis=1)
        centre = P + np.array([cam.Lx / 2.0, cam.Ly / 2.0, 0.0])
        if kind == "ortho":
            o, d = grid, np.tile(centre - eye, (BW * BH, 1))
        else:
            o = np.tile(eye + np.array([0.2 * c.scale, 0.0, 0.0]), (BW * BH, 1))
            d = grid - o
        _bundles[key] = R.Ref(rt, c.scene, o, d)
    return _bundles[key]


@pytest.mark.parametrize("kind", ["ortho", "pinhole"])
@pytest.mark.parametrize("pl", [UNPLACED, "mid", "far", "big"])
@pytest.mark.parametrize("name", ["config5", "torture/csg_ops", "torture/xform_in_csg"])
def test_bundles(gpu, name, pl, kind):
    r = _bundle(gpu, name, pl, kind)
    assert len(r) == BW * BH
    _radiance(gpu, r, f"{name} {pl} {kind} bundle", placed_case(gpu, name, pl).step)
    assert (np.abs(r.rgb - r.background).max(axis=1) > 0).sum() >= len(r) // 4


# -------------------------------------------------------------------- shading
def _shade_ref(rt, name, pl):
    if (name, pl) not in _shade:
        c = placed_case(rt, name, pl)
        _shade[name, pl] = ShadeRef(rt, c.scene, c.rays["o"], c.rays["d"])
    return _shade[name, pl]


def _pipeline(rt, r, flags=0):
    """rt_query_intersect_device, then rt_query_shade_device on its (hits, mask) in place, wo = -d."""
    lib, n = rt.amd_lib(), len(r)
    d_rays, d_hits, d_mask = rt.DeviceBuffer(n * 64), rt.DeviceBuffer(n * 64), rt.DeviceBuffer(n)
    d_wo, d_rgb = rt.DeviceBuffer(n * 24), rt.DeviceBuffer(n * 24)
    d_rays.from_host(rt.make_rays(r.o, r.d))
    d_wo.from_host(r.wo)
    assert lib.rt_query_intersect_device(r.sc.handle, d_rays.ptr, n, flags, d_hits.ptr, d_mask.ptr, None, None) == 0, \
        rt.last_error()
    st = rt.Stats()
    rt.query_shade_device(r.sc, d_hits, d_wo, d_mask, n, d_rgb, flags=flags, stats=st)
    return d_rgb.to_host(np.float64, (n, 3)), d_mask.to_host(np.uint8).astype(bool), int(st.rays_occluded)


@pytest.mark.parametrize("pl", ["mid", "far", "big", "tiny"])
@pytest.mark.parametrize("name", ["config5", "torture/pokeball_csg"])
def test_shading(gpu, name, pl):
    c = placed_case(gpu, name, pl)
    r = _shade_ref(gpu, name, pl)
    what = f"{name} {pl}"
    # the oracle's hits shaded: test_gpu_shade's bar, exact rays_occluded
    got = S.shade(gpu, r)
    S.check(gpu, r, got, what + " shade", step=c.step)
    assert got.tobytes() == S.shade(gpu, r, flags=gpu.RT_FLAG_NO_CULL).tobytes()
    assert r.hit.sum() >= len(r) // 4
    # the deferred pipeline on the device: its own hits, the same colours
    rgb, mask, n_occ = _pipeline(gpu, r)
    bad = np.flatnonzero(mask != r.hit)
    with np.errstate(invalid="ignore"):
        diff = np.abs(rgb - r.rgb).max(axis=1)
        bad = np.union1d(bad, np.flatnonzero(~(diff <= TOL)))
    left_out = [int(k) for k in bad if r.hit[k] and S.oracle_unstable(gpu, r, k, r.wo, r.rgb[k], r.no[k], c.step)]
    wrong = sorted(set(bad.tolist()) - set(left_out))
    keep = np.ones(len(r), dtype=bool)
    keep[left_out] = False
    print(f"  {what} intersect -> shade on the device: {int(mask.sum())} of {len(r)} hit, max|d|="
          f"{float(diff[keep].max(initial=0.0)):.3g}, left out {len(left_out)}, occluded {n_occ} (oracle {int(r.no.sum())})")
    assert not wrong, (what, wrong[:8])
    assert len(left_out) <= int(r.hit.sum()) // 100
    if not left_out:
        assert n_occ == int(r.no.sum())
    rgb_nc, mask_nc, occ_nc = _pipeline(gpu, r, gpu.RT_FLAG_NO_CULL)
    assert rgb.tobytes() == rgb_nc.tobytes() and np.array_equal(mask, mask_nc) and n_occ == occ_nc
    # the unplaced scene's lights placed by the same map, given to the call: the placed scene's own
    d0 = c.base.scene.desc
    mapped = [((c.scale * np.array(list(d0.lights[i].pos)) + np.array(c.offset)).tolist(),
               (c.scale * c.scale * np.array(list(d0.lights[i].intensity))).tolist()) for i in range(d0.n_lights)]
    assert d0.n_lights > 0 and S.shade(gpu, r, lights=mapped).tobytes() == got.tobytes()


# ---------------------------------- far origins and odd ranges on unplaced scenes
def _far_groups(rt, c, seed):
    """name -> (closest-hit rays, occlusion rays) of one unplaced case."""
    rng = np.random.default_rng(seed)
    hit = np.flatnonzero(c.cam_hit)
    pick = hit[rng.integers(0, len(hit), 256)]
    p, n = c.cam_rec["p"][pick], c.cam_rec["n"][pick]
    target = p + rng.normal(0.0, 0.05, (256, 3))
    u = rng.normal(size=(256, 3))
    u /= np.sqrt((u * u).sum(axis=1))[:, None]
    out = {}
    for tag, dist in (("origins 1e4 away", 1e4), ("origins 1e7 away", 1e7)):
        o = target + dist * u
        rays = rt.make_rays(o, target - o, 1e-4, INF)
        out[tag] = (rays, rays)
    so = p + 1e-3 * n
    sd = (so + 1e7 * u) - so
    length = np.sqrt((sd * sd).sum(axis=1))
    for tag, tmax in (("segments 1e7 long", length), ("tmax 1e30", 1e30), ("tmax 1e39", 1e39), ("tmax inf", INF)):
        rays = rt.make_rays(so, sd, 1e-4, tmax)
        out[tag] = (rays, rays)
    for tag, tmin, tmax in (("tmin -5", -5.0, None), ("tmin 0", 0.0, None), ("tmax 0", None, 0.0),
                            ("tmin > tmax", 3.0, 1.0)):
        pair = []
        for base in (c.rays, c.seg_rays):
            rays = base.copy()
            if tmin is not None:
                rays["tmin"] = tmin
            if tmax is not None:
                rays["tmax"] = tmax
            pair.append(rays)
        out[tag] = tuple(pair)
    return out


@pytest.mark.parametrize("name", ["config5", "torture/halfspace_in_csg", "bvh/ties"])
def test_far_origins_and_odd_ranges(gpu, name):
    """Each group once as a batch of its own and once interleaved with the
    case's ordinary rays: a far or empty-range lane changes nothing for its
    wave-mates, nor they for it."""
    c = case(gpu, name)
    plain_hits, plain_occ = q_isect(gpu, c.scene, c.rays), q_occl(gpu, c.scene, c.seg_rays)
    n_hit = {}
    for tag, (rays, segs) in _far_groups(gpu, c, 31337 + len(name)).items():
        what = f"{name} {tag}"
        ref_hit, ref_rec = c.oracle_intersect(rays)
        n_hit[tag] = int(ref_hit.sum())
        got = q_isect(gpu, c.scene, rays)
        check_hits(c, rays, got, ref_hit, ref_rec, what, scale=1.0)
        occ = q_occl(gpu, c.scene, segs)
        check_occluded(c, segs, occ, c.oracle_occluded(segs), what + " occluded")
        assert _same_hits(got, q_isect(gpu, c.scene, rays, flags=gpu.RT_FLAG_NO_CULL)), what
        assert np.array_equal(occ, q_occl(gpu, c.scene, segs, flags=gpu.RT_FLAG_NO_CULL)), what
        # interleaved with ordinary rays, lane by lane
        m = min(len(rays), len(c.rays))
        mix, mix_seg = np.empty(2 * m, dtype=rays.dtype), np.empty(2 * m, dtype=rays.dtype)
        mix[0::2], mix[1::2] = rays[:m], c.rays[:m]
        mix_seg[0::2], mix_seg[1::2] = segs[:m], c.seg_rays[:m]
        both = q_isect(gpu, c.scene, mix)
        assert both.records[0::2].tobytes() == got.records[:m].tobytes(), what
        assert both.records[1::2].tobytes() == plain_hits.records[:m].tobytes(), what
        assert np.array_equal(both.hit[0::2], got.hit[:m]) and np.array_equal(both.hit[1::2], plain_hits.hit[:m])
        both_occ = q_occl(gpu, c.scene, mix_seg)
        assert np.array_equal(both_occ[0::2], occ[:m]) and np.array_equal(both_occ[1::2], plain_occ[:m]), what
    # (the groups do what their names say)
    assert n_hit["origins 1e4 away"] >= 64 and n_hit["origins 1e7 away"] >= 64
    assert n_hit["tmax 0"] == 0 and n_hit["tmin > tmax"] == 0 and n_hit["tmin 0"] >= len(c.rays) // 4


# --------------------------- a clamped light distance in a scene of ordinary size
def _behind_light_scene(layout, shadow=True):
    """A light 0.05 above a floor and a small sphere 0.04 beyond it.  Within 0.1
    of a light the reference clamps the distance to 0.1 (shading.cpp:81-84) and
    its shadow ray runs that far along the normalised direction: past the
    light, into the sphere behind it.  The shadow culls once measured that
    segment along the unnormalised direction (to_light / 0.1), where it ends
    at the light; every placement of scale <= 0.01 is this case throughout.
    Layouts as scenes.shading_layout: few (no wave culls), wave (the capsule),
    bvh (the light-centred hull)."""
    objs = [scenes._floor(-1.0)]
    if shadow:
        objs.append(scenes._sph([0.0, -0.91, -1.0], 0.02, scenes._mat([0.9, 0.2, 0.2])))
    objs.append(scenes._sph([1.5, 0.0, -2.0], 0.5, scenes._mat([0.2, 0.5, 0.8])))
    if layout != "few":
        objs += [scenes._sph([-1.5 + 0.7 * i, 0.5, -3.0], 0.3, scenes._mat([0.3, 0.8, 0.3])) for i in range(4)]
    if layout == "bvh":
        objs += [scenes._sph([-2.4 + 0.3 * (k % 17), 1.5 + 0.2 * (k // 17), -4.0], 0.05, scenes._mat([0.5, 0.5, 0.5]))
                 for k in range(17 * 16)]
    lights = [{"position": [0.0, -0.95, -1.0], "intensity": [0.02, 0.02, 0.015]},
              {"position": [3, 5, 4], "intensity": [12, 12, 12]}]
    return scenes._base(objs, recursion=1, dpi=24, lights=lights)


@pytest.mark.parametrize("layout", ["few", "wave", "bvh"])
def test_occluder_behind_a_near_light(gpu, layout):
    sc = load(gpu, _behind_light_scene(layout))
    # a 32 x 32 bundle straight down onto the floor within 0.08 of the light's foot
    g = (np.arange(32) + 0.5) / 32 * 0.16 - 0.08
    x, z = np.meshgrid(g, g - 1.0)
    o = np.stack([x.ravel(), np.full(1024, 2.0), z.ravel()], axis=1)
    d = np.tile(np.array([0.0, -1.0, 0.0]), (1024, 1))
    r = R.Ref(gpu, sc, o, d)
    _radiance(gpu, r, f"occluder behind a near light, {layout}", 1e-7)
    # (the sphere behind the light does shadow floor points under it)
    bare, _, _ = gpu.oracle_trace(load(gpu, _behind_light_scene(layout, shadow=False)), r.o, r.d)
    floor = np.hypot(r.o[:, 0], r.o[:, 2] + 1.0) > 0.03
    darker = floor & ((bare - r.rgb).max(axis=1) > 100 * TOL)
    print(f"  {layout}: {int(darker.sum())} floor points lose the near light to the sphere behind it")
    assert darker.sum() >= 16
    # a 48 x 24 frame of the same patch: the trace kernels' shadow queries, one cull variant per layout
    wv = {"few": "0", "wave": "1", "bvh": "2"}[layout]
    frames = []
    for shadow in (True, False):
        win = scenes._window(_behind_light_scene(layout, shadow), [[0.0, -1.0, -1.0]], (0.2, 0.1), 240)
        fsc = load(gpu, win)
        ref, ost = gpu.oracle_render(fsc, fsc.width, fsc.height, 0, threads=8)
        frames.append(ref)
        if not shadow:
            continue
        fb, counts, rows = _render(gpu, fsc, 0, log=True)
        err = float(np.abs(fb - ref).max())
        print(f"  {layout} frame: {fsc.width}x{fsc.height} max|d|={err:.3g} rays {counts} rows {rows}")
        assert len(rows) == 1 and rows[0].split("<")[1].split(",")[1].strip() == wv
        assert err <= TOL and counts == (ost.rays_intersect, ost.rays_occluded)
        nc, nc_counts, _ = _render(gpu, load(gpu, win), 0, gpu.RT_FLAG_NO_CULL)
        assert np.array_equal(fb, nc) and nc_counts == counts
    assert (np.abs(frames[0] - frames[1]).max(axis=2) > 100 * TOL).sum() >= 16
