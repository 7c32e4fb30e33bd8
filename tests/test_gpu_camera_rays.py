"""Device-side camera rays and sample resolve (rt_camera_rays[_device],
rt_resolve_samples_device) against the CPU oracle (oracle_camera_ray,
oracle_jitter, oracle_render, oracle_primary_hits) and numpy.

Bar for rays: BIT EQUALITY with the oracle, for o, d, tmin and tmax.  The
device code is built without FP contraction and with IEEE sqrt / div (norm3 is
held bit-equal to sqrt and `/` by tests/test_gpu_norm3.py), the oracle for
x86-64 without FMA, so both sides make the same roundings in the same order,
the double normalisation of Ray{eye, d} included; a differing bit is a defect
of gen_ray / gen_ray_subpixel, which the frames share.  Nothing is left out of
any comparison.  Bar for composed frames: max|d| <= 1e-5 against oracle_render
and rt_render, the project's parity bar, with the oracle frame's ray counts
exactly.  That the oracle's own rays traced and averaged are the oracle's
frame is held on the CPU by tests/test_radiance_plan.py (see
tests/test_camera_rays_plan.py)."""
import ctypes as C

import numpy as np
import pytest

import scenes
from test_camera_rays_plan import numpy_resolve, resolve_input, same_bits
from test_gpu_query import TOL, case, check_hits
from test_gpu_radiance import _frame_scene

pytestmark = pytest.mark.gpu

_dp = C.POINTER(C.c_double)
EYE, SCREEN_P = (0.3, -0.2, 4.0), (-1.1, -0.7, 1.0)
_base = {}


def make_camera(rt, nx, ny, dpi=16):
    """The test's own camera with an nx x ny screen."""
    cam = rt.Camera()
    cam.eye[:] = EYE
    cam.P[:] = SCREEN_P
    cam.Lx, cam.Ly, cam.dpi = nx / dpi, ny / dpi, dpi
    lib = rt.host_lib()
    assert (lib.rt_camera_width(C.byref(cam)), lib.rt_camera_height(C.byref(cam))) == (nx, ny)
    return cam


def desc_of(rt, cam):
    """A scene descriptor for the oracle whose camera is `cam` (the oracle's
    camera functions read nothing else)."""
    if "sc" not in _base:
        _base["sc"] = rt.load_scene_from_json_text(scenes.config_json(3, dpi=24)[0])
    d = rt.SceneDesc.from_buffer_copy(_base["sc"].desc)
    d.camera = cam
    return d


def _rays(rt, shape):
    r = np.zeros(shape, dtype=rt.RAY_DTYPE)
    r["tmin"], r["tmax"] = 1e-4, np.inf
    return r


def oracle_centre(rt, cam, W, H, rows=None):
    """Camera::generate_ray(x, row) of every pixel of `rows` through the oracle."""
    lib, d = rt.oracle_lib(), desc_of(rt, cam)
    rows = list(range(H)) if rows is None else list(rows)
    out = _rays(rt, (len(rows), W))
    o3, d3 = (C.c_double * 3)(), (C.c_double * 3)()
    for ri, r in enumerate(rows):
        for x in range(W):
            lib.oracle_camera_ray(C.byref(d), x, r, 0.0, 0.0, 0, o3, d3)
            out["o"][ri, x], out["d"][ri, x] = tuple(o3), tuple(d3)
    return out


def oracle_jittered(rt, cam, W, H, rows=None):
    """generate_ray_subpixel(x, y, dx, dy) at loop row y = H-1-r, sample s of
    pixel (x, y) taking draws 2*((y*W + x)*8 + s) and + 1 (tracer.cpp:284-297)."""
    lib, d = rt.oracle_lib(), desc_of(rt, cam)
    rows = list(range(H)) if rows is None else list(rows)
    y_top = max(H - 1 - r for r in rows)
    jit = np.zeros(16 * W * (y_top + 1))
    lib.oracle_jitter(0, len(jit), jit.ctypes.data_as(_dp))
    jit = jit.reshape(y_top + 1, W, 8, 2)
    out = _rays(rt, (len(rows), W, 8))
    o3, d3 = (C.c_double * 3)(), (C.c_double * 3)()
    for ri, r in enumerate(rows):
        y = H - 1 - r
        for x in range(W):
            for s in range(8):
                lib.oracle_camera_ray(C.byref(d), x, y, jit[y, x, s, 0], jit[y, x, s, 1], 1, o3, d3)
                out["o"][ri, x, s], out["d"][ri, x, s] = tuple(o3), tuple(d3)
    return out


def assert_same_rays(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.tobytes() != want.tobytes():
        g, w = got.reshape(-1), want.reshape(-1)
        k = next(i for i in range(len(g)) if g[i].tobytes() != w[i].tobytes())
        raise AssertionError(f"{what}: ray {k} of {len(g)} differs: {g[k]} != {w[k]}")
    print(f"  {what}: {got.size} rays bit-equal to the oracle")


def scene_camera(rt, sc):
    return rt.Camera.from_buffer_copy(sc.desc.camera)


# ------------------------------------------------------------ 1. centre rays
@pytest.mark.parametrize("nx,ny", [(1, 1), (63, 3), (64, 3), (65, 3), (129, 2)])
def test_centre_rays(gpu, nx, ny):
    cam = make_camera(gpu, nx, ny)
    st = gpu.Stats()
    got = gpu.camera_rays(cam, nx, ny, gpu.RT_RAYS_CENTRE, stats=st)
    assert_same_rays(got, oracle_centre(gpu, cam, nx, ny), f"centre {nx}x{ny}")
    assert (st.pixels, st.rays_intersect, st.rays_occluded, st.rays_traced, st.n_gpus) == (nx * ny, 0, 0, 0, 1)
    assert st.ms_kernel > 0.0 and st.ms_total >= st.ms_kernel
    # a frame larger than the camera's screen: camera.h:47-49 outside nx x ny
    W, H = nx + 2, ny + 1
    got = gpu.camera_rays(cam, W, H, gpu.RT_RAYS_CENTRE)
    assert_same_rays(got, oracle_centre(gpu, cam, W, H), f"centre {nx}x{ny} camera, {W}x{H} frame")
    outside = np.ones((H, W), dtype=bool)
    outside[:ny, :nx] = False
    assert np.array_equal(got["o"][outside], np.tile(np.array(EYE), (int(outside.sum()), 1)))
    assert got["d"][outside].tobytes() == np.tile(np.array([0.0, 0.0, -1.0]), (int(outside.sum()), 1)).tobytes()
    assert not np.any(np.all(got["d"][~outside] == np.array([0.0, 0.0, -1.0]), axis=-1))


@pytest.mark.parametrize("name", ["config2", "config3", "config4", "config5", "placed"])
def test_centre_rays_of_scene_cameras(gpu, name):
    if name == "placed":
        import json
        text = json.dumps(scenes.placed(scenes.with_dpi(scenes.cfg4_scene(), 24), 1e-3, [1e6, 1e6, 1e6]))
    else:
        text = scenes.config_json(int(name[6:]), dpi=24)[0]
    sc = gpu.load_scene_from_json_text(text)
    W, H = sc.width, sc.height
    got = gpu.camera_rays(sc, W, H, gpu.RT_RAYS_CENTRE)
    assert_same_rays(got, oracle_centre(gpu, scene_camera(gpu, sc), W, H), f"centre {name} {W}x{H}")


# ---------------------------------------------------------- 2. jittered rays
def test_jittered_rays_whole_frame_config3(gpu):
    sc = gpu.load_scene_from_json_text(scenes.config_json(3, dpi=24)[0])
    W, H = sc.width, sc.height
    st = gpu.Stats()
    got = gpu.camera_rays(sc, W, H, gpu.RT_RAYS_JITTERED, stats=st)
    assert_same_rays(got, oracle_jittered(gpu, scene_camera(gpu, sc), W, H), f"jittered config3 {W}x{H}")
    assert (st.pixels, st.rays_traced, st.n_gpus) == (W * H, 0, 1) and st.ms_kernel > 0.0
    # ... which are the rays the existing host-fed frame test builds (frame order)
    o, d = gpu.oracle_frame_rays(sc)
    assert got["o"].tobytes() == o.tobytes() and got["d"].tobytes() == d.tobytes()


@pytest.mark.parametrize("nx,ny", [(1, 1), (65, 3)])
def test_jittered_rays_small_cameras(gpu, nx, ny):
    cam = make_camera(gpu, nx, ny)
    got = gpu.camera_rays(cam, nx, ny, gpu.RT_RAYS_JITTERED)
    assert_same_rays(got, oracle_jittered(gpu, cam, nx, ny), f"jittered {nx}x{ny}")


def test_jittered_rays_across_a_checkpoint_segment(gpu):
    """256 x 160, output rows 2, 3, 4: loop row 156 (output row 3) starts at
    pixel 39,936, whose first draw is number 638,976 of the stream, i.e. stream
    word 1,277,952 = 128 x (16 twist blocks of 624 words): the first pixel
    whose draws begin exactly on a segment boundary of the checkpoint table, in
    the middle of a request that starts and ends inside other segments."""
    W, H, rows = 256, 160, [2, 3, 4]
    assert 156 * W == 39936 and 39936 * 16 == 638976 and 638976 * 2 == 128 * 16 * 624
    cam = make_camera(gpu, W, H)
    got = gpu.camera_rays(cam, W, H, gpu.RT_RAYS_JITTERED, rows=rows)
    assert_same_rays(got, oracle_jittered(gpu, cam, W, H, rows), f"jittered {W}x{H} rows {rows}")


# ------------------------------------------------------------- 3. row lists
@pytest.mark.parametrize("kind", [0, 1], ids=["centre", "jittered"])
def test_row_lists(gpu, kind):
    W, H = 65, 40
    cam = make_camera(gpu, W, H)
    full = gpu.camera_rays(cam, W, H, kind)
    want = oracle_jittered(gpu, cam, W, H) if kind else oracle_centre(gpu, cam, W, H)
    assert_same_rays(full, want, f"65x40 kind {kind}, all rows")
    lists = {"single": [17], "reversed": list(range(H - 1, -1, -1)), "strips": gpu.dist_rows(H, 3, 1)}
    assert len(lists["strips"]) >= 8 and len(lists["strips"]) % 8 == 0
    for what, rows in lists.items():
        st = gpu.Stats()
        got = gpu.camera_rays(cam, W, H, kind, rows=rows, stats=st)
        assert got.tobytes() == full[rows].tobytes(), (what, rows)
        assert st.pixels == len(rows) * W
        print(f"  rows {what}: {got.size} rays bit-equal to those rows of the full frame")
    # an explicit 0..H-1 list is the NULL list
    assert gpu.camera_rays(cam, W, H, kind, rows=list(range(H))).tobytes() == full.tobytes()


# ---------------------------------------------------------- 4. buffer bounds
def _dev_rays(rt, cam, W, H, kind, rows, cap, stream=None, stats=None):
    """rt_camera_rays_device into a buffer of cap rays filled with 0xAB; (bytes, n)."""
    d_rays = rt.DeviceBuffer(cap * 64)
    d_rays.from_host(np.full(cap * 64, 0xAB, dtype=np.uint8))
    n = rt.camera_rays_device(cam, W, H, kind, rows, d_rays, stream, stats)
    return d_rays.to_host(np.uint8), n


@pytest.mark.parametrize("kind", [0, 1], ids=["centre", "jittered"])
@pytest.mark.parametrize("nx,ny", [(1, 1), (65, 3)])
def test_nothing_is_written_past_the_rays(gpu, nx, ny, kind):
    cam = make_camera(gpu, nx, ny)
    n = nx * ny * (8 if kind else 1)
    raw, n_got = _dev_rays(gpu, cam, nx, ny, kind, None, n + 70)
    assert n_got == n
    want = oracle_jittered(gpu, cam, nx, ny) if kind else oracle_centre(gpu, cam, nx, ny)
    assert raw[:n * 64].tobytes() == want.tobytes()
    assert np.all(raw[n * 64:] == 0xAB)
    print(f"  {nx}x{ny} kind {kind}: {n} rays bit-equal, {70 * 64} guard bytes untouched")
    with pytest.raises(ValueError):
        gpu.camera_rays_device(cam, nx, ny, kind, None, gpu.DeviceBuffer(max(1, n * 64 - 1)))


# ------------------------------------------------- 5. host form = device form
@pytest.mark.parametrize("kind", [0, 1], ids=["centre", "jittered"])
def test_host_form_is_the_device_form(gpu, kind):
    sc = gpu.load_scene_from_json_text(scenes.config_json(4, dpi=24)[0])
    W, H = sc.width, sc.height
    per_row = W * (8 if kind else 1)
    stream = gpu.Stream()
    try:
        raw, n = _dev_rays(gpu, sc, W, H, kind, None, per_row * H, stream=stream)
    finally:
        stream.destroy()
    host = gpu.camera_rays(sc, W, H, kind)
    assert n == host.size and raw.tobytes() == host.tobytes()
    want = oracle_jittered(gpu, scene_camera(gpu, sc), W, H) if kind else oracle_centre(gpu, scene_camera(gpu, sc), W, H)
    assert_same_rays(host, want, f"config4 {W}x{H} kind {kind}, host form")
    # the staging chunk forced small: whole rows, at least 3 chunks
    rows_per_chunk = H // 3 - 1
    assert rows_per_chunk >= 1 and -(-H // rows_per_chunk) >= 3
    gpu.camera_chunk_rays(rows_per_chunk * per_row + per_row // 2)
    try:
        chunked = gpu.camera_rays(sc, W, H, kind)
        gpu.camera_chunk_rays(1)   # (less than a row: one row per chunk)
        by_row = gpu.camera_rays(sc, W, H, kind, rows=list(range(H - 1, -1, -1)))
    finally:
        gpu.camera_chunk_rays(0)
    assert chunked.tobytes() == host.tobytes()
    assert by_row.tobytes() == host[::-1].tobytes()


# ------------------------------------------------ 6. the jitter cache is shared
def test_the_jitter_cache_is_shared_with_the_frames(gpu):
    sc = gpu.load_scene_from_json_text(scenes.config_json(4, dpi=24)[0])
    W, H = sc.width, sc.height
    request = H * W * 16 * 8   # bytes of the frame's draws
    try:
        gpu.jitter_cache_budget(-1)   # (empties the cache and zeroes the counts)
        resident = gpu.camera_rays(sc, W, H, gpu.RT_RAYS_JITTERED)
        a = gpu.jitter_cache_stats()
        assert (a["hits"], a["misses"], a["entries"]) == (0, 1, 1) and a["bytes"] >= request
        fb = gpu.Tracer(sc, W, H, 0).render()
        b = gpu.jitter_cache_stats()
        assert (b["hits"], b["misses"], b["entries"]) == (a["hits"] + 1, a["misses"], 1)
        again = gpu.camera_rays(sc, W, H, gpu.RT_RAYS_JITTERED)
        c = gpu.jitter_cache_stats()
        assert (c["hits"], c["misses"]) == (b["hits"] + 1, b["misses"]) and again.tobytes() == resident.tobytes()
        # the reverse order: the frame fills, the rays find the draws resident
        gpu.jitter_cache_budget(-1)
        fb2 = gpu.Tracer(sc, W, H, 0).render()
        a = gpu.jitter_cache_stats()
        assert (a["hits"], a["misses"], a["entries"]) == (0, 1, 1)
        st = gpu.Stats()
        rays = gpu.camera_rays(sc, W, H, gpu.RT_RAYS_JITTERED, stats=st)
        b = gpu.jitter_cache_stats()
        assert (b["hits"], b["misses"], b["entries"]) == (1, 1, 1)
        assert rays.tobytes() == resident.tobytes() and np.array_equal(fb, fb2)
        print(f"  resident draws: ms_rng {st.ms_rng:.4f}")
        # no cache, and a budget smaller than the request: a transient buffer, the same rays
        for budget in (0, request // 2):
            gpu.jitter_cache_budget(budget)
            for _ in range(2):
                rays = gpu.camera_rays(sc, W, H, gpu.RT_RAYS_JITTERED)
                assert rays.tobytes() == resident.tobytes(), budget
            s = gpu.jitter_cache_stats()
            assert (s["entries"], s["bytes"], s["hits"], s["misses"]) == (0, 0, 0, 2), (budget, s)
            assert np.array_equal(gpu.Tracer(sc, W, H, 0).render(), fb)
    finally:
        gpu.jitter_cache_budget(-1)
    assert_same_rays(resident, oracle_jittered(gpu, scene_camera(gpu, sc), W, H), f"jittered config4 {W}x{H}")


# ---------------------------------------------------------- 7. device resolve
@pytest.mark.parametrize("n_pixels", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("spp", [1, 3, 8, 64])
def test_device_resolve_is_the_numpy_loop(gpu, spp, n_pixels):
    rgb = resolve_input(n_pixels, spp, 77 * spp + n_pixels)
    want = numpy_resolve(rgb, spp)
    d_rgb = gpu.DeviceBuffer(rgb.nbytes)
    d_rgb.from_host(rgb)
    cap = n_pixels + 33
    d_fb = gpu.DeviceBuffer(cap * 24)
    d_fb.from_host(np.full(cap * 24, 0xAB, dtype=np.uint8))
    gpu.resolve_samples_device(d_rgb, n_pixels, spp, d_fb)
    raw = d_fb.to_host(np.uint8)
    got = raw[:n_pixels * 24].view(np.float64).reshape(n_pixels, 3)
    assert same_bits(got, want)
    assert np.all(raw[n_pixels * 24:] == 0xAB)
    assert same_bits(got, gpu.resolve_samples(rgb, spp))


# ------------------------------------------- 8. the frame, composed on the device
def compose(rt, sc, cam, W, H, rows=None, stats=None):
    """camera_rays_device (jittered) -> query_radiance_device ->
    resolve_samples_device with no host copy between the steps, then one D2H."""
    n_rows = H if rows is None else len(rows)
    n = n_rows * W * 8
    d_rays, d_rgb, d_fb = rt.DeviceBuffer(n * 64), rt.DeviceBuffer(n * 24), rt.DeviceBuffer(n_rows * W * 24)
    assert rt.camera_rays_device(cam, W, H, rt.RT_RAYS_JITTERED, rows, d_rays) == n
    rt.query_radiance_device(sc, d_rays, n, d_rgb, stats=stats)
    rt.resolve_samples_device(d_rgb, n_rows * W, 8, d_fb)
    return d_fb.to_host(shape=(n_rows, W, 3))


@pytest.mark.parametrize("name", ["config3", "config4", "config5", "deep/mirrors_rec24", "dir/pokeball_csg_sun"])
def test_frame_composed_on_the_device(gpu, name):
    sc = _frame_scene(gpu, name)
    W, H = sc.width, sc.height
    st = gpu.Stats()
    fb = compose(gpu, sc, sc, W, H, stats=st)
    ref, ost = gpu.oracle_render(sc, W, H, 0, threads=8)
    fst = gpu.Stats()
    frame = gpu.Tracer(sc, W, H, 0).render(fst)
    e_or, e_fb = float(np.abs(fb - ref).max()), float(np.abs(fb - frame).max())
    print(f"  {name}: {W}x{H}, {8 * W * H} rays, max|d| oracle {e_or:.3g}, rt_render {e_fb:.3g}, "
          f"bit-identical to rt_render: {fb.tobytes() == frame.tobytes()}")
    assert e_or <= TOL and e_fb <= TOL
    assert (st.rays_intersect, st.rays_occluded) == (ost.rays_intersect, ost.rays_occluded)
    if name == "config4":
        rows = [5, 0, 9]
        part = compose(gpu, sc, sc, W, H, rows=rows)
        e = float(np.abs(part - frame[rows]).max())
        print(f"  {name} rows {rows}: max|d| rt_render {e:.3g}, bit-identical: {part.tobytes() == frame[rows].tobytes()}")
        assert e <= TOL and float(np.abs(part - ref[rows]).max()) <= TOL


# ------------------------------------------------- 9. another camera, same scene
def test_another_camera_on_the_resident_scene(gpu):
    lib = gpu.amd_lib()
    sc = gpu.load_scene_from_json_text(scenes.config_json(4, dpi=24)[0])
    gpu.Tracer(sc, sc.width, sc.height, 0).render()   # (the scene is resident from here on)
    cam = scene_camera(gpu, sc)
    cam.eye[0] += 0.4
    cam.eye[1] += 0.1
    cam.dpi = 16
    W, H = lib.rt_camera_width(C.byref(cam)), lib.rt_camera_height(C.byref(cam))
    assert (W, H) != (sc.width, sc.height)
    t = (C.c_double * 4)()

    def scene_ms():
        assert lib.rt_setup_times(t, 4) == 0
        return t[0]

    ms0 = scene_ms()
    st = gpu.Stats()
    fb = compose(gpu, sc, cam, W, H, stats=st)
    assert scene_ms() == ms0   # no scene was compiled or uploaded for the second camera
    desc = gpu.SceneDesc.from_buffer_copy(sc.desc)   # (shares the scene's arrays: `sc` stays alive)
    desc.camera = cam
    ref, ost = np.zeros((H, W, 3)), gpu.OracleStats()
    assert gpu.oracle_lib().oracle_render_rows(C.byref(desc), W, H, 0, 0, H, ref.ctypes.data_as(_dp), C.byref(ost), 8) == 0
    err = float(np.abs(fb - ref).max())
    print(f"  config4 from a moved eye at dpi 16: {W}x{H}, max|d| oracle {err:.3g}")
    assert err <= TOL
    assert (st.rays_intersect, st.rays_occluded) == (ost.rays_intersect, ost.rays_occluded)


# --------------------------------------------------------------- 10. G-buffer
class _NothingLeftOut:
    """check_hits' instability probe answering "stable": every difference counts."""
    @staticmethod
    def oracle_unstable(ray, occluded, step=1e-7):
        return False


def test_gbuffer_from_device_rays(gpu):
    lib = gpu.amd_lib()
    sc = case(gpu, "config5").scene
    W, H = sc.width, sc.height
    n = W * H
    d_rays, d_hits, d_mask = gpu.DeviceBuffer(n * 64), gpu.DeviceBuffer(n * 64), gpu.DeviceBuffer(n)
    assert gpu.camera_rays_device(sc, W, H, gpu.RT_RAYS_CENTRE, None, d_rays) == n
    st = gpu.Stats()
    assert lib.rt_query_intersect_device(sc.handle, d_rays.ptr, n, 0, d_hits.ptr, d_mask.ptr, None, C.byref(st)) == 0
    got = gpu.QueryHits(d_hits.to_host(np.uint8).view(gpu.HIT_DTYPE), d_mask.to_host(np.uint8).astype(bool))
    rays = d_rays.to_host(np.uint8).view(gpu.RAY_DTYPE)
    ref = gpu.oracle_primary_hits(sc)
    assert rays["d"].tobytes() == ref["d"].tobytes() and st.rays_intersect == n
    assert np.array_equal(got.hit, ref["hit"])
    hit = ref["hit"]
    assert np.array_equal(got.mat[hit], ref["mat"][hit]) and np.array_equal(got.front_face[hit], ref["front_face"][hit])
    check_hits(_NothingLeftOut, rays, got, ref["hit"], ref, f"G-buffer config5 {W}x{H}")
    assert hit.sum() > n // 4


# -------------------------------------------------------------- 11. launch log
def test_launch_log(gpu):
    cam = make_camera(gpu, 65, 3)
    try:
        gpu.jitter_cache_budget(-1)   # (a cold cache)
        gpu.launch_log(True)
        gpu.camera_rays(cam, 65, 3, gpu.RT_RAYS_CENTRE)
        assert gpu.launch_log_get() == ["rtd::k_camera_rays<false>"]
        gpu.launch_log(True)
        gpu.camera_rays(cam, 65, 3, gpu.RT_RAYS_JITTERED)
        log = gpu.launch_log_get()
        print(f"  cold jittered call launched {log}")
        assert len(log) >= 2 and log[-1] == "rtd::k_camera_rays<true>"
        assert all("k_mt_fill" in k for k in log[:-1])
        gpu.launch_log(True)
        gpu.camera_rays(cam, 65, 3, gpu.RT_RAYS_JITTERED)   # resident draws: no fill
        assert gpu.launch_log_get() == ["rtd::k_camera_rays<true>"]
        d_rgb, d_fb = gpu.DeviceBuffer(65 * 8 * 24), gpu.DeviceBuffer(65 * 24)
        gpu.launch_log(True)
        gpu.resolve_samples_device(d_rgb, 65, 8, d_fb)
        assert gpu.launch_log_get() == ["rtd::k_resolve_samples"]
        gpu.launch_log(True)
        gpu.camera_rays(cam, 65, 3, gpu.RT_RAYS_JITTERED, rows=[])
        gpu.resolve_samples_device(d_rgb, 0, 8, d_fb)
        assert gpu.launch_log_get() == []
    finally:
        gpu.launch_log(False)
        gpu.jitter_cache_budget(-1)
