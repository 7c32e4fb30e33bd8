"""Camera rays and sample resolve on the CPU (no device is touched): the
exported symbols and wrappers, the argument checks of rt_camera_rays[_device]
and rt_resolve_samples[_device] (all made before any device work), and the
host resolve loop of librt_host.so against the numpy statement of the frame's
sum (tracer.cpp:291-296).

The oracle's side of the composed frame - the frame's own 8 W H jittered rays
(rtamd.oracle_frame_rays) traced by oracle_trace and averaged in sample order
are oracle_render's frame, for config 3 at dpi 24 - is held by
tests/test_radiance_plan.py::test_oracle_trace_over_the_frames_rays_is_oracle_render;
tests/test_gpu_camera_rays.py relies on it and does not repeat it."""
import ctypes as C

import numpy as np
import pytest

RT_OK, RT_ERR_INVALID_ARG = 0, -1
_i32p = C.POINTER(C.c_int32)


def _cam(rt):
    cam = rt.Camera()
    cam.eye[:] = [0.3, -0.2, 4.0]
    cam.P[:] = [-1.1, -0.7, 1.0]
    cam.Lx, cam.Ly, cam.dpi = 4.0, 3.0, 4   # 16 x 12
    return cam


def _rows(v):
    return (C.c_int32 * len(v))(*v)


# ------------------------------------------------------------------ symbols
def test_symbols_and_wrappers(rt):
    amd, host = rt.amd_lib(), rt.host_lib()
    for name in ("rt_camera_rays", "rt_camera_rays_device", "rt_resolve_samples_device", "rt_resolve_samples"):
        assert hasattr(amd, name), name   # (librtamd.so links librt_host.so: its symbols resolve through it)
    assert hasattr(host, "rt_resolve_samples")
    for name in ("camera_rays", "camera_rays_device", "resolve_samples", "resolve_samples_device", "Camera"):
        assert callable(getattr(rt, name)), name
    assert (rt.RT_RAYS_CENTRE, rt.RT_RAYS_JITTERED, rt.RT_SPP) == (0, 1, 8)
    assert amd.rt_abi_version() == 6


# ---------------------------------------------------------- argument checks
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_argument_checks_come_before_any_device_work(rt, device):
    lib = rt.amd_lib()
    cam = _cam(rt)
    W, H = 16, 12
    out = np.zeros(W * H * 8, dtype=rt.RAY_DTYPE)
    op = out.ctypes.data_as(C.c_void_p)
    fname = "rt_camera_rays_device" if device else "rt_camera_rays"

    def call(cam_p, W, H, kind, rows, n_rows, outp):
        if device:
            return lib.rt_camera_rays_device(cam_p, W, H, kind, rows, n_rows, outp, None, None)
        return lib.rt_camera_rays(cam_p, W, H, kind, rows, n_rows, outp, None)

    cp = C.byref(cam)
    bad = {
        "NULL cam": (None, W, H, 0, None, H, op),
        "W = 0": (cp, 0, H, 0, None, H, op),
        "H = -1": (cp, W, -1, 0, None, 0, op),
        "kind = 2": (cp, W, H, 2, None, H, op),
        "a duplicate row": (cp, W, H, 1, _rows([3, 5, 3]), 3, op),
        "a row equal to H": (cp, W, H, 0, _rows([0, H]), 2, op),
        "a negative row": (cp, W, H, 0, _rows([-1]), 1, op),
        "NULL rows with n_rows != H": (cp, W, H, 0, None, 3, op),
        "NULL output with n_rows > 0 (centre)": (cp, W, H, 0, _rows([1, 2]), 2, None),
        "NULL output with n_rows > 0 (jittered)": (cp, W, H, 1, None, H, None),
    }
    for what, args in bad.items():
        assert call(*args) == RT_ERR_INVALID_ARG, what
        msg = rt.last_error()
        assert msg.startswith(fname + ":"), (what, msg)
    # n_rows == 0 is RT_OK without a launch, whatever the output pointer; stats are zeroed
    st = rt.Stats()
    st.rays_traced = st.pixels = 77
    for kind in (0, 1):
        if device:
            assert lib.rt_camera_rays_device(cp, W, H, kind, None, 0, None, None, C.byref(st)) == RT_OK
        else:
            assert lib.rt_camera_rays(cp, W, H, kind, _rows([]), 0, None, C.byref(st)) == RT_OK
        assert (st.rays_traced, st.pixels, st.rays_intersect, st.rays_occluded, st.n_gpus) == (0, 0, 0, 0, 1)
    assert not out.view(np.uint8).any()
    # the wrappers refuse what the library would: a buffer too small, a bad camera argument
    with pytest.raises(TypeError):
        rt.camera_rays(None, W, H, 0)
    assert rt.camera_rays(cam, W, H, rt.RT_RAYS_JITTERED, rows=[]).shape == (0, W, 8)
    with pytest.raises(rt.RTError) as e:
        rt.camera_rays(cam, W, H, 2)
    assert e.value.code == RT_ERR_INVALID_ARG


def test_resolve_argument_checks(rt):
    amd, host = rt.amd_lib(), rt.host_lib()
    rgb, fb = np.zeros((4, 8, 3)), np.zeros((4, 3))
    rp, fp = rgb.ctypes.data_as(C.c_void_p), fb.ctypes.data_as(C.c_void_p)
    for spp in (0, 65, -3):
        assert host.rt_resolve_samples(rp, 4, spp, fp) == RT_ERR_INVALID_ARG
        assert rt.last_error().startswith("rt_resolve_samples:")
        assert amd.rt_resolve_samples_device(rp, 4, spp, fp, None) == RT_ERR_INVALID_ARG
        assert rt.last_error().startswith("rt_resolve_samples_device:")
        # (also at n_pixels == 0)
        assert host.rt_resolve_samples(None, 0, spp, None) == RT_ERR_INVALID_ARG
        assert amd.rt_resolve_samples_device(None, 0, spp, None, None) == RT_ERR_INVALID_ARG
    for args in ((None, 4, 8, fp), (rp, 4, 8, None), (rp, 4, 8, rp), (rp, 4, 8, C.c_void_p(rp.value + 24 * 8))):
        assert host.rt_resolve_samples(*args) == RT_ERR_INVALID_ARG
        assert rt.last_error().startswith("rt_resolve_samples:")
        assert amd.rt_resolve_samples_device(*args, None) == RT_ERR_INVALID_ARG
        assert rt.last_error().startswith("rt_resolve_samples_device:")
    assert host.rt_resolve_samples(None, 0, 8, None) == RT_OK
    assert amd.rt_resolve_samples_device(None, 0, 8, None, None) == RT_OK
    with pytest.raises(ValueError):
        rt.resolve_samples(np.zeros((4, 7, 3)), 8)


# ------------------------------------------------------------- host resolve
def resolve_input(n_pixels, spp, seed):
    """Seeded colours: ordinary values, large and tiny magnitudes, subnormals,
    zeros of both signs, and a few inf / -inf / nan (so that some pixels sum
    inf + -inf)."""
    rng = np.random.default_rng(seed)
    n = n_pixels * spp * 3
    v = rng.uniform(-2.0, 2.0, n) * 10.0 ** rng.integers(-12, 12, n)
    special = np.array([np.inf, -np.inf, np.nan, 5e-324, -5e-324, 2.2250738585072009e-308, 1.1e-310, 0.0, -0.0,
                        1.7976931348623157e308, -1.7976931348623157e308])
    k = rng.random(n) < 0.15
    v[k] = special[rng.integers(0, len(special), int(k.sum()))]
    return v.reshape(n_pixels, spp, 3)


def numpy_resolve(rgb, spp):
    """acc = 0; acc += rgb[:, s] for s in order; acc * (1.0 / spp)."""
    acc = np.zeros((rgb.shape[0], 3))
    with np.errstate(all="ignore"):
        for s in range(spp):
            acc += rgb[:, s]
        return acc * (1.0 / spp)


def same_bits(a, b):
    """Bit equality (signed zeros and subnormals included), NaN matching NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb)) and a[~na].tobytes() == b[~nb].tobytes()


@pytest.mark.parametrize("n_pixels", [1, 1000])
@pytest.mark.parametrize("spp", [1, 3, 8, 64])
def test_host_resolve_is_the_numpy_loop(rt, spp, n_pixels):
    rgb = resolve_input(n_pixels, spp, 1000 * spp + n_pixels)
    assert np.isnan(rgb).any() or n_pixels == 1
    want = numpy_resolve(rgb, spp)
    got = rt.resolve_samples(rgb, spp)
    assert got.shape == (n_pixels, 3)
    assert same_bits(got, want)
    if n_pixels == 1000:
        assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any()
