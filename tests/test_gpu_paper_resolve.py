"""Paper frames composed from the queries, on the device: k_paper_resolve and
k_rays_wo (rt_paper_f64.hip) held bit for bit to the host forms of
librt_host.so, which tests/test_paper_resolve_plan.py holds to the oracle and
to the numpy restatement of tracer.cpp; and the composed frame
  paper_resolve(hits, mask, query_shade(hits, rays_wo(rays), mask, miss = white)),
  (hits, mask) = query_intersect(rays), rays = camera_rays(cam, CENTRE)
with every buffer on the device, held to the oracle's paper frame and to
rt_render's with np.array_equal.

The widths are the kernel's column tile (64) and twice it, each +- 1, and 1
and 2; the heights give workgroups with one row, full row groups (8 rows)
and a ragged last one (9 = 8 + 1, 33 = 4 * 8 + 1)."""
import ctypes as C
import json

import numpy as np
import pytest

import scenes
from test_paper_resolve_plan import (band_of, band_shapes, bits, load_frame_scene, synthetic_grid, wo_ray_sets)

pytestmark = pytest.mark.gpu

PAD = 256   # guard bytes behind every output


class _At:
    """A device buffer's bytes from `offset` on, as the *_device wrappers take one."""

    def __init__(self, buf, offset):
        self.ptr, self.nbytes, self._keep = C.c_void_p(buf.ptr.value + offset), buf.nbytes - offset, buf


def _guarded(rt, nbytes):
    buf = rt.DeviceBuffer(nbytes + PAD)
    buf.from_host(np.full(nbytes + PAD, 0xAB, dtype=np.uint8))
    return buf


def _out(buf, nbytes, shape):
    raw = buf.to_host(np.uint8)
    assert np.all(raw[nbytes:] == 0xAB), "bytes behind the output were written"
    out = raw[:nbytes].view(np.float64)
    return out if shape is None else out.reshape(shape)


def device_resolve(rt, hits, mask, rgb, W, H, row0, n_rows, fb=True, edge=True, stream=None, stats=None, shift=0):
    """paper_resolve_device of host arrays holding rows paper_band(H, row0, n_rows): (fb or None, edge or None).
    shift: byte offset of the hits inside their allocation (8: records that are not 16-byte aligned)."""
    n_out = n_rows * W
    d_hits = rt.DeviceBuffer(hits.nbytes + shift)
    h = _At(d_hits, shift)
    rt.amd_lib().rt_memcpy_h2d(h.ptr, np.ascontiguousarray(hits).ctypes.data_as(C.c_void_p), hits.nbytes)
    d_mask = d_rgb = None
    if mask is not None:
        d_mask = rt.DeviceBuffer(mask.nbytes)
        d_mask.from_host(mask)
    if rgb is not None:
        d_rgb = rt.DeviceBuffer(rgb.nbytes)
        d_rgb.from_host(rgb)
    d_fb = _guarded(rt, n_out * 24) if fb else None
    d_edge = _guarded(rt, n_out * 8) if edge else None
    rt.paper_resolve_device(h, d_mask, d_rgb, W, H, row0, n_rows, d_fb, d_edge, stream=stream, stats=stats)
    return (_out(d_fb, n_out * 24, (n_rows, W, 3)) if fb else None,
            _out(d_edge, n_out * 8, (n_rows, W)) if edge else None)


# ------------------------------------------- 1. device form against host form
@pytest.mark.parametrize("W", [1, 2, 63, 64, 65, 127, 130])
def test_device_form_is_the_host_form(gpu, W):
    for H in (1, 2, 3, 9, 33):
        hits, mask, rgb = synthetic_grid(gpu, W, H, 7000 + 100 * W + H)
        want, want_edge = gpu.paper_resolve(hits, mask, rgb, W, H, want_edge=True)
        st = gpu.Stats()
        fb, edge = device_resolve(gpu, hits, mask, rgb, W, H, 0, H, stats=st)
        assert np.array_equal(bits(fb), bits(want)), (W, H, np.argwhere(bits(fb) != bits(want))[:4].tolist())
        assert np.array_equal(bits(edge), bits(want_edge)), (W, H)
        assert st.pixels == W * H and st.n_gpus == 1 and st.rays_traced == 0 and st.ms_kernel > 0 and st.ms_total > 0
        # one output at a time; rgb is not needed for the edge map alone
        only_fb, none = device_resolve(gpu, hits, mask, rgb, W, H, 0, H, edge=False)
        assert none is None and np.array_equal(bits(only_fb), bits(want))
        none, only_edge = device_resolve(gpu, hits, mask, None, W, H, 0, H, fb=False)
        assert none is None and np.array_equal(bits(only_edge), bits(want_edge))
        # NULL mask: every entry is a hit
        want0, want0_edge = gpu.paper_resolve(hits, None, rgb, W, H, want_edge=True)
        fb0, edge0 = device_resolve(gpu, hits, None, rgb, W, H, 0, H)
        assert np.array_equal(bits(fb0), bits(want0)) and np.array_equal(bits(edge0), bits(want0_edge)), (W, H)
        # bands with halos
        for row0, n_rows in band_shapes(H):
            if n_rows < 1 or row0 + n_rows > H:
                continue
            b, be = device_resolve(gpu, band_of(gpu, hits, W, H, row0, n_rows), band_of(gpu, mask, W, H, row0, n_rows),
                                   band_of(gpu, rgb, W, H, row0, n_rows, 3), W, H, row0, n_rows)
            assert np.array_equal(bits(b), bits(want[row0:row0 + n_rows])), (W, H, row0, n_rows)
            assert np.array_equal(bits(be), bits(want_edge[row0:row0 + n_rows])), (W, H, row0, n_rows)


def test_a_stream_of_the_callers_and_unaligned_records(gpu):
    W, H = 65, 33
    hits, mask, rgb = synthetic_grid(gpu, W, H, 31)
    want, want_edge = gpu.paper_resolve(hits, mask, rgb, W, H, want_edge=True)
    stream = gpu.Stream()
    try:
        gpu.launch_log(True)
        fb, edge = device_resolve(gpu, hits, mask, rgb, W, H, 0, H, stream=stream)
        assert gpu.launch_log_get() == ["rtd::k_paper_resolve<true>"]
        assert np.array_equal(bits(fb), bits(want)) and np.array_equal(bits(edge), bits(want_edge))
        gpu.launch_log(True)
        fb, edge = device_resolve(gpu, hits, mask, rgb, W, H, 0, H, stream=stream, shift=8)
        assert gpu.launch_log_get() == ["rtd::k_paper_resolve<false>"]
        assert np.array_equal(bits(fb), bits(want)) and np.array_equal(bits(edge), bits(want_edge))
    finally:
        gpu.launch_log(False)
        stream.destroy()


def test_device_argument_checks_come_before_any_launch(gpu):
    lib = gpu.amd_lib()
    W, H = 4, 5
    d_hits, d_rgb, d_fb = gpu.DeviceBuffer(64 * W * H), gpu.DeviceBuffer(24 * W * H), gpu.DeviceBuffer(24 * W * H)
    call = lambda *a: lib.rt_paper_resolve_device(*a, None, None)   # noqa: E731
    gpu.launch_log(True)
    try:
        assert call(d_hits.ptr, None, d_rgb.ptr, 0, H, 0, H, d_fb.ptr, None) == -1
        assert call(d_hits.ptr, None, d_rgb.ptr, W, H, -1, 1, d_fb.ptr, None) == -1
        assert call(d_hits.ptr, None, d_rgb.ptr, W, H, 0, -1, d_fb.ptr, None) == -1
        assert call(d_hits.ptr, None, d_rgb.ptr, W, H, 1, H, d_fb.ptr, None) == -1
        assert call(None, None, d_rgb.ptr, W, H, 0, H, d_fb.ptr, None) == -1
        assert call(d_hits.ptr, None, d_rgb.ptr, W, H, 0, H, None, None) == -1
        assert call(d_hits.ptr, None, None, W, H, 0, H, d_fb.ptr, None) == -1
        assert call(d_hits.ptr, None, d_rgb.ptr, W, H, 0, H, d_rgb.ptr, None) == -1   # fb on rgb
        assert call(d_hits.ptr, None, d_rgb.ptr, W, H, 0, H, d_fb.ptr, d_hits.ptr) == -1   # edge on hits
        assert b"rt_paper_resolve_device" in gpu.host_lib().rt_last_error()
        assert call(None, None, None, W, H, 2, 0, None, None) == 0   # n_rows == 0
        assert lib.rt_rays_wo_device(None, 0, None, None) == 0        # n == 0
        assert lib.rt_rays_wo_device(None, 3, d_fb.ptr, None) == -1
        assert lib.rt_rays_wo_device(d_hits.ptr, 3, d_hits.ptr, None) == -1
        assert gpu.launch_log_get() == []
    finally:
        gpu.launch_log(False)


# --------------------------------------------------------- 2. the composed frame
def compose(rt, sc, cam, W, H, row0=0, n_rows=None, lights=None, stream=None, times=None):
    """Rows [row0, row0 + n_rows) of the paper frame: camera_rays_device (centre)
    -> query_intersect_device -> rays_wo_device -> query_shade_device (misses
    white) -> paper_resolve_device, no host copy between the steps; (fb, edge)."""
    n_rows = H - row0 if n_rows is None else n_rows
    in0, in1 = rt.paper_band(H, row0, n_rows)
    rows = None if (in0, in1) == (0, H) else list(range(in0, in1))
    n, n_out = (in1 - in0) * W, n_rows * W
    d_rays, d_hits, d_mask = rt.DeviceBuffer(n * 64), rt.DeviceBuffer(n * 64), rt.DeviceBuffer(n)
    d_wo, d_rgb = rt.DeviceBuffer(n * 24), rt.DeviceBuffer(n * 24)
    d_fb, d_edge = rt.DeviceBuffer(n_out * 24), rt.DeviceBuffer(n_out * 8)
    st = [rt.Stats() for _ in range(4)]
    assert rt.camera_rays_device(cam, W, H, rt.RT_RAYS_CENTRE, rows, d_rays, stream=stream, stats=st[0]) == n
    rt.query_intersect_device(sc, d_rays, n, d_hits, d_mask, stream=stream, stats=st[1])
    rt.rays_wo_device(d_rays, n, d_wo, stream=stream)
    rt.query_shade_device(sc, d_hits, d_wo, d_mask, n, d_rgb, lights=lights, miss_rgb=(1.0, 1.0, 1.0), stream=stream,
                          stats=st[2])
    rt.paper_resolve_device(d_hits, d_mask, d_rgb, W, H, row0, n_rows, d_fb, d_edge, stream=stream, stats=st[3])
    if times is not None:
        times.update(rays=st[0].ms_kernel, intersect=st[1].ms_kernel, shade=st[2].ms_kernel, resolve=st[3].ms_kernel)
    return d_fb.to_host(shape=(n_rows, W, 3)), d_edge.to_host(shape=(n_rows, W))


def _scene(rt, name, dpi=25):
    if name.startswith("graph"):
        return rt.load_scene_from_json_text(json.dumps(scenes.graph_scene(int(name.split()[1]), dpi=dpi)))
    return rt.load_scene_from_json_text(json.dumps(scenes.with_dpi(scenes.load_example(name), dpi)))


@pytest.mark.parametrize("name", ["penguin", "pokeballs", "snorlax", "graph 3"])
def test_frame_composed_on_the_device(gpu, name):
    sc = _scene(gpu, name)   # the camera is 100 x 75
    for W, H in ((100, 60), (65, 37)):
        fb, edge = compose(gpu, sc, sc, W, H)
        ref, _ = gpu.oracle_render(sc, W, H, gpu.RT_MODE_PAPER)
        frame = gpu.Tracer(sc, W, H, gpu.RT_MODE_PAPER).render()
        d_or, d_fr = int((fb != ref).any(axis=2).sum()), int((fb != frame).any(axis=2).sum())
        print(f"  {name} {W}x{H}: pixels differing from the oracle {d_or}, from rt_render {d_fr}; "
              f"edge pixels {int((edge > 0).sum())}")
        assert np.array_equal(fb, ref), (name, W, H, d_or)
        assert np.array_equal(fb, frame), (name, W, H, d_fr)
        assert (edge > 0).any()
        # two bands with halos
        cut = H // 2 + 1
        top, top_edge = compose(gpu, sc, sc, W, H, 0, cut)
        bottom, bottom_edge = compose(gpu, sc, sc, W, H, cut, H - cut)
        assert np.array_equal(np.concatenate([top, bottom]), ref), (name, W, H, "bands")
        assert np.array_equal(bits(np.concatenate([top_edge, bottom_edge])), bits(edge)), (name, W, H, "bands")


def test_paper_frame_from_a_moved_camera_and_under_other_lights(gpu):
    lib = gpu.amd_lib()
    sc = _scene(gpu, "pokeballs", dpi=16)
    gpu.Tracer(sc, sc.width, sc.height, gpu.RT_MODE_PAPER).render()   # (the scene is resident from here on)
    cam = gpu.Camera.from_buffer_copy(sc.desc.camera)
    cam.eye[0] += 0.4
    cam.eye[1] += 0.1
    cam.dpi = 20
    W, H = lib.rt_camera_width(C.byref(cam)), lib.rt_camera_height(C.byref(cam))
    assert (W, H) != (sc.width, sc.height)
    t = (C.c_double * 4)()

    def scene_ms():
        assert lib.rt_setup_times(t, 4) == 0
        return t[0]

    ms0 = scene_ms()
    fb, _ = compose(gpu, sc, cam, W, H)
    lights = [([2.0, 4.0, 3.0], [0.9, 0.8, 0.7]), ([-3.0, 1.0, 2.0], [0.3, 0.3, 0.5])]
    relit, _ = compose(gpu, sc, cam, W, H, lights=lights)
    assert scene_ms() == ms0   # no scene was compiled or uploaded for the camera or the lights
    desc = gpu.SceneDesc.from_buffer_copy(sc.desc)   # (shares the scene's arrays: `sc` stays alive)
    desc.camera = cam
    moved = gpu.scene_from_desc(desc)
    ref, _ = gpu.oracle_render(moved, W, H, gpu.RT_MODE_PAPER)
    assert np.array_equal(fb, ref), int((fb != ref).any(axis=2).sum())
    ref2, _ = gpu.oracle_render(gpu.with_point_lights(moved, lights), W, H, gpu.RT_MODE_PAPER)
    assert np.array_equal(relit, ref2), int((relit != ref2).any(axis=2).sum())
    assert not np.array_equal(ref, ref2)


# ------------------------------------------------------------ 3. rays_wo_device
def _device_wo(rt, rays, shift=0):
    n = len(rays)
    d_rays = rt.DeviceBuffer(max(n, 1) * 64)
    d_rays.from_host(rays)
    d_wo = _guarded(rt, n * 24 + shift)
    rt.rays_wo_device(d_rays, n, _At(d_wo, shift))
    return _out(d_wo, n * 24 + shift, None)[shift // 8:].reshape(n, 3)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_device_wo_is_the_host_wo(gpu, n):
    sets = wo_ray_sets(gpu)
    every = np.concatenate(list(sets.values()))   # ordinary, unnormalised, short and odd directions
    rays = np.resize(every, n) if n > len(every) else every[len(every) - n:]   # (the odd groups are at the end)
    want = gpu.rays_wo(rays)
    assert np.array_equal(bits(_device_wo(gpu, rays)), bits(want))
    assert np.array_equal(bits(_device_wo(gpu, rays, shift=8)), bits(want))   # a wo that is not 16-byte aligned


def test_device_wo_of_every_odd_group_and_no_launch_for_none(gpu):
    for name, rays in wo_ray_sets(gpu).items():
        assert np.array_equal(bits(_device_wo(gpu, rays)), bits(gpu.rays_wo(rays))), name
    d = gpu.DeviceBuffer(64)
    gpu.launch_log(True)
    try:
        gpu.rays_wo_device(d, 0, d)
        assert gpu.launch_log_get() == []
        gpu.rays_wo_device(d, 1, gpu.DeviceBuffer(24))
        assert gpu.launch_log_get() == ["rtd::k_rays_wo<true>"]
    finally:
        gpu.launch_log(False)


def test_device_wo_of_camera_rays_is_the_frames(gpu):
    """On the rays the frames trace, wo is bit for bit what the host form gives for the oracle's rays."""
    sc, W, H = load_frame_scene(gpu, "penguin wide")
    d_rays, d_wo = gpu.DeviceBuffer(W * H * 64), gpu.DeviceBuffer(W * H * 24)
    gpu.camera_rays_device(sc, W, H, gpu.RT_RAYS_CENTRE, None, d_rays)
    gpu.rays_wo_device(d_rays, W * H, d_wo)
    d = gpu.oracle_primary_hits(sc, W, H)["d"]
    assert np.array_equal(bits(d_wo.to_host(shape=(W * H, 3))), bits(gpu.rays_wo(gpu.make_rays(np.zeros_like(d), d))))


# ---------------------------------------------------------- 4. the resident scene
def test_the_resident_scene_is_left_alone(gpu):
    lib = gpu.amd_lib()
    sc = _scene(gpu, "snorlax", dpi=16)
    W, H = sc.width, sc.height
    before = gpu.Tracer(sc, W, H, gpu.RT_MODE_PAPER).render()
    t = (C.c_double * 4)()
    assert lib.rt_setup_times(t, 4) == 0
    ms0 = t[0]
    fb, _ = compose(gpu, sc, sc, W, H)
    hits, mask, rgb = synthetic_grid(gpu, 65, 9, 3)
    device_resolve(gpu, hits, mask, rgb, 65, 9, 0, 9)
    after = gpu.Tracer(sc, W, H, gpu.RT_MODE_PAPER).render()
    again, _ = compose(gpu, sc, sc, W, H)
    assert lib.rt_setup_times(t, 4) == 0
    assert t[0] == ms0   # frames and queries after these calls upload nothing
    assert after.tobytes() == before.tobytes() == fb.tobytes()
    assert again.tobytes() == fb.tobytes()
