"""The paper-mode frame plan executed on the device at a shape the other GPU
tests do not reach: an odd width (the one-pixel-per-thread finish pass, a
partial 16-column primary block) and one strip plus a row, traced by two
rt_frame_trace calls on two streams: the second call has no primary hit left
to compute (the first traced row 30 as row 29's neighbour), and its finish
pass waits for the first call's primary pass across the streams
(csrc/host/frame_plan.hpp PaperCalls)."""
import ctypes as C

import numpy as np
import pytest

import scenes


@pytest.mark.gpu
def test_paper_strip_plus_a_row_on_two_streams(gpu):
    rt = gpu
    W, H, mode = 17, 31, 1
    sc = rt.load_scene_from_json_text(scenes.config_json(5, dpi=24)[0])
    lib = rt.amd_lib()
    rows = list(range(H))
    streams = [rt.Stream(), rt.Stream()]
    row_bytes = W * 3 * 8
    buf = rt.DeviceBuffer(H * row_bytes)
    fr = C.c_void_p()
    rc = lib.rt_frame_begin(sc.handle, W, H, mode, 0, (C.c_int32 * H)(*rows), H, streams[0].handle, C.byref(fr))
    assert rc == 0, rt.last_error()
    for k, (a, b) in enumerate([(0, 30), (30, 31)]):
        rc = lib.rt_frame_trace(fr, a, b, C.c_void_p(buf.ptr.value + a * row_bytes), streams[k].handle)
        assert rc == 0, rt.last_error()
    st = rt.Stats()
    assert lib.rt_frame_end(fr, C.byref(st)) == 0, rt.last_error()
    rt.device_synchronize()
    fb = buf.to_host(np.float64, (H, W, 3))
    ref, ost = rt.oracle_render(sc, W, H, mode)
    assert np.array_equal(fb, ref)
    assert (st.rays_intersect, st.rays_occluded) == (ost.rays_intersect, ost.rays_occluded)
