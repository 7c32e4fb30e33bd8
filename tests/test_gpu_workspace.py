"""GPU: every group of the device workspace (the resident scene with its node
programs and ray BVH, the frame buffers, the query staging buffers, the events)
is released by rt_shutdown and rebuilt by the next call, and a displaced scene
comes back as it was.

One round runs every entry-point family once at the smallest shapes at which
this code can go wrong - the config-3 scene at a 24 x 10 frame (no multiple of
a 16- or 64-pixel tile, nor of 4 rows), 130 rays (two waves and two lanes), row
subsets out of order - and is repeated after shutdown(), and a third time with
no shutdown between.  Config 3 has no CSG node, so the node interval query on a
CSG node is config 4's (at dpi 8), in the middle of the round: every round
therefore also displaces the first scene by a second and brings it back.
Every result of a later round equals the first round's byte for byte, and
rt_setup_times()[0] grows across each shutdown() and each displacement and
stands still between two calls on a resident scene."""
import ctypes as C

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

W, H, N = 24, 10, 130
FRAME_ROWS = [7, 2, 9, 0, 4]
RAY_ROWS = [8, 1, 5]
STD, PAPER = 0, 1


def _scene_ms(rt):
    t = (C.c_double * 4)()
    assert rt.amd_lib().rt_setup_times(t, 4) == 0
    return t[0]


def _frame(rt, sc, mode, flags, rows):
    buf = rt.DeviceBuffer(len(rows) * W * 3 * 8)
    st = rt.Stats()
    rc = rt.amd_lib().rt_render_rows_device(sc.handle, W, H, mode, flags, (C.c_int32 * len(rows))(*rows), len(rows),
                                            buf.ptr, None, C.byref(st))
    assert rc == 0, rt.last_error()
    out = buf.to_host().tobytes()
    buf.free()
    return out, (st.rays_intersect, st.rays_occluded, st.pixels)


def _dev(rt, arr):
    b = rt.DeviceBuffer(max(arr.nbytes, 1))
    b.from_host(arr)
    return b


def _csg_node(sc):
    d = sc.desc
    return next(i for i in range(d.n_nodes) if int(d.nodes[i].kind) == 6)


def _round(rt, a, b):
    """Every family once; {name: bytes or tuple}, and the setup time before /
    after the second scene's call / after the first scene's next call."""
    out = {}
    out["std"] = _frame(rt, a, STD, 0, FRAME_ROWS)
    out["paper"] = _frame(rt, a, PAPER, 0, FRAME_ROWS)
    out["fp32"] = _frame(rt, a, STD, rt.RT_FLAG_FP32, FRAME_ROWS)
    centre = rt.camera_rays(a, W, H, rt.RT_RAYS_CENTRE)   # all rows in order
    out["centre"] = centre.tobytes()
    out["centre rows"] = rt.camera_rays(a, W, H, rt.RT_RAYS_CENTRE, rows=RAY_ROWS).tobytes()
    out["jittered rows"] = rt.camera_rays(a, W, H, rt.RT_RAYS_JITTERED, rows=RAY_ROWS).tobytes()
    rays = centre.reshape(-1)[:N]
    o, d = rays["o"], rays["d"]
    q = rt.query_intersect(a, o, d)
    out["intersect"] = (q.records.tobytes(), q.hit.tobytes())
    qb = rt.query_intersect(a, o, d, flags=rt.RT_FLAG_RAY_BVH)
    out["intersect ray bvh"] = (qb.records.tobytes(), qb.hit.tobytes())
    out["occluded"] = rt.query_occluded(a, o, d).tobytes()
    rgb = rt.query_radiance(a, o, d)
    out["radiance"] = rgb.tobytes()
    wo = -d / np.linalg.norm(d, axis=1, keepdims=True)
    lights = [((2.0, 5.0, 3.0), (30.0, 20.0, 10.0)), ((-4.0, 1.0, 6.0), (5.0, 15.0, 25.0))]
    out["shade"] = rt.query_shade(a, q.records, wo, mask=q.hit, lights=lights).tobytes()
    e, x, ok = rt.query_node_interval(a, 0, o, d)
    out["node interval"] = (e.tobytes(), x.tobytes(), ok.tobytes())

    ms = [_scene_ms(rt)]
    e, x, ok = rt.query_node_interval(b, _csg_node(b), o, d)   # the second scene displaces the first
    out["csg node interval"] = (e.tobytes(), x.tobytes(), ok.tobytes())
    ms.append(_scene_ms(rt))

    # bounce: the parents' children, then the fold of (made-up) child colours into the parents' own
    hit8 = q.hit.astype(np.uint8)
    d_rays, d_hits, d_mask = _dev(rt, rays), _dev(rt, q.records), _dev(rt, hit8)
    d_spawn, d_first = rt.DeviceBuffer(N), rt.DeviceBuffer(8 * N)
    d_crays, d_cw = rt.DeviceBuffer(2 * N * rt.RAY_DTYPE.itemsize), rt.DeviceBuffer(2 * N * 8)
    m = rt.scatter_rays_device(a, d_rays, d_hits, d_mask, N, 0, d_spawn, d_first, d_crays, d_cw, 2 * N)   # the first scene is back
    ms.append(_scene_ms(rt))
    child_rgb = np.linspace(0.0, 1.0, 3 * 2 * N).reshape(2 * N, 3)
    d_rgb, d_crgb = _dev(rt, rgb), _dev(rt, child_rgb)
    rt.combine_bounce_device(d_rgb, d_spawn, d_first, N, d_crgb, d_cw, m)
    out["scatter"] = (m, d_spawn.to_host(np.uint8).tobytes(), d_first.to_host(np.uint64).tobytes(),
                      d_crays.to_host(np.uint8)[:m * rt.RAY_DTYPE.itemsize].tobytes(), d_cw.to_host()[:m].tobytes())
    out["combine"] = d_rgb.to_host().tobytes()

    # paper resolve of the whole 24 x 10 frame from the centre rays' hits
    full = centre.reshape(-1)
    qf = rt.query_intersect(a, full["o"], full["d"])
    d_fh, d_fm = _dev(rt, qf.records), _dev(rt, qf.hit.astype(np.uint8))
    d_frgb = _dev(rt, np.linspace(0.0, 1.0, 3 * W * H))
    d_fb, d_edge = rt.DeviceBuffer(W * H * 24), rt.DeviceBuffer(W * H * 8)
    rt.paper_resolve_device(d_fh, d_fm, d_frgb, W, H, 0, H, d_fb, d_edge)
    out["paper resolve"] = (d_fb.to_host().tobytes(), d_edge.to_host().tobytes())
    for buf in (d_rays, d_hits, d_mask, d_spawn, d_first, d_crays, d_cw, d_rgb, d_crgb, d_fh, d_fm, d_frgb, d_fb, d_edge):
        buf.free()
    return out, ms


def test_every_group_is_released_and_rebuilt(gpu):
    rt = gpu
    a = rt.load_scene_from_json_text(scenes.config_json(3, dpi=24)[0])
    b = rt.load_scene_from_json_text(scenes.config_json(4, dpi=8)[0])
    rt.shutdown()   # (whatever earlier test files left resident)
    t0 = _scene_ms(rt)
    first, ms1 = _round(rt, a, b)
    assert any(first["intersect"][1]) and any(first["csg node interval"][2])   # (some rays hit, some intervals exist)
    assert first["intersect ray bvh"] == first["intersect"]
    rt.shutdown()
    t1 = _scene_ms(rt)
    second, ms2 = _round(rt, a, b)
    t2 = _scene_ms(rt)
    third, ms3 = _round(rt, a, b)   # no shutdown: the second scene displaced the first, and the first came back
    for name, want in first.items():
        assert second[name] == want, f"{name}: after shutdown()"
        assert third[name] == want, f"{name}: after a displacement"
    # compile + upload time: grows across each shutdown() ...
    assert t0 < ms1[0] and t1 < ms2[0], (t0, ms1, t1, ms2)
    # ... and across each displacement (the second scene in, the first scene back), in every round
    for ms in (ms1, ms2, ms3):
        assert ms[0] < ms[1] < ms[2], ms
    # (round 3 finds the first scene resident; its FP32 frame displaces the FP64 copy, which the next call brings back)
    assert t2 < ms3[0]
    # ... and stands still between two calls on a resident scene
    _frame(rt, a, STD, 0, FRAME_ROWS)
    ta = _scene_ms(rt)
    again = _frame(rt, a, STD, 0, FRAME_ROWS)
    q = rt.query_occluded(a, *[rt.camera_rays(a, W, H, rt.RT_RAYS_CENTRE).reshape(-1)[:N][k] for k in ("o", "d")])
    assert _scene_ms(rt) == ta
    assert again == first["std"] and q.tobytes() == first["occluded"]
    print(f"  scene setup ms: {t0:.3f} -> round 1 {ms1} -> shutdown {t1:.3f} -> round 2 {ms2} -> round 3 {ms3}")
