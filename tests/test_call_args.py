"""The argument failures of the frame path and of the batched entry points
that return before any device call (no device is touched: this file runs
without a GPU): the status and the whole rt_last_error() text of each, the
order of the checks where two faults meet, and the n == 0 calls.

The expected texts are written out here as the library gave them before its
render host file was split by concern (rt_frame.hip, rt_batch.hip,
rt_workspace.hip): the split may not change one byte of them."""
import ctypes as C

import numpy as np
import pytest

import scenes

OK, INVALID, UNSUPPORTED = 0, -1, -6
FP32_MSG = "ray queries have no FP32 kernels (RT_FLAG_FP32): they run the FP64 parity path"
COUNT_MSG = "ray queries do not count ops (RT_FLAG_COUNT_OPS)"
UNKNOWN_BIT = 64   # the first bit above RT_FLAG_RAY_BVH


@pytest.fixture(scope="module")
def sc(rt):
    text, _ = scenes.config_json(3, dpi=24)
    return rt.load_scene_from_json_text(text)


@pytest.fixture(scope="module")
def buf():
    """Host memory to point at: no call here gets as far as reading it."""
    a = np.zeros(4096, dtype=np.uint8)
    return a, C.c_void_p(a.ctypes.data)


def _rows(v):
    return (C.c_int32 * len(v))(*v)


def _check(rt, rc, want_rc, want_msg, what):
    assert rc == want_rc, (what, rc, rt.last_error())
    assert rt.last_error() == want_msg, what


def _zeroed(st):
    return (st.rays_traced, st.rays_intersect, st.rays_occluded, st.pixels, st.n_gpus) == (0, 0, 0, 0, 1)


def _dirty(rt):
    st = rt.Stats()
    st.rays_traced = st.rays_intersect = st.rays_occluded = st.pixels = 77
    st.n_gpus = 9
    return st


# ------------------------------------------------------------- frame path
FRAME_CASES = [
    # (what, scene?, W, H, mode, rows, n_rows, message)
    ("NULL scene", False, 24, 10, 0, [0], 1, "rt_render: scene is NULL"),
    ("W = 0", True, 0, 10, 0, [0], 1, "rt_render: W and H must be > 0"),
    ("H = -1", True, 24, -1, 0, [0], 1, "rt_render: W and H must be > 0"),
    ("bad mode", True, 24, 10, 2, [0], 1, "rt_render: bad mode"),
    ("negative n_rows", True, 24, 10, 0, [0], -1, "rt_render: bad rows"),
    ("NULL rows with n_rows > 0", True, 24, 10, 0, None, 2, "rt_render: bad rows"),
    ("a row equal to H", True, 24, 10, 1, [0, 10], 2, "rt_render: row out of range"),
    ("a negative row", True, 24, 10, 0, [-1], 1, "rt_render: row out of range"),
    ("a duplicate row", True, 24, 10, 0, [3, 5, 3], 3, "rt_render: duplicate row"),
    # two faults at once: the order of the checks
    ("NULL scene and W = 0", False, 0, 10, 0, [0], 1, "rt_render: scene is NULL"),
    ("W = 0 and bad mode", True, 0, 10, 7, [0], 1, "rt_render: W and H must be > 0"),
    ("bad mode and a duplicate row", True, 24, 10, 2, [3, 3], 2, "rt_render: bad mode"),
    ("a duplicate row, then a row out of range", True, 24, 10, 0, [3, 3, 10], 3, "rt_render: duplicate row"),
    ("a row out of range, then a duplicate row", True, 24, 10, 0, [10, 3, 3], 3, "rt_render: row out of range"),
]


@pytest.mark.parametrize("case", FRAME_CASES, ids=[c[0] for c in FRAME_CASES])
def test_frame_argument_failures(rt, sc, buf, case):
    what, with_scene, W, H, mode, rows, n_rows, msg = case
    lib = rt.amd_lib()
    h = sc.handle if with_scene else None
    r = _rows(rows) if rows is not None else None
    _check(rt, lib.rt_render_rows_device(h, W, H, mode, 0, r, n_rows, buf[1], None, None), INVALID, msg, what)
    f = C.c_void_p(1234)
    _check(rt, lib.rt_frame_begin(h, W, H, mode, 0, r, n_rows, None, C.byref(f)), INVALID, msg, what)
    assert f.value is None, what   # (*out is NULL after a failure)


def test_frame_entry_points_own_checks(rt, sc, buf):
    lib = rt.amd_lib()
    # rt_render_rows_device looks at its output before the frame's arguments; rt_frame_begin at `out`
    _check(rt, lib.rt_render_rows_device(None, 0, 0, 9, 0, _rows([0]), 1, None, None, None), INVALID,
           "rt_render: bad rows/fb", "NULL fb before everything else")
    _check(rt, lib.rt_frame_begin(None, 0, 0, 9, 0, None, -1, None, None), INVALID, "rt_frame_begin: out is NULL",
           "NULL out before everything else")
    _check(rt, lib.rt_frame_trace(None, 0, 1, buf[1], None), INVALID, "rt_frame_trace: frame is NULL", "trace")
    _check(rt, lib.rt_frame_end(None, None), INVALID, "rt_frame_end: frame is NULL", "end")
    _check(rt, lib.rt_render(sc.handle, 24, 10, 0, 0, None, None), INVALID, "rt_render: fb is NULL", "rt_render fb")
    fb = np.zeros(3)
    _check(rt, lib.rt_render(sc.handle, 0, 10, 0, 0, fb.ctypes.data_as(C.POINTER(C.c_double)), None), INVALID,
           "rt_render: W and H must be > 0", "rt_render W")
    _check(rt, lib.rt_render(None, 0, 10, 0, 0, None, None), INVALID, "rt_render: fb is NULL", "rt_render fb first")


# ---------------------------------------------------------- query families
def _ray_families(lib, p):
    """name -> call(scene, rays, n, flags, result, stats) of the six ray and radiance forms and their depth twins."""
    return {
        "rt_query_intersect": lambda s, r, n, fl, out, st: lib.rt_query_intersect(s, r, n, fl, out, None, st),
        "rt_query_intersect_device": lambda s, r, n, fl, out, st: lib.rt_query_intersect_device(s, r, n, fl, out, p, None, st),
        "rt_query_occluded": lambda s, r, n, fl, out, st: lib.rt_query_occluded(s, r, n, fl, out, st),
        "rt_query_occluded_device": lambda s, r, n, fl, out, st: lib.rt_query_occluded_device(s, r, n, fl, out, None, st),
        "rt_query_radiance": lambda s, r, n, fl, out, st: lib.rt_query_radiance(s, r, n, fl, out, st),
        "rt_query_radiance_device": lambda s, r, n, fl, out, st: lib.rt_query_radiance_device(s, r, n, fl, out, None, st),
        "rt_query_radiance_depth": lambda s, r, n, fl, out, st: lib.rt_query_radiance_depth(s, r, n, fl, 2, out, st),
        "rt_query_radiance_depth_device":
            lambda s, r, n, fl, out, st: lib.rt_query_radiance_depth_device(s, r, n, fl, 2, out, None, st),
    }


def _shade_families(lib, p):
    """The same shape for the shading queries: rays -> hits (wo, rgb and no lights of its own are given)."""
    return {
        "rt_query_shade": lambda s, h, n, fl, out, st: lib.rt_query_shade(s, h, p, None, n, None, -1, None, fl, out, st),
        "rt_query_shade_device":
            lambda s, h, n, fl, out, st: lib.rt_query_shade_device(s, h, p, None, n, None, -1, None, fl, out, None, st),
    }


def _node_families(lib, node=0):
    """The same shape for the node queries of node `node` (interval: the result is the enter records)."""
    return {
        "rt_query_node_intersect":
            lambda s, r, n, fl, out, st: lib.rt_query_node_intersect(s, node, r, n, fl, out, None, st),
        "rt_query_node_intersect_device":
            lambda s, r, n, fl, out, st: lib.rt_query_node_intersect_device(s, node, r, n, fl, out, None, None, st),
        "rt_query_node_interval":
            lambda s, r, n, fl, out, st: lib.rt_query_node_interval(s, node, r, n, fl, out, None, None, st),
        "rt_query_node_interval_device":
            lambda s, r, n, fl, out, st: lib.rt_query_node_interval_device(s, node, r, n, fl, out, None, None, None, st),
    }


def _all_families(lib, p):
    return {**_ray_families(lib, p), **_shade_families(lib, p), **_node_families(lib)}


QUERY_NAMES = ["rt_query_intersect", "rt_query_intersect_device", "rt_query_occluded", "rt_query_occluded_device",
               "rt_query_radiance", "rt_query_radiance_device", "rt_query_radiance_depth",
               "rt_query_radiance_depth_device", "rt_query_shade", "rt_query_shade_device", "rt_query_node_intersect",
               "rt_query_node_intersect_device", "rt_query_node_interval", "rt_query_node_interval_device"]


@pytest.mark.parametrize("name", QUERY_NAMES)
def test_query_argument_failures(rt, sc, buf, name):
    lib = rt.amd_lib()
    p = buf[1]
    call = _all_families(lib, p)[name]
    h = sc.handle
    first = "hits" if "shade" in name else "rays"
    cases = [
        ("NULL scene", (None, p, 4, 0, p), INVALID, f"{name}: scene is NULL"),
        ("an unknown flag bit", (h, p, 4, UNKNOWN_BIT, p), INVALID, f"{name}: unknown flag bits"),
        ("RT_FLAG_FP32", (h, p, 4, rt.RT_FLAG_FP32, p), UNSUPPORTED, FP32_MSG),
        ("RT_FLAG_COUNT_OPS", (h, p, 4, rt.RT_FLAG_COUNT_OPS, p), UNSUPPORTED, COUNT_MSG),
        ("RT_FLAG_FP32 | RT_FLAG_COUNT_OPS", (h, p, 4, rt.RT_FLAG_FP32 | rt.RT_FLAG_COUNT_OPS, p), UNSUPPORTED, FP32_MSG),
        (f"NULL {first}", (h, None, 4, 0, p), INVALID, f"{name}: {first} is NULL"),
        ("NULL result", (h, p, 4, 0, None), INVALID, f"{name}: the result buffer is NULL"),
        # two faults at once: the order of the checks
        ("NULL scene and an unknown bit", (None, p, 4, UNKNOWN_BIT, p), INVALID, f"{name}: scene is NULL"),
        ("an unknown bit and RT_FLAG_FP32", (h, p, 4, UNKNOWN_BIT | rt.RT_FLAG_FP32, p), INVALID,
         f"{name}: unknown flag bits"),
        ("RT_FLAG_COUNT_OPS and NULL input", (h, None, 4, rt.RT_FLAG_COUNT_OPS, p), UNSUPPORTED, COUNT_MSG),
        ("NULL input and NULL result", (h, None, 4, 0, None), INVALID, f"{name}: {first} is NULL"),
        # the scene and the flags are checked at n == 0 too
        ("NULL scene at n == 0", (None, None, 0, 0, None), INVALID, f"{name}: scene is NULL"),
        ("an unknown bit at n == 0", (h, None, 0, UNKNOWN_BIT, None), INVALID, f"{name}: unknown flag bits"),
    ]
    for what, args, rc, msg in cases:
        st = _dirty(rt)
        _check(rt, call(*args, C.byref(st)), rc, msg, what)
        # the stats are zeroed once the scene and the flags are fine, before the buffers are looked at
        if msg.endswith("is NULL") and "scene" not in msg:
            assert _zeroed(st), what
        else:
            assert st.n_gpus == 9 and st.pixels == 77, what
    # n == 0: RT_OK, stats zeroed with n_gpus == 1, nothing else looked at
    st = _dirty(rt)
    assert call(h, None, 0, 0, None, C.byref(st)) == OK
    assert _zeroed(st)
    assert call(h, None, 0, 0, None, None) == OK


def test_shade_own_checks(rt, sc, buf):
    lib, p, h = rt.amd_lib(), buf[1], sc.handle
    for name, fn in (("rt_query_shade", lambda *a: lib.rt_query_shade(*a, None)),
                     ("rt_query_shade_device", lambda *a: lib.rt_query_shade_device(*a, None, None))):
        # (scene, hits, wo, mask, n, lights, n_lights, miss, flags, rgb)
        _check(rt, fn(h, p, None, None, 4, None, -1, None, 0, p), INVALID, f"{name}: wo is NULL", name)
        _check(rt, fn(h, p, p, None, 4, None, 2, None, 0, p), INVALID, f"{name}: lights is NULL with n_lights > 0", name)
        _check(rt, fn(h, None, None, None, 4, None, 2, None, 0, None), INVALID, f"{name}: hits is NULL", name)
        _check(rt, fn(h, p, None, None, 4, None, 2, None, 0, None), INVALID, f"{name}: wo is NULL", name)
        _check(rt, fn(h, p, p, None, 4, None, 2, None, 0, None), INVALID, f"{name}: the result buffer is NULL", name)


def test_node_own_checks(rt, sc, buf):
    lib, p, h = rt.amd_lib(), buf[1], sc.handle
    n_nodes = sc.desc.n_nodes
    for node in (-1, n_nodes, n_nodes + 7):
        for name, call in _node_families(lib, node).items():
            msg = f"{name}: node is outside [0, n_nodes)"
            _check(rt, call(h, p, 4, 0, p, None), INVALID, msg, (name, node))
            # ... after the flags, before n == 0 and the buffers
            _check(rt, call(h, None, 0, 0, None, None), INVALID, msg, (name, node, "n == 0"))
            _check(rt, call(h, None, 4, 0, None, None), INVALID, msg, (name, node, "NULL rays"))
            _check(rt, call(h, p, 4, rt.RT_FLAG_FP32, p, None), UNSUPPORTED, FP32_MSG, (name, node, "flags first"))
    # an interval query needs one of its three results
    _check(rt, lib.rt_query_node_interval(h, 0, p, 4, 0, None, None, None, None), INVALID,
           "rt_query_node_interval: the result buffer is NULL", "interval results")
    _check(rt, lib.rt_query_node_interval_device(h, 0, p, 4, 0, None, None, None, None, None), INVALID,
           "rt_query_node_interval_device: the result buffer is NULL", "interval results")


# ------------------------------------------------------------- camera rays
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_camera_rays_argument_failures(rt, sc, buf, device):
    lib, p = rt.amd_lib(), buf[1]
    name = "rt_camera_rays_device" if device else "rt_camera_rays"
    cam = C.byref(sc.desc.camera)
    W, H = 24, 10

    def call(cam_p, W, H, kind, rows, n_rows, out, st=None):
        r = _rows(rows) if rows is not None else None
        if device:
            return lib.rt_camera_rays_device(cam_p, W, H, kind, r, n_rows, out, None, st)
        return lib.rt_camera_rays(cam_p, W, H, kind, r, n_rows, out, st)

    cases = [
        ("NULL cam", (None, W, H, 0, None, H, p), "cam is NULL"),
        ("W = 0", (cam, 0, H, 0, None, H, p), "W and H must be > 0"),
        ("kind = 2", (cam, W, H, 2, None, H, p), "unknown kind"),
        ("W beyond a launch's row", (cam, 1 << 28, H, 1, None, H, p), "W is beyond one launch's row"),
        ("negative n_rows", (cam, W, H, 0, [0], -1, p), "bad rows"),
        ("n_rows > H", (cam, W, H, 0, [0] * 11, 11, p), "bad rows"),
        ("NULL rows with n_rows != H", (cam, W, H, 0, None, 3, p), "rows is NULL with n_rows != H"),
        ("a row equal to H", (cam, W, H, 0, [0, H], 2, p), "row out of range"),
        ("a negative row", (cam, W, H, 1, [-1], 1, p), "row out of range"),
        ("a duplicate row", (cam, W, H, 1, [3, 5, 3], 3, p), "duplicate row"),
        ("NULL rays", (cam, W, H, 0, [7, 2], 2, None), "the ray buffer is NULL"),
        # two faults at once: the order of the checks
        ("NULL cam and W = 0", (None, 0, H, 0, None, H, p), "cam is NULL"),
        ("kind = 2 and bad rows", (cam, W, H, 2, [0], -1, p), "unknown kind"),
        ("a duplicate row, then a row out of range", (cam, W, H, 0, [3, 3, H], 3, p), "duplicate row"),
        ("a row out of range, then a duplicate row", (cam, W, H, 0, [H, 3, 3], 3, p), "row out of range"),
        ("a duplicate row and NULL rays", (cam, W, H, 0, [3, 3], 2, None), "duplicate row"),
    ]
    for what, args, msg in cases:
        _check(rt, call(*args), INVALID, f"{name}: {msg}", what)
    for kind in (0, 1):
        st = _dirty(rt)
        assert call(cam, W, H, kind, [], 0, None, C.byref(st)) == OK
        assert _zeroed(st)


# -------------------------------------------- bounce loop and paper resolve
def test_scatter_combine_resolve_argument_failures(rt, sc, buf):
    lib, p, h = rt.amd_lib(), buf[1], sc.handle
    a = buf[0].ctypes.data
    at = lambda off: C.c_void_p(a + off)
    m = C.c_size_t(55)
    mp = C.byref(m)

    def scatter(s, rays, hits, n, spawn, first, crays, cw, cap, nch, st=None):
        return lib.rt_scatter_rays_device(s, rays, hits, None, n, 0, spawn, first, crays, cw, cap, nch, None, st)

    name = "rt_scatter_rays_device"
    _check(rt, scatter(None, p, p, 1, p, p, p, p, 1, mp), INVALID, f"{name}: scene is NULL", "scene")
    _check(rt, scatter(h, p, p, 1, p, p, p, p, 1, None), INVALID, f"{name}: n_children is NULL", "n_children")
    _check(rt, scatter(None, p, p, 1, p, p, p, p, 1, None), INVALID, f"{name}: scene is NULL", "scene first")
    _check(rt, scatter(h, None, p, 1, p, p, p, p, 1, mp), INVALID, f"{name}: rays or hits is NULL", "rays")
    _check(rt, scatter(h, at(0), at(64), 1, None, at(256), at(512), at(1024), 1, mp), INVALID,
           f"{name}: spawn or first is NULL", "spawn")
    _check(rt, scatter(h, at(0), at(64), 1, at(128), at(256), None, at(1024), 1, mp), INVALID,
           f"{name}: a child buffer is NULL with child_cap > 0", "child")
    _check(rt, scatter(h, at(0), at(64), 1, at(0), at(256), at(512), at(1024), 1, mp), INVALID,
           f"{name}: an output overlaps an input", "overlap")
    assert m.value == 55   # (untouched by a refused call)
    st = _dirty(rt)
    assert scatter(h, None, None, 0, None, None, None, None, 0, mp, C.byref(st)) == OK
    assert m.value == 0 and _zeroed(st)

    name = "rt_combine_bounce_device"
    _check(rt, lib.rt_combine_bounce_device(None, p, p, 1, p, p, 1, None), INVALID, f"{name}: NULL buffer", "rgb")
    _check(rt, lib.rt_combine_bounce_device(at(0), at(64), at(128), 1, None, at(256), 1, None), INVALID,
           f"{name}: a child buffer is NULL with n_children > 0", "child")
    _check(rt, lib.rt_combine_bounce_device(at(0), at(64), at(128), 1, at(8), at(256), 1, None), INVALID,
           f"{name}: rgb overlaps child_rgb", "overlap")
    assert lib.rt_combine_bounce_device(None, None, None, 0, None, None, 0, None) == OK

    name = "rt_paper_resolve_device"

    def resolve(hits, rgb, W, H, row0, n_rows, fb, edge, st=None):
        return lib.rt_paper_resolve_device(hits, None, rgb, W, H, row0, n_rows, fb, edge, None, st)

    _check(rt, resolve(p, p, 0, 4, 0, 1, p, None), INVALID, f"{name}: W and H must be > 0", "W")
    _check(rt, resolve(p, p, 4, 4, 3, 2, p, None), INVALID, f"{name}: rows [row0, row0 + n_rows) must lie in [0, H)",
           "rows")
    _check(rt, resolve(None, p, 4, 4, 0, 1, p, None), INVALID, f"{name}: hits is NULL", "hits")
    _check(rt, resolve(p, p, 4, 4, 0, 1, None, None), INVALID, f"{name}: fb and edge are both NULL", "outputs")
    _check(rt, resolve(p, None, 4, 4, 0, 1, p, None), INVALID, f"{name}: rgb is NULL with an fb", "rgb")
    _check(rt, resolve(None, None, 0, 4, 9, 1, None, None), INVALID, f"{name}: W and H must be > 0", "W first")
    st = _dirty(rt)
    assert resolve(None, None, 4, 4, 2, 0, None, None, C.byref(st)) == OK
    assert _zeroed(st)

    name = "rt_rays_wo_device"
    _check(rt, lib.rt_rays_wo_device(None, 2, p, None), INVALID, f"{name}: NULL buffer", "rays")
    _check(rt, lib.rt_rays_wo_device(at(0), 2, at(64), None), INVALID, f"{name}: wo overlaps rays", "overlap")
    assert lib.rt_rays_wo_device(None, 0, None, None) == OK

    name = "rt_resolve_samples_device"
    _check(rt, lib.rt_resolve_samples_device(p, 4, 0, at(2048), None), INVALID, f"{name}: spp must be in [1, 64]", "spp")
    _check(rt, lib.rt_resolve_samples_device(None, 4, 8, at(2048), None), INVALID, f"{name}: NULL buffer", "rgb")
    _check(rt, lib.rt_resolve_samples_device(at(0), 4, 8, at(24), None), INVALID, f"{name}: fb overlaps rgb", "overlap")
    _check(rt, lib.rt_resolve_samples_device(None, 4, 65, None, None), INVALID, f"{name}: spp must be in [1, 64]",
           "spp first")
    assert lib.rt_resolve_samples_device(None, 0, 8, None, None) == OK
