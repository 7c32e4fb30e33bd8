"""GPU: the jitter cache (csrc/host/jitter_cache.hpp, rt_render.hip
frame_begin): a standard frame's draws stay resident by (W, H, rows), so only the
first frame of a key runs the fill and uploads the rows list.

The cache can go wrong in its key, its lifetime or its ordering, not in its
size, so the frames are tiny.  Every frame rendered with the cache on is
compared np.array_equal, ray counts included, with the same call at budget 0:
the path before the cache existed, in the same build (same kernels, same
inputs).  Each distinct (scene, size) is also compared once, on a hit, with
the CPU oracle at the project's standing 1e-5 with equal ray counts.  The
scenes have several lights (snorlax 3, penguin 3, config 4 five), so shading
depends on the draws."""
import ctypes as C
import json

import numpy as np
import pytest

import scenes

STD, PAPER = 0, 1
BIG = 64 << 20   # holds every entry of a test (a 64x48 entry is 393,600 B)

_off = {}        # budget-0 frames by (scene, W, H, mode, flags): (frame, Stats)
_oracled = set()


def _scene(rt, name, W, H):
    if name == "cfg4":
        sc = rt.load_scene_from_json_text(scenes.config_json(4, dpi=W // 4)[0])
    else:
        sc = rt.load_scene_from_json_text(json.dumps(scenes.with_size(scenes.load_example(name), W, H)))
    assert (sc.width, sc.height) == (W, H)
    return sc


def _render(rt, sc, W, H, mode=STD, flags=0):
    st = rt.Stats()
    return rt.Tracer(sc, W, H, mode, flags).render(st), st


def _rays(st):
    return (st.rays_intersect, st.rays_occluded)


def _render_rows(rt, sc, W, H, rows, flags=0):
    buf = rt.DeviceBuffer(len(rows) * W * 3 * 8)
    st = rt.Stats()
    rc = rt.amd_lib().rt_render_rows_device(sc.handle, W, H, STD, flags, (C.c_int32 * len(rows))(*rows), len(rows),
                                            buf.ptr, None, C.byref(st))
    assert rc == 0, rt.last_error()
    return buf.to_host(np.float64, (len(rows), W, 3)), st


def _budget0(rt, name, sc, W, H, mode=STD, flags=0):
    """The frame with the cache off (computed once per case, never changed).
    Leaves the budget at 0 and the counts zeroed."""
    key = (name, W, H, mode, flags)
    rt.jitter_cache_budget(0)
    if key not in _off:
        fb, st = _render(rt, sc, W, H, mode, flags)
        s = rt.jitter_cache_stats()
        assert (s["hits"], s["entries"], s["bytes"]) == (0, 0, 0)
        fb.setflags(write=False)
        _off[key] = (fb, st)
    return _off[key]


def _same(got, want):
    fb, st = got
    assert np.array_equal(fb, want[0])
    assert _rays(st) == _rays(want[1])


def _oracle_once(rt, name, sc, W, H, got):
    """(scene, size) against the CPU oracle, once, with a frame that was a hit."""
    if (name, W, H) in _oracled:
        return
    fb, st = got
    ref, ost = rt.oracle_render(sc, W, H, STD)
    err = float(np.abs(fb - ref).max())
    assert err <= 1e-5, err
    assert _rays(st) == (ost.rays_intersect, ost.rays_occluded)
    _oracled.add((name, W, H))


def _counts(rt, slot=None):
    s = rt.jitter_cache_stats(slot)
    return s["hits"], s["misses"]


@pytest.fixture(autouse=True)
def _device_and_budget(gpu):
    yield
    gpu.jitter_cache_budget(-1)   # back to RT_JITTER_CACHE_MB for the other test files


@pytest.mark.gpu
def test_repeat(rt):
    W, H = 64, 48
    sc = _scene(rt, "snorlax", W, H)
    off = _budget0(rt, "snorlax", sc, W, H)
    rt.jitter_cache_budget(BIG)
    f1 = _render(rt, sc, W, H)
    assert _counts(rt) == (0, 1)
    f2 = _render(rt, sc, W, H)
    assert _counts(rt) == (1, 1)
    s = rt.jitter_cache_stats()
    assert s["entries"] == 1 and 0 < s["bytes"] <= BIG
    _same(f1, off)
    _same(f2, off)
    assert np.array_equal(f1[0], f2[0])
    _oracle_once(rt, "snorlax", sc, W, H, f2)
    assert f2[1].ms_rng >= 0.0   # (its events are recorded on a hit too: an empty interval)


@pytest.mark.gpu
def test_same_byte_size_different_key(rt):
    """64x48 and 48x64 take the same number of draws: a stale hit would fit."""
    a, b = (64, 48), (48, 64)
    sa, sb = _scene(rt, "snorlax", *a), _scene(rt, "snorlax", *b)
    off_a, off_b = _budget0(rt, "snorlax", sa, *a), _budget0(rt, "snorlax", sb, *b)
    rt.jitter_cache_budget(BIG)
    _same(_render(rt, sa, *a), off_a)
    _same(_render(rt, sb, *b), off_b)
    assert _counts(rt) == (0, 2)
    third = _render(rt, sa, *a)
    assert _counts(rt) == (1, 2)
    _same(third, off_a)
    hit_b = _render(rt, sb, *b)
    assert _counts(rt) == (2, 2)
    _same(hit_b, off_b)
    _oracle_once(rt, "snorlax", sa, *a, third)
    _oracle_once(rt, "snorlax", sb, *b, hit_b)


@pytest.mark.gpu
def test_row_sets_of_one_size(rt):
    W, H = 64, 48
    sc = _scene(rt, "snorlax", W, H)
    full = _budget0(rt, "snorlax", sc, W, H)[0]
    sets = [list(range(0, 24)), list(range(24, 48)),
            [r for s in (0, 16, 32) for r in range(s, s + 8)]]
    assert len({len(s) for s in sets}) == 1   # equal length: equal buffer sizes
    rt.jitter_cache_budget(0)
    off_rays = [_rays(_render_rows(rt, sc, W, H, rows)[1]) for rows in sets]
    rt.jitter_cache_budget(BIG)
    for rnd in range(2):
        for k, rows in enumerate(sets):
            got, st = _render_rows(rt, sc, W, H, rows)
            assert np.array_equal(got, full[rows]), (rnd, k)
            assert _rays(st) == off_rays[k]
            assert _counts(rt) == ((0, k + 1) if rnd == 0 else (k + 1, 3)), (rnd, k)
    assert rt.jitter_cache_stats()["entries"] == 3


@pytest.mark.gpu
def test_same_rows_of_another_height(rt):
    """Output row r reads the stream at loop row H-1-r, so rows 0-7 of a
    64x48 frame and of a 64x56 frame are two keys (equal W, rows and bytes)."""
    W, rows = 64, list(range(8))
    cases = []
    for H in (48, 56):
        sc = _scene(rt, "snorlax", W, H)
        cases.append((H, sc, _budget0(rt, "snorlax", sc, W, H)[0]))
    rt.jitter_cache_budget(BIG)
    for rnd in range(2):
        for k, (H, sc, full) in enumerate(cases):
            got, st = _render_rows(rt, sc, W, H, rows)
            assert np.array_equal(got, full[rows]), (rnd, H)
            assert _counts(rt) == ((0, k + 1) if rnd == 0 else (k + 1, 2)), (rnd, H)
            if rnd == 1 and ("snorlax", W, H, "rows 0-7") not in _oracled:
                ref, ost = rt.oracle_render(sc, W, H, STD, 0, 8)
                assert float(np.abs(got - ref).max()) <= 1e-5
                assert _rays(st) == (ost.rays_intersect, ost.rays_occluded)
                _oracled.add(("snorlax", W, H, "rows 0-7"))


@pytest.mark.gpu
def test_scene_independence(rt):
    W, H = 64, 48
    first, second = _scene(rt, "snorlax", W, H), _scene(rt, "penguin", W, H)
    off = _budget0(rt, "penguin", second, W, H)
    off_first = _budget0(rt, "snorlax", first, W, H)
    assert not np.array_equal(off[0], off_first[0])
    rt.jitter_cache_budget(BIG)
    _same(_render(rt, first, W, H), off_first)
    got = _render(rt, second, W, H)
    assert _counts(rt) == (1, 1)   # another scene's first frame: a hit
    _same(got, off)
    _oracle_once(rt, "penguin", second, W, H, got)


@pytest.mark.gpu
def test_flags_and_modes(rt):
    W, H = 64, 48
    sc = _scene(rt, "snorlax", W, H)
    flags = [rt.RT_FLAG_FP32, rt.RT_FLAG_NO_CULL, rt.RT_FLAG_COUNT_OPS]
    off = {fl: _budget0(rt, "snorlax", sc, W, H, STD, fl) for fl in [0] + flags}
    off_paper = _budget0(rt, "snorlax", sc, W, H, PAPER)
    rt.jitter_cache_budget(BIG)
    _same(_render(rt, sc, W, H), off[0])
    assert _counts(rt) == (0, 1)
    _same(_render(rt, sc, W, H, STD, rt.RT_FLAG_FP32), off[rt.RT_FLAG_FP32])
    assert _counts(rt) == (1, 1)
    before = rt.jitter_cache_stats()
    _same(_render(rt, sc, W, H, PAPER), off_paper)   # a paper frame in between
    assert rt.jitter_cache_stats() == before
    _same(_render(rt, sc, W, H, STD, rt.RT_FLAG_FP32), off[rt.RT_FLAG_FP32])
    for n, fl in enumerate((rt.RT_FLAG_NO_CULL, rt.RT_FLAG_COUNT_OPS)):
        got = _render(rt, sc, W, H, STD, fl)
        assert _counts(rt) == (3 + n, 1)
        _same(got, off[fl])
        assert list(got[1].ops) == list(off[fl][1].ops)
    assert any(off[rt.RT_FLAG_COUNT_OPS][1].ops)
    assert rt.jitter_cache_stats()["entries"] == 1


@pytest.mark.gpu
def test_eviction_and_budget(rt):
    a, b = (64, 48), (40, 30)
    sa, sb = _scene(rt, "snorlax", *a), _scene(rt, "snorlax", *b)
    off_a, off_b = _budget0(rt, "snorlax", sa, *a), _budget0(rt, "snorlax", sb, *b)
    rt.jitter_cache_budget(BIG)
    _render(rt, sa, *a)
    bytes_a = rt.jitter_cache_stats()["bytes"]
    _render(rt, sb, *b)
    bytes_b = rt.jitter_cache_stats()["bytes"] - bytes_a
    assert 0 < bytes_b < bytes_a
    budget = bytes_a   # holds exactly one of the two
    rt.jitter_cache_budget(budget)
    for k in range(3):
        for sc, size, off in ((sa, a, off_a), (sb, b, off_b)):
            _same(_render(rt, sc, *size), off)
            s = rt.jitter_cache_stats()
            assert s["entries"] <= 1 and s["bytes"] <= budget
    assert _counts(rt) == (0, 6)   # each evicted the other
    hit_b = _render(rt, sb, *b)    # the resident one still hits
    assert _counts(rt) == (1, 6)
    _same(hit_b, off_b)
    _oracle_once(rt, "snorlax", sb, *b, hit_b)
    rt.jitter_cache_budget(bytes_b - 1)   # below one frame of either size
    for sc, size, off in ((sa, a, off_a), (sb, b, off_b), (sb, b, off_b)):
        _same(_render(rt, sc, *size), off)
        s = rt.jitter_cache_stats()
        assert (s["entries"], s["bytes"], s["hits"]) == (0, 0, 0)


@pytest.mark.gpu
def test_begin_without_trace(rt):
    W, H = 64, 48
    sc = _scene(rt, "snorlax", W, H)
    off = _budget0(rt, "snorlax", sc, W, H)
    rt.jitter_cache_budget(BIG)
    lib = rt.amd_lib()
    stream = rt.Stream()
    rows = list(range(H))   # rt_render's row list: the same key
    fr = C.c_void_p()
    rc = lib.rt_frame_begin(sc.handle, W, H, STD, 0, (C.c_int32 * H)(*rows), H, stream.handle, C.byref(fr))
    assert rc == 0, rt.last_error()
    assert lib.rt_frame_end(fr, None) == 0, rt.last_error()
    assert _counts(rt) == (0, 1)
    _same(_render(rt, sc, W, H), off)   # whether that entry counts as valid or not
    _same(_render(rt, sc, W, H), off)
    assert rt.jitter_cache_stats()["hits"] >= 1
    stream.destroy()


@pytest.mark.gpu
def test_shutdown_frees_the_entries(rt):
    W, H = 64, 48
    sc = _scene(rt, "snorlax", W, H)
    off = _budget0(rt, "snorlax", sc, W, H)
    rt.jitter_cache_budget(BIG)
    _same(_render(rt, sc, W, H), off)
    _same(_render(rt, sc, W, H), off)
    assert _counts(rt) == (1, 1) and rt.jitter_cache_stats()["entries"] == 1
    rt.shutdown()
    s = rt.jitter_cache_stats()
    assert (s["entries"], s["bytes"]) == (0, 0)
    _same(_render(rt, sc, W, H), off)
    assert _counts(rt) == (1, 2)   # a miss
    _same(_render(rt, sc, W, H), off)
    assert _counts(rt) == (2, 2)


@pytest.mark.gpu
def test_thread_ranks(rt):
    """World 2 on one GPU, each rank a host thread with its own workspace
    (slot rank + 1) and so its own cache: its strips are the same rows every
    frame."""
    W, H = 160, 90
    sc = _scene(rt, "cfg4", W, H)
    off = _budget0(rt, "cfg4", sc, W, H)
    rt.jitter_cache_budget(BIG)
    _render(rt, sc, W, H)
    one_gpu = _render(rt, sc, W, H)
    assert _counts(rt) == (1, 1)
    _same(one_gpu, off)
    _oracle_once(rt, "cfg4", sc, W, H, one_gpu)
    out, rc, _, msg = rt.dist_threads(sc, W, H, STD, 2, frames=2)
    assert (rc == 0).all(), msg
    for f in range(2):
        assert np.array_equal(out[f], one_gpu[0]), f
    for rank in range(2):
        assert _counts(rt, slot=rank + 1) == (1, 1), rank   # the first frame filled, the second did not
    assert _counts(rt) == (1, 1)   # (the process's own workspace took no part)
