"""The frame planners (csrc/host/frame_plan.hpp): which rows a rank owns, how
they are chunked and where a gathered slot lands, the standard-mode jitter
layout, the paper-mode halo rows and per-call lists, and the kernel a frame
launches.  rt_render.hip and rt_dist.hip execute these plans; here they run at
full frame sizes on the CPU through the rt_test_plan_* hooks (host code only:
no device is touched)."""
import ctypes as C
import json
import os

import pytest

import frame_dist
import scenes
from conftest import GOLDEN

I32, I64 = C.c_int32, C.c_int64
STD, PAPER = 0, 1
RT_ERR_UNSUPPORTED = -6


@pytest.fixture(scope="module")
def lib(rt):
    return rt.amd_lib()


# ------------------------------------------------------------------ dist plan
def _dist(lib, H, world, rank, mode, kind, chunks, table=False):
    counts, rows, bounds = (I32 * 3)(), (I32 * H)(), (I32 * 8)()
    tab = (I32 * (world * H))() if table else None
    assert lib.rt_test_plan_dist(H, world, rank, mode, kind, chunks, counts, rows, bounds, tab, world * H) == 0
    n, m, nb = counts
    return (list(rows[:n]), m, [(bounds[2 * k], bounds[2 * k + 1]) for k in range(nb)],
            list(tab[:world * m]) if table else None)


DIST_CASES = [
    (2160, 8, STD, 4, 0), (4320, 8, PAPER, 2, 0), (2160, 3, STD, 4, 0), (4320, 3, PAPER, 2, 0),
    (2160, 8, STD, 4, 1), (4320, 8, PAPER, 2, 1),   # RGB8 output: the root sheds nothing
    (17, 4, STD, 4, 0), (17, 4, PAPER, 2, 0), (5, 8, STD, 4, 0), (5, 8, PAPER, 2, 0), (1, 1, STD, 4, 0),
    (1, 1, PAPER, 2, 0),
]


@pytest.mark.parametrize("H,world,mode,chunks,kind", DIST_CASES)
def test_dist_plan(lib, H, world, mode, chunks, kind):
    S = frame_dist.strip_for(mode)
    plans = [_dist(lib, H, world, r, mode, kind, chunks, table=(r == 0)) for r in range(world)]
    _, m, bounds, tab = plans[0]
    assert m == max(len(p[0]) for p in plans) and all(p[1] == m and p[2] == bounds for p in plans)
    # the ranks' rows partition the frame (a rank may own none: a valid, empty plan)
    assert sorted(r for p in plans for r in p[0]) == list(range(H))
    if H < world:
        assert any(p[0] == [] for p in plans)
    # the placement table: a permutation of the rows, each at its slot
    assert len(tab) == world * m
    assert sorted(v for v in tab if v >= 0) == list(range(H))
    for a, b in bounds:
        for r in range(world):
            rows = plans[r][0]
            for i in range(a, b):
                assert tab[world * a + r * (b - a) + (i - a)] == (rows[i] if i < len(rows) else -1)
    # chunks: contiguous over [0, m), whole strips, sizes 4:3:2:1 (n : n-1 : ... : 1) to within one strip
    assert bounds[0][0] == 0 and bounds[-1][1] == m
    assert all(bounds[k][1] == bounds[k + 1][0] for k in range(len(bounds) - 1))
    assert all(a % S == 0 for a, _ in bounds) and all(b % S == 0 for _, b in bounds[:-1])
    units = (m + S - 1) // S
    n = min(chunks, units)
    assert len(bounds) == n
    wsum = n * (n + 1) // 2
    for k, (a, b) in enumerate(bounds):
        assert abs((b - a + S - 1) // S - units * (n - k) / wsum) <= 1
    # the Python twin: its chunks, and (one chunk, FP64 output) its gather layout
    assert bounds == frame_dist.chunk_bounds(m, chunks, S)
    if kind == 0:
        assert _dist(lib, H, world, 0, mode, 0, 1, table=True)[3] == frame_dist.gather_row_index(H, world, S)


# -------------------------------------------------------------- standard plan
@pytest.mark.parametrize("rows,n_ranges", [([4, 3, 2, 1, 0], 1), ([0, 2, 4], 3), ([2, 0, 1], 1)])
def test_std_plan(lib, rows, n_ranges):
    W, H, n = 3, 5, len(rows)
    jrow, ranges, out3 = (I32 * n)(), (I64 * (3 * n))(), (I64 * 3)()
    assert lib.rt_test_plan_std(W, H, (I32 * n)(*rows), n, jrow, ranges, out3) == 0
    ys = [H - 1 - r for r in rows]   # the reference's loop rows
    assert list(jrow) == [sorted(ys).index(y) for y in ys]
    R = [tuple(ranges[3 * i:3 * i + 3]) for i in range(out3[0])]
    assert len(R) == n_ranges
    assert all(qa < qb for qa, qb, _ in R) and all(R[i][1] <= R[i + 1][0] for i in range(len(R) - 1))
    assert sum(qb - qa for qa, qb, _ in R) == 32 * W * n
    for y, j in zip(ys, jrow):   # the row's draws land at its jitter row
        (qa, _, dst), = [g for g in R if g[0] <= 32 * W * y < g[1]]
        assert dst + (32 * W * y - qa) // 2 == j * 16 * W
    assert out3[1] == 32 * W * (max(ys) + 1) and out3[2] >= 1


# ----------------------------------------------------------------- paper plan
def _paper(lib, W, H, rows):
    n = len(rows)
    ext, shade, pos, nbr, out6 = (I32 * H)(), (I32 * H)(), (I32 * H)(), (I32 * (3 * n))(), (I64 * 6)()
    assert lib.rt_test_plan_paper(W, H, (I32 * n)(*rows), n, ext, shade, pos, nbr, out6) == 0
    n_ext = out6[0]
    return dict(ext=list(ext[:n_ext]), shade=list(shade[:n_ext]), pos=list(pos), nbr=list(nbr), n_ext=n_ext,
                isect=out6[1], aux_ints=out6[2], list_cap=out6[3], gtime_words=out6[4], wpg=out6[5])


def _calls(lib, W, H, rows, calls, n_ext, rollback_after=-1):
    n, k = len(rows), len(calls)
    flat = (I32 * (3 * k))(*[v for c in calls for v in c])
    out, lists, done = (I32 * (4 * k))(), (I32 * (24 * n_ext))(), (I32 * n_ext)()
    assert lib.rt_test_plan_paper_calls(W, H, (I32 * n)(*rows), n, flat, k, rollback_after, out, lists,
                                        24 * n_ext, done) == 0
    res, used = [], 0
    for i in range(k):
        ok, off, ln, mask = out[4 * i:4 * i + 4]
        assert ok == 1 and off == used
        res.append((list(lists[used:used + ln]), [c for c in range(k) if mask >> c & 1]))
        used += ln
    return res, list(done)


def _check_lists(plan, lists):
    seen = [e for L in lists for e in L if e >= 0]
    assert sorted(seen) == list(range(plan["n_ext"]))   # every ext index in exactly one call's list
    for L in lists:
        assert len(L) % 16 == 0
        for i, e in enumerate(L):   # a run of consecutive rows starts on a wave (8-entry) boundary
            run_start = e >= 0 and (i == 0 or L[i - 1] < 0 or plan["ext"][L[i - 1]] + 1 != plan["ext"][e])
            assert not run_start or i % 8 == 0
    assert sum(len(L) for L in lists) <= 24 * plan["n_ext"] == plan["list_cap"]


@pytest.mark.parametrize("H", [1, 2, 31])
def test_paper_plan_whole_frames(lib, H):
    W, rows = 17, list(range(H))
    p = _paper(lib, W, H, rows)
    assert p["ext"] == rows and p["shade"] == [1] * H and p["pos"] == rows
    assert p["nbr"] == [v for r in rows for v in (r - 1 if r > 0 else -1, r, r + 1 if r + 1 < H else -1)]
    assert p["wpg"] == 4 and p["gtime_words"] == 3 * H * 4 * 2 and p["aux_ints"] == 2 * H + 4 * H + 24 * H
    calls_sets = [[(0, H, 1)]] + ([[(0, 30, 1), (30, 31, 2)]] if H == 31 else [])
    for calls in calls_sets:
        res, done = _calls(lib, W, H, rows, calls, p["n_ext"])
        _check_lists(p, [L for L, _ in res])
        assert all(done)


def test_paper_plan_split_rows_and_second_call(lib):
    H = 70
    rows = list(range(30)) + list(range(60, 70))
    p = _paper(lib, 5, H, rows)
    assert p["ext"] == list(range(31)) + list(range(59, 70))
    assert p["shade"] == [1] * 30 + [0, 0] + [1] * 10
    res, _ = _calls(lib, 5, H, rows, [(0, len(rows), 1)], p["n_ext"])
    _check_lists(p, [res[0][0]])
    # rows 0..59 in two calls: the second computes what the first left, and
    # waits for the first's primary hits (row 29 and 30) only across streams
    rows = list(range(60))
    p = _paper(lib, 5, H, rows)
    assert p["ext"] == list(range(61))
    for streams, waits in (((1, 2), [0]), ((1, 1), [])):
        res, done = _calls(lib, 5, H, rows, [(0, 30, streams[0]), (30, 60, streams[1])], p["n_ext"])
        _check_lists(p, [L for L, _ in res])
        assert [p["ext"][e] for e in res[0][0] if e >= 0] == list(range(31))
        assert [p["ext"][e] for e in res[1][0] if e >= 0] == list(range(31, 61))
        assert res[0][1] == [] and res[1][1] == waits
        assert done == [1] * 31 + [2] * 30
    _, first_only = _calls(lib, 5, H, rows, [(0, 30, 1)], p["n_ext"])
    _, rolled_back = _calls(lib, 5, H, rows, [(0, 30, 1), (30, 60, 2)], p["n_ext"], rollback_after=1)
    assert rolled_back == first_only == [1] * 31 + [0] * 30


@pytest.mark.parametrize("W", [1, 5])
def test_paper_plan_logical_intersects(lib, W):
    """Per pixel: trace_paper's ray, the centre probe and one probe per
    neighbour inside the frame (tracer.cpp:133-178, 258-281)."""
    H, rows = 7, [0, 1, 3, 6]
    want = sum(2 + (x > 0) + (x + 1 < W) + (r > 0) + (r + 1 < H) for r in rows for x in range(W))
    assert _paper(lib, W, H, rows)["isect"] == want


# ------------------------------------------------------------- kernel variant
FLAGS = {"NONE": 0, "COUNT_OPS": 1, "NO_CULL": 2, "FP32": 4, "NO_BVH": 8}


def _scene_text(name):
    kind, _, which = name.partition("/")
    if kind.startswith("config"):
        return scenes.config_json(int(kind[6:]), dpi=24)[0]
    return json.dumps({"torture": scenes.torture_scenes(dpi=12), "bvh": scenes.bvh_scenes(16),
                       "deep": scenes.deep_scenes()}[kind][which])


def _kernel_name(rt, lib, text, mode, flags):
    sc = rt.load_scene_from_json_text(text)
    buf = C.create_string_buffer(160)
    return lib.rt_test_kernel_name(sc.handle, mode, flags, buf, 160), buf.value.decode()


def test_kernel_names_match_the_recorded_ones(rt, lib):
    """tests/golden/kernel_names.json: the names rt_test_kernel_name gave before
    the kernel choice moved into pick_variant + the dispatch tables (what
    rocprofv3 prints, and bench.py's `kernel` field)."""
    with open(os.path.join(GOLDEN, "kernel_names.json")) as f:
        cases = json.load(f)
    assert len(cases) == 108
    texts = {}
    for c in cases:
        text = texts.setdefault(c["scene"], _scene_text(c["scene"]))
        assert _kernel_name(rt, lib, text, c["mode"], FLAGS[c["flags"]]) == (0, c["kernel"]), c


@pytest.mark.parametrize("mode", [STD, PAPER])
def test_kernel_name_refuses_what_a_frame_refuses(rt, lib, mode):
    """A big-stack scene has no FP32 kernel: the frame is refused
    (tests/test_gpu_deep.py), and so is the question which kernel it runs."""
    rc, _ = _kernel_name(rt, lib, _scene_text("deep/csg_right12"), mode, FLAGS["FP32"])
    assert rc == RT_ERR_UNSUPPORTED
    assert "FP32" in rt.last_error()
