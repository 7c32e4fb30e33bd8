"""The jitter cache's host-only logic (csrc/host/jitter_cache.hpp): which
buffer a standard frame's draws live in, by (W, rows) - whole-key compare,
valid only after the filling frame has ended, least-recently-used eviction
under a byte budget, the uncached buffer for frames beyond it, and allocation
failures.  Driven over host memory through rt_test_jitter_cache_sim (no device
is touched); the simulation also checks that a buffer a frame neither fills
nor uploads to still holds that frame's own draws and rows."""
import pytest

FRAME, ABANDON, CLEAR, FAIL_NEXT, BUDGET, RELEASE = range(6)
W = 2


def entry_bytes(n_rows, w=W):
    """The draws (16 doubles per pixel) padded to 256 B, then rows | jitter rows."""
    jit = n_rows * 16 * w * 8
    return (jit + 255) // 256 * 256 + 2 * n_rows * 4


def frame(row0, n_rows=3, w=W, op=FRAME, h=0):
    return (op, w, row0, n_rows, h)


A, B, C_ = frame(0), frame(3), frame(6)
BIG = 1 << 20
CACHED, UNCACHED = 1, 2


@pytest.fixture(scope="module")
def sim(rt):
    rt.amd_lib()

    def run(ops, budget):
        rc, states = rt.jitter_cache_sim(ops, budget)
        assert rc == 0, rc   # 1: a resident buffer held another key's contents; 2: a leak or a double free
        assert states[-1]["live"] == 0   # every script ends with RELEASE
        return states[:-1]

    return lambda ops, budget=BIG: run(list(ops) + [(RELEASE, 0, 0, 0, 0)], budget)


def test_repeat_is_one_miss_one_hit(sim):
    s = sim([A, A, A])
    assert [(x["buffer"], x["fill"], x["upload_rows"]) for x in s] == [(CACHED, 1, 1), (CACHED, 0, 0), (CACHED, 0, 0)]
    assert (s[-1]["hits"], s[-1]["misses"], s[-1]["entries"], s[-1]["bytes"]) == (2, 1, 1, entry_bytes(3))


def test_same_byte_size_different_key(sim):
    """Equal draw bytes (3 rows of width 2, 2 rows of width 3; other rows of
    the same count): a stale hit would fit the buffer, so only the whole key
    (W and every row) may decide."""
    wide = frame(0, n_rows=2, w=3)
    assert 3 * 16 * 2 == 2 * 16 * 3
    s = sim([A, wide, B, A, wide, B])
    assert [x["fill"] for x in s] == [1, 1, 1, 0, 0, 0]
    assert s[-1]["entries"] == 3 and (s[-1]["hits"], s[-1]["misses"]) == (3, 3)
    # one row differs (the last): rows 0-2 against rows 0-1 + 3 cannot be spelled
    # by this script's consecutive rows, so rows 1-3 against 0-2 stands in
    s = sim([A, frame(1), A])
    assert [x["fill"] for x in s] == [1, 1, 0]


def test_the_same_rows_of_another_height_are_another_key(sim):
    """Output row r reads the stream at loop row H-1-r: equal W and rows, but
    other draws."""
    s = sim([frame(0, h=48), frame(0, h=56), frame(0, h=48), frame(0, h=56)])
    assert [x["fill"] for x in s] == [1, 1, 0, 0] and s[-1]["entries"] == 2
    s = sim([frame(0, h=48), frame(0, h=56), frame(0, h=56), frame(0, h=48)], budget=0)
    assert [x["upload_rows"] for x in s] == [1, 1, 0, 1]   # (the uncached buffer's rows list too)


def test_an_abandoned_frame_leaves_no_valid_entry(sim):
    s = sim([frame(0, op=ABANDON), A, A])
    assert [(x["fill"], x["upload_rows"]) for x in s] == [(1, 1), (1, 1), (0, 0)]
    assert [x["entries"] for x in s] == [1, 1, 1]   # the key's own buffer is written again
    assert (s[-1]["hits"], s[-1]["misses"]) == (1, 2)
    # a hit frame that is abandoned takes nothing away
    s = sim([A, frame(0, op=ABANDON), A])
    assert [x["fill"] for x in s] == [1, 0, 0]


def test_least_recently_used_goes_first(sim):
    s = sim([A, B, A, C_, A, B], budget=2 * entry_bytes(3))
    assert [x["fill"] for x in s] == [1, 1, 0, 1, 0, 1]   # C evicted B, not A; then B evicted C
    assert all(x["entries"] <= 2 and x["bytes"] <= 2 * entry_bytes(3) for x in s)
    assert all(x["buffer"] == CACHED for x in s)


def test_budget_of_exactly_one_entry(sim):
    small = frame(0, n_rows=2)
    s = sim([A, small, A, small, small], budget=entry_bytes(3))
    assert [x["fill"] for x in s] == [1, 1, 1, 1, 0]
    assert all(x["buffer"] == CACHED and x["entries"] == 1 and x["bytes"] <= entry_bytes(3) for x in s)
    assert s[0]["bytes"] == entry_bytes(3) and s[1]["bytes"] == entry_bytes(2)


@pytest.mark.parametrize("budget", [0, entry_bytes(3) - 1])
def test_beyond_the_budget_is_uncached(sim, budget):
    """One uncached buffer, filled every frame; only its rows list is reused
    by the next frame of the same key (as before the cache existed)."""
    s = sim([A, A, B, A], budget=budget)
    assert [(x["buffer"], x["fill"], x["upload_rows"]) for x in s] == [
        (UNCACHED, 1, 1), (UNCACHED, 1, 0), (UNCACHED, 1, 1), (UNCACHED, 1, 1)]
    assert all(x["entries"] == 0 and x["bytes"] == 0 and x["live"] == 1 for x in s)
    assert (s[-1]["hits"], s[-1]["misses"]) == (0, 4)


def test_a_frame_that_fits_does_not_evict_for_one_that_does_not(sim):
    s = sim([A, frame(0, n_rows=4), A], budget=entry_bytes(3))
    assert [(x["buffer"], x["fill"]) for x in s] == [(CACHED, 1), (UNCACHED, 1), (CACHED, 0)]


def test_shrinking_the_budget_evicts_at_the_next_miss(sim):
    s = sim([A, B, (BUDGET, 0, 0, 0, entry_bytes(3)), A, C_, C_])
    assert [x["entries"] for x in s] == [1, 2, 2, 2, 1, 1]
    assert [x["fill"] for x in (s[3], s[4], s[5])] == [0, 1, 0]


def test_entry_allocation_failure_is_not_a_frame_failure(sim):
    # the entry cannot be had: every entry is given back and the frame runs uncached
    s = sim([A, (FAIL_NEXT, 0, 0, 0, 1), B, B, A])
    assert (s[2]["buffer"], s[2]["fill"], s[2]["entries"], s[2]["live"]) == (UNCACHED, 1, 0, 1)
    assert (s[3]["buffer"], s[3]["fill"]) == (CACHED, 1)   # "once": the next frame tries the cache again
    assert (s[4]["buffer"], s[4]["fill"]) == (CACHED, 1)   # (A's entry went with the failure)
    # the uncached buffer cannot grow while entries hold memory: they go first
    s = sim([A, (FAIL_NEXT, 0, 0, 0, 1), frame(0, n_rows=4)], budget=entry_bytes(3))
    assert (s[2]["buffer"], s[2]["entries"], s[2]["live"]) == (UNCACHED, 0, 1)
    # nothing to be had at all: the frame fails (buffer 0) and nothing leaks
    s = sim([A, (FAIL_NEXT, 0, 0, 0, 3), B, B])
    assert (s[2]["buffer"], s[2]["entries"], s[2]["live"]) == (0, 0, 0)
    assert s[3]["buffer"] == UNCACHED   # (the third failure: B's entry)


def test_clear_and_release(sim):
    s = sim([A, B, (CLEAR, 0, 0, 0, 0), A, frame(0, n_rows=4, w=64), (RELEASE, 0, 0, 0, 0), A],
            budget=2 * entry_bytes(3))
    assert [x["entries"] for x in s] == [1, 2, 0, 1, 1, 0, 1]
    assert [x["live"] for x in s] == [1, 2, 0, 1, 2, 0, 1]
    assert [x["fill"] for x in (s[3], s[6])] == [1, 1]
    assert (s[-1]["hits"], s[-1]["misses"]) == (0, 5)   # the counts outlive the buffers


def test_bad_scripts_are_refused(rt):
    rt.amd_lib()
    assert rt.jitter_cache_sim([(9, 0, 0, 0, 0)], 0)[0] == rt.RT_ERR_INVALID_ARG
    assert rt.jitter_cache_sim([(FRAME, 0, 0, 3, 0)], 0)[0] == rt.RT_ERR_INVALID_ARG
    assert rt.jitter_cache_sim([A], -1)[0] == rt.RT_ERR_INVALID_ARG
