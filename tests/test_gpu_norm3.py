"""norm3 (rt_device.hpp): |v| and v / |v| with the square root's refinement
shared by the three divisions.  It replaces `__builtin_sqrt` + div3 in every
normalisation and in shade()'s light direction, so it must equal sqrt and `/`
bit for bit.  The fused path runs only when every active lane of the wave has
2^-600 <= s <= 2^600 and every |v_k| >= 2^-600; otherwise the whole wave takes
sqrt + div3.  rt_test_norm3 (include/rt_test.h) runs one lane per vector in
256-thread blocks in input order, so 64 consecutive vectors form a wave; it
returns norm3's (L, q), the plain operations' (L, q) from the same kernel and
whether the lane's wave took the fused path.  The in-range cases require
fast == 1, so they cannot pass through the fallback; the references are the
plain operations on the device and numpy's on the host, never another call of
the code under test."""
import ctypes as C

import numpy as np
import pytest


def _norm3(rt, v, n=None):
    lib = rt.amd_lib()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    lib.rt_test_norm3.argtypes = [dp, C.c_int, dp, dp, dp, dp, ip]
    v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1, 3)
    n = len(v) if n is None else n
    L, pL = np.zeros(n), np.zeros(n)
    q, pq = np.zeros((n, 3)), np.zeros((n, 3))
    fast = np.full(n, -1, dtype=np.int32)
    rc = lib.rt_test_norm3(v.ctypes.data_as(dp), n, L.ctypes.data_as(dp), q.ctypes.data_as(dp), pL.ctypes.data_as(dp),
                           pq.ctypes.data_as(dp), fast.ctypes.data_as(ip))
    assert rc == 0
    return L, q, pL, pq, fast


def _normalized(rt, v):
    lib = rt.amd_lib()
    dp = C.POINTER(C.c_double)
    lib.rt_test_normalized.argtypes = [dp, C.c_int, dp]
    v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1, 3)
    out = np.zeros((len(v), 3))
    assert lib.rt_test_normalized(v.ctypes.data_as(dp), len(v), out.ctypes.data_as(dp)) == 0
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b):
    """Bit-equal, NaN matching NaN."""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (_bits(a) == _bits(b))))


def _host(v):
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        L = np.sqrt((x * x + y * y) + z * z)
        return L, v / L[:, None]


def _directions(rng, n):
    return rng.normal(size=(n, 3)) * 2.0 ** rng.integers(-250, 251, size=(n, 1))


def _in_range(rng, n):
    """n of each family of the fused path's domain, plus its corners."""
    dirs = _directions(rng, n)
    unit = rng.normal(size=(n, 3))
    unit = _host(unit)[1]                       # L within an ulp of 1
    skew = rng.uniform(0.25, 1.0, size=(n, 3)) * rng.choice([-1.0, 1.0], size=(n, 3))
    skew[np.arange(n), rng.integers(0, 3, n)] *= 2.0 ** -500
    corners = np.array([[1.0, 2.0, 3.0]]) * np.array([[2.0 ** -299], [2.0 ** 298]])
    corners = np.concatenate([corners, [[2.0 ** -600, 1.0, -1.0], [-1.0, 2.0 ** -600, 0.5], [2.0 ** -300, 2.0 ** -600, 2.0 ** -600],
                                        [2.0 ** 299, 2.0 ** 299, 2.0 ** 299]]])
    return np.concatenate([dirs, unit, skew, corners])


@pytest.mark.gpu
def test_in_range_vectors_take_the_fused_path_and_match_bit_for_bit(gpu):
    rng = np.random.default_rng(310)
    v = _in_range(rng, 100_000)
    L, q, pL, pq, fast = _norm3(gpu, v)
    assert np.all(fast == 1), f"{int((fast != 1).sum())} lanes went through the fallback"
    badL, badq = int((_bits(L) != _bits(pL)).sum()), int((_bits(q) != _bits(pq)).sum())
    hL, hq = _host(v)
    hbadL, hbadq = int((_bits(L) != _bits(hL)).sum()), int((_bits(q) != _bits(hq)).sum())
    print(f"  {len(v)} vectors: L / q differing from the device's sqrt and '/': {badL} / {badq}, from numpy's: {hbadL} / {hbadq}")
    assert badL == 0 and badq == 0
    assert hbadL == 0 and hbadq == 0
    # normalized(): the same quotients above kEPS = 1e-6, (0, 1, 0) at or below
    u = _normalized(gpu, v)
    want = np.where((hL > 1e-6)[:, None], hq, np.array([0.0, 1.0, 0.0]))
    assert int((hL <= 1e-6).sum()) > 1000 and np.array_equal(_bits(u), _bits(want))


BIG, TINY = 2.0 ** 300, 2.0 ** -303
OUT_OF_RANGE = {
    "s_below": (TINY, 2 * TINY, 3 * TINY),            # s = 14 * 2^-606
    "s_above": (BIG, 2 * BIG, 3 * BIG),               # s = 14 * 2^600
    "s_just_above": (2.0 ** 300, 2.0 ** 290, 2.0 ** 290),   # s = 2^600 (1 + 2^-19)
    "s_overflows": (2.0 ** 600, 2.0 ** 600, -2.0 ** 600),
    "component_below": (2.0 ** -601, 1.0, 1.0),
    "denormal_min": (5e-324, 1.0, -2.0),
    "denormal": (0.5, -1e-310, 2.0),
    "all_denormal": (3e-310, 1e-310, 2e-310),
    "zero": (0.0, 1.0, 2.0),
    "minus_zero": (1.0, -0.0, 2.0),
    "two_zeros": (0.0, -0.0, -3.0),
    "inf": (np.inf, 1.0, 1.0),
    "minus_inf": (1.0, 1.0, -np.inf),
    "nan": (1.0, np.nan, 1.0),
    "zero_vector": (0.0, 0.0, 0.0),
    "minus_zero_vector": (-0.0, 0.0, -0.0),
}


def _fused_domain(v):
    """The fused path's condition on one lane (rt_device.hpp sqrt_div3)."""
    lo, hi = 2.0 ** -600, 2.0 ** 600
    with np.errstate(all="ignore"):
        s = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        return (s >= lo) & (s <= hi) & np.all(np.abs(v) >= lo, axis=1)


def test_case_tables_lie_on_the_intended_side_of_the_range():
    assert np.all(_fused_domain(_in_range(np.random.default_rng(310), 1000)))
    for name, bad in OUT_OF_RANGE.items():
        assert not _fused_domain(np.array([bad]))[0], name


@pytest.mark.gpu
def test_out_of_range_lanes_send_their_whole_wave_to_sqrt_and_div3(gpu):
    """Per case two waves: 64 copies of the vector, and one copy among 63
    in-range directions; a third, all in range, shows that the next wave is
    not affected."""
    rng = np.random.default_rng(600)
    blocks, names = [], list(OUT_OF_RANGE)
    for i, name in enumerate(names):
        bad = np.array(OUT_OF_RANGE[name])
        mixed = _directions(rng, 64)
        mixed[(7 * i + 3) % 64] = bad
        blocks += [np.tile(bad, (64, 1)), mixed, _directions(rng, 64)]
    v = np.concatenate(blocks)
    L, q, pL, pq, fast = _norm3(gpu, v)
    fast = fast.reshape(len(names), 3, 64)
    for i, name in enumerate(names):
        assert np.all(fast[i, :2] == 0), f"{name}: the fused path ran"
        assert np.all(fast[i, 2] == 1), f"{name}: the in-range wave after it fell back"
    assert _same(L, pL) and _same(q, pq)
    hL, hq = _host(v)
    assert _same(L, hL) and _same(q, hq)
    u = _normalized(gpu, v).reshape(len(names), 3, 64, 3)
    want = np.where((hL > 1e-6)[:, None], hq, np.array([0.0, 1.0, 0.0])).reshape(u.shape)
    assert _same(u, want)
    for name in ("zero_vector", "minus_zero_vector", "all_denormal"):
        assert np.array_equal(_bits(u[names.index(name), 0]), _bits(np.tile([0.0, 1.0, 0.0], (64, 1)))), name


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 64 * 3 + 1])
def test_partial_last_wave(gpu, n):
    """Lanes past n are not launched: out-of-range values in the slots of the
    input behind them do not force the fallback."""
    rng = np.random.default_rng(n)
    v = np.full((n + 63, 3), np.nan)
    v[n:n + 8] = 0.0
    v[:n] = _directions(rng, n)
    L, q, pL, pq, fast = _norm3(gpu, v, n)
    assert np.all(fast == 1)
    hL, hq = _host(v[:n])
    assert np.array_equal(_bits(L), _bits(pL)) and np.array_equal(_bits(q), _bits(pq))
    assert np.array_equal(_bits(L), _bits(hL)) and np.array_equal(_bits(q), _bits(hq))
