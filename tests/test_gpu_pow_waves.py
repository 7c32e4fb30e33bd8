"""pow_spec (rt_device.hpp) by wave composition.  Its powering loop runs to
the largest exponent among the lanes of a wave, and any scheme that moves the
loop's control to the scalar unit (tried and rejected so far, DESIGN.md
§Measured) depends on which exponents share a wave.  These cases choose that
(rt_test_pow_spec: 256-thread blocks in input order, so 64 consecutive
elements form a wave) and check every lane against the exact power, never
against another call of the code under test.

Integer k in [0, 1023]: the correctly rounded x^k, float(Fraction(x) ** k),
wherever that is >= 2^-1000 (below: a value in [0, 2^-999]); k == 0 gives
exactly 1.0 for every x, NaN included.  Other exponents are the device
library's pow (pow_general): within 1e-12 relative of a 60-digit power, with
pow(0, y > 0) = 0 and pow(1, y) = 1 exactly (include/rt_test.h)."""
from fractions import Fraction

import numpy as np
import pytest

N = 197                  # three full waves and a partial one of 5 lanes
TINY = 2.0 ** -1000
OTHER_Y = (0.5, 12.5, 1023.5, 1024.0, 2000.0)   # pow_general: non-integer or out of range


def _xs(seed):
    """N inputs >= 0 where rdotv lives, the special values spread over the
    waves (the partial wave included)."""
    rng = np.random.default_rng(seed)
    j = 1 + np.arange(N) % 30
    x = np.where(np.arange(N) % 2 == 0, rng.random(N), 1.0 - rng.random(N) * 2.0 ** -j)
    special = [0.0, 1.0, 1.0 - 2.0 ** -53, 1.0 - 2.0 ** -30, 1.0 + 2.0 ** -52, 2.0 ** -1074, 5e-310, np.nan, 0.5]
    at = rng.permutation(N - 5)[:3 * len(special)]
    for i, p in enumerate(at):
        x[p] = special[i % len(special)]
    x[N - 5:] = [np.nan, 0.0, 1.0 - 2.0 ** -53, 2.0 ** -1074, 0.75]   # the partial wave
    return x


def _check(gpu, x, y):
    import mpmath

    mpmath.mp.dps = 60
    got = gpu.pow_spec(x, y)
    bad = []
    for i in range(len(x)):
        xi, yi, g = float(x[i]), float(y[i]), float(got[i])
        integer = 0.0 <= yi < 1024.0 and yi == int(yi)
        if integer and yi == 0.0:
            ok = g == 1.0
        elif np.isnan(xi):
            ok = np.isnan(g)
        elif integer:
            want = float(Fraction(xi) ** int(yi))
            ok = (g == want) if want >= TINY else (0.0 <= g <= 2.0 ** -999)
        elif xi == 0.0:
            ok = g == 0.0
        elif xi == 1.0:
            ok = g == 1.0
        else:
            exact = mpmath.power(mpmath.mpf(xi), mpmath.mpf(yi))
            if exact >= TINY:
                ok = g > 0.0 and abs(mpmath.mpf(g) - exact) / exact <= 1e-12
            else:
                ok = 0.0 <= g <= 2.0 ** -999
        if not ok:
            bad.append((i, xi, yi, g))
    print(f"  {len(x)} lanes, {len(bad)} wrong")
    assert not bad, bad[:8]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 2, 3, 4, 5, 20, 24, 32, 1023])
def test_one_exponent_per_wave(gpu, k):
    _check(gpu, _xs(k), np.full(N, float(k)))


@pytest.mark.gpu
@pytest.mark.parametrize("ks", [(4, 32), (1, 1023), (0, 5), (3, 20, 24), (0, 1, 2), (6, 7, 1000)])
def test_alternating_exponents(gpu, ks):
    """Lanes alternate 2 or 3 distinct exponents."""
    y = np.array([float(ks[i % len(ks)]) for i in range(N)])
    _check(gpu, _xs(100 + sum(ks)), y)


@pytest.mark.gpu
def test_block_halves_and_single_odd_lane(gpu):
    """Exponents split a wave into halves, and one lane differs from 63 others."""
    y = np.full(N, 8.0)
    y[32:64] = 10.0
    y[64 + 17] = 33.0
    y[128:160] = 0.0
    y[N - 1] = 3.0
    _check(gpu, _xs(7), y)


@pytest.mark.gpu
def test_sixty_four_distinct_exponents(gpu):
    rng = np.random.default_rng(5)
    y = np.empty(N)
    for w in range(0, N, 64):
        ks = np.concatenate([[0, 1, 1023], 2 + rng.permutation(1021)[:61]])
        assert len(set(ks)) == 64
        ks = rng.permutation(ks)
        y[w:w + 64] = ks[:min(64, N - w)]
    _check(gpu, _xs(11), y)


@pytest.mark.gpu
@pytest.mark.parametrize("ks", [(4,), (0, 32), (1, 5, 1023)])
def test_integer_and_other_exponents_mixed(gpu, ks):
    """pow_general lanes take the out-of-line call; the integer lanes around
    them still get their own exponent's power."""
    rng = np.random.default_rng(13 + len(ks))
    y = np.array([float(ks[i % len(ks)]) for i in range(N)])
    other = rng.random(N) < 0.4
    other[N - 5], other[N - 4] = True, False
    y[other] = rng.choice(OTHER_Y, int(other.sum()))
    _check(gpu, _xs(17), y)
