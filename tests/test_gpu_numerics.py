"""Device arithmetic helpers that must round exactly like the plain FP64
operations they replace.

div3 (rt_device.hpp) divides three numerators by one denominator with the
compiler's own v_div_scale / v_rcp / Newton / v_div_fmas / v_div_fixup
sequence, doing the reciprocal refinement once; it replaces every
normalisation (Dir3::normalized, core.h:95-101), the light direction
tl / dist (shading.cpp:81-83) and the sphere normal (p - c) / r
(geometry.cpp:30, 67-77).  It must equal `/` bit for bit on every input,
including zeros of both signs, denormals, infinities, NaN and the exponent
extremes where the scaled denominator depends on the numerator."""
import ctypes as C
import math

import numpy as np
import pytest


def _run(rt, a, b):
    lib = rt.amd_lib()
    dp = C.POINTER(C.c_double)
    lib.rt_test_div3.argtypes = [dp, dp, C.c_int, dp, dp]
    n = len(b)
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(n, 3)
    b = np.ascontiguousarray(b, dtype=np.float64)
    o3 = np.zeros((n, 3))
    op = np.zeros((n, 3))
    rc = lib.rt_test_div3(a.ctypes.data_as(dp), b.ctypes.data_as(dp), n, o3.ctypes.data_as(dp), op.ctypes.data_as(dp))
    assert rc == 0
    return o3, op


@pytest.mark.gpu
def test_div3_bit_identical_to_division(gpu):
    rng = np.random.default_rng(11)
    n = 1 << 20
    # geometry-like values: unit-ish vectors, distances, radii
    a = rng.normal(size=(n, 3)) * np.exp(rng.uniform(-20, 20, size=(n, 1)))
    b = np.abs(rng.normal(size=n)) * np.exp(rng.uniform(-20, 20, size=n)) + 1e-12
    o3, op = _run(gpu, a, b)
    assert np.array_equal(o3.view(np.uint64), op.view(np.uint64))


@pytest.mark.gpu
def test_div3_edge_values(gpu):
    specials = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 1e-300, 1e-310, 1.0, -1.0,
                         1e300, 1.7976931348623157e308, np.inf, -np.inf, np.nan, 3.0, 1e-17, 2.0 ** -969,
                         2.0 ** -970, 2.0 ** 1023], dtype=np.float64)
    rng = np.random.default_rng(5)
    n = 64 * 2048
    a = rng.choice(specials, size=(n, 3))
    b = rng.choice(specials, size=n)
    # one wave in four gets ordinary values mixed with extremes in the same wave
    a[::4] = rng.normal(size=(len(a[::4]), 3))
    o3, op = _run(gpu, a, b)
    assert np.array_equal(o3.view(np.uint64), op.view(np.uint64))


# ---------------------------------------------------------------- pow_spec
# pow_spec (rt_device.hpp) is std::pow(rdotv, shininess) of the specular term
# (shading.cpp:124).  Its claim for integer exponents 0..1023 is "the correctly
# rounded x^k" (an unnormalised double-double by binary powering), so the
# reference here is the exact power, rounded once to nearest-even with integer
# arithmetic; every other exponent goes to the device library's pow
# (pow_general), checked against a 60-digit mpmath power.  These guard the
# compiled code (fma contraction, reassociation, a later "optimisation").
POW_INT_K = (1, 2, 3, 4, 5, 6, 7, 8, 16, 20, 24, 32, 64, 80, 127, 128, 255, 256, 511, 512, 1000, 1023)
POW_OTHER_Y = (0.5, 1e-3, 12.5, 1023.5, 1024.0, 2000.0, -2.0)
POW_SPECIAL_X = (0.0, 1.0, 2.0 ** -1074, 1.0 - 2.0 ** -53, 0.5)
TINY = 2.0 ** -1000      # the code's claim holds from here up; below, the term is 0 to any tolerance


def _exact_pow(x: float, k: int):
    """(the correctly rounded x^k, the distance of the exact x^k from the
    nearest midpoint between adjacent doubles, in ulp) for a double x >= 0 and
    an integer k >= 1, in exact integer arithmetic."""
    if x == 0.0:
        return 0.0, 0.5
    m, e = math.frexp(x)
    m, e = int(m * 2 ** 53), e - 53          # x = m * 2^e exactly
    N, E = m ** k, e * k
    shift = N.bit_length() - 53
    if shift <= 0:
        return math.ldexp(N, E), 0.5
    q, rem, half = N >> shift, N & ((1 << shift) - 1), 1 << (shift - 1)
    mid = abs(rem - half) / (1 << shift)
    if rem > half or (rem == half and (q & 1)):
        q += 1
    try:
        return math.ldexp(q, shift + E), mid
    except OverflowError:
        return math.inf, mid


def _pow_x_families(rng, n):
    """n values in [0, 1] and n of the form 1 - u * 2^-j (j = 1..30), where rdotv lives."""
    j = 1 + np.arange(n) % 30
    return rng.random(n), 1.0 - rng.random(n) * 2.0 ** -j


_pow_cases = {}


def _pow_int_cases():
    """(x, k, exact) of the integer-exponent cases, built once."""
    if "int" not in _pow_cases:
        rng = np.random.default_rng(2024)
        xs, ks, exact = [], [], []
        for k in POW_INT_K:
            a, b = _pow_x_families(rng, 256)
            pa, pb = _pow_x_families(rng, 1000)
            pool = np.concatenate([pa, pb])
            near = sorted((_exact_pow(float(x), k)[1], float(x)) for x in pool)[:64]
            case = list(a) + list(b) + [x for _, x in near] + list(POW_SPECIAL_X)
            if k == 2:   # exact ties: (2^27 - m)^2 is an odd 54-bit integer, so x^2 needs round-to-even
                m = 2 * rng.integers(0, 2 ** 24, 256) + 1
                ties = 1.0 - m * 2.0 ** -27
                assert all(_exact_pow(float(x), 2)[1] == 0.0 for x in ties)
                case += list(ties)
            for x in case:
                xs.append(float(x))
                ks.append(float(k))
                exact.append(_exact_pow(float(x), k)[0])
        _pow_cases["int"] = (np.array(xs), np.array(ks), np.array(exact))
    return _pow_cases["int"]


def _pow_other_cases():
    """(x, y, exact as mpmath numbers) of the non-integer / out-of-range exponents."""
    if "other" not in _pow_cases:
        import mpmath

        mpmath.mp.dps = 60
        rng = np.random.default_rng(77)
        xs, ys, exact = [], [], []
        for y in POW_OTHER_Y:
            a, b = _pow_x_families(rng, 256)
            for x in list(a) + list(b) + list(POW_SPECIAL_X):
                x = float(x)
                xs.append(x)
                ys.append(y)
                if x == 0.0:
                    exact.append(mpmath.inf if y < 0 else mpmath.mpf(0))
                else:
                    exact.append(mpmath.power(mpmath.mpf(x), mpmath.mpf(y)))
        _pow_cases["other"] = (np.array(xs), np.array(ys), exact)
    return _pow_cases["other"]


def test_exact_pow_reference_is_the_rounded_fraction():
    """The integer rounding above against float(Fraction(x) ** k) (CPython
    rounds an int / int quotient correctly)."""
    from fractions import Fraction

    rng = np.random.default_rng(3)
    for k in (1, 2, 3, 7, 64, 255, 1023):
        for x in list(1.0 - rng.random(20) * 2.0 ** -(1 + np.arange(20))) + list(rng.random(10)) + [0.5, 1.0]:
            want = float(Fraction(float(x)) ** k)
            if want >= 2.0 ** -1022:
                assert _exact_pow(float(x), k)[0] == want, (x, k)
    assert _exact_pow(1.0 - 3 * 2.0 ** -27, 2) == ((1.0 - 3 * 2.0 ** -27) ** 2, 0.0)   # a tie, to even


@pytest.mark.gpu
def test_pow_spec_integer_exponents_correctly_rounded(gpu):
    x, k, exact = _pow_int_cases()
    # integer and non-integer exponents share waves: the out-of-line pow_general sits under a divergent branch
    xo, yo, _ = _pow_other_cases()
    n = min(len(x), len(xo))
    mix_x, mix_y = np.empty(len(x) + n), np.empty(len(x) + n)
    sel = np.ones(len(mix_x), dtype=bool)
    sel[1:2 * n:2] = False
    mix_x[sel], mix_y[sel] = x, k
    mix_x[~sel], mix_y[~sel] = xo[:n], yo[:n]
    got = gpu.pow_spec(mix_x, mix_y)[sel]
    alone = gpu.pow_spec(x, k)
    assert np.array_equal(got.view(np.uint64), alone.view(np.uint64)), "result depends on the lane's neighbours"
    big = exact >= TINY
    bad = np.flatnonzero(big & (got != exact))
    print(f"  {len(x)} integer cases, {int(big.sum())} with x^k >= 2^-1000, {len(bad)} not correctly rounded")
    assert len(bad) == 0, [(x[i].hex(), int(k[i]), got[i].hex(), exact[i].hex()) for i in bad[:8]]
    small = got[~big]
    assert np.all((small >= 0.0) & (small <= 2.0 ** -999))


@pytest.mark.gpu
def test_pow_spec_exponent_zero_is_one(gpu):
    x = np.array([0.0, -0.0, 1.0, 0.5, 2.0 ** -1074, 1.0 - 2.0 ** -53, np.nan, np.inf, 3.0] * 16)
    got = gpu.pow_spec(x, np.zeros(len(x)))
    assert np.array_equal(got, np.ones(len(x)))


@pytest.mark.gpu
def test_pow_spec_other_exponents_against_mpmath(gpu):
    """Bar: relative error <= 1e-12 wherever the exact power is a normal
    number >= 2^-1000.  Derived, not measured: the term reaches a pixel
    multiplied by ks * I_L, below 1e3 in any scene here, so 1e-12 keeps it seven
    orders under the 1e-5 frame bar.  Below 2^-1000 (x^2000 of most x) a
    relative bar has no meaning: the result must lie in [0, 2^-999]; a power
    beyond the largest double (2^-1074 to the -2) must be +inf."""
    import mpmath

    x, y, exact = _pow_other_cases()
    got = gpu.pow_spec(x, y)
    worst_rel, worst_ulp, worst_at = 0.0, 0.0, None
    for i in range(len(x)):
        g, e = float(got[i]), exact[i]
        if x[i] == 0.0:
            assert g == (math.inf if y[i] < 0 else 0.0) and not math.copysign(1.0, g) < 0, (x[i], y[i], g)
        elif x[i] == 1.0:
            assert g == 1.0, (y[i], g)
        elif e >= mpmath.mpf(2) ** 1024:
            assert g == math.inf, (x[i], y[i], g)
        elif e < TINY:
            assert 0.0 <= g <= 2.0 ** -999, (x[i], y[i], g)
        else:
            err = abs(mpmath.mpf(g) - e)
            rel = float(err / e)
            ulp = float(err / mpmath.mpf(math.ulp(float(e))))
            if ulp > worst_ulp:
                worst_rel, worst_ulp, worst_at = rel, ulp, (x[i].hex(), y[i])
            assert rel <= 1e-12, (x[i].hex(), y[i], g.hex(), rel)
    print(f"  pow_general: {len(x)} cases, largest error {worst_ulp:.3f} ulp (relative {worst_rel:.3g}) at {worst_at}")
