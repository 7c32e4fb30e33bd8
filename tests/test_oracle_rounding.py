"""The oracle whose specular power is the device's (oracle_set_pow(1),
rtamd.oracle_pow) and the oracle's own shading of caller-given hits
(oracle_shade_hits), on the CPU: what tests/test_gpu_rounding.py holds the FP64
kernels to bit for bit.

Mode 0 is the reference: libm pow, every fixture under tests/golden.  Mode 1
answers the two pow(rdotv, shininess) calls of shade() with the correctly
rounded x^k wherever the device takes pow_spec (rt_device.hpp: an integer
exponent in [0, 1024), and in the shading queries also |x| <= 2) and with libm
everywhere else.  The power is binary powering in __float128 rounded once, not
the device's double-double: the two are held to the exact integer power
(test_gpu_numerics._exact_pow) separately, here and in
test_gpu_numerics.test_pow_spec_integer_exponents_correctly_rounded.

Nothing computed under mode 1 enters a cache of another test module: this file
keeps its own, and every `with rt.oracle_pow(1)` block restores mode 0."""
import json

import numpy as np
import pytest

import scenes
from test_gpu_numerics import POW_OTHER_Y, TINY, _pow_int_cases, _pow_x_families
from test_gpu_parity import SMALL
from test_gpu_query import SCENES
from test_shade_plan import BAR, OVERRIDES, SHADING, shade_ref

SHADING_DPI = 16


def pow_spec_takes(y: float) -> bool:
    """pow_spec's condition on the exponent (rt_device.hpp): an integer in [0, 1024)."""
    return bool(0.0 <= y < 1024.0 and float(int(y)) == y)


def integer_exponents(sc) -> bool:
    """Every material of the loaded scene has an exponent pow_spec takes."""
    d = sc.desc
    return all(pow_spec_takes(d.materials[i].shininess) for i in range(d.n_materials))


def shading_scene_names(integer: bool) -> list:
    """scenes.shading_scenes() names whose exponents all are (integer) / are not all in pow_spec's range."""
    out = []
    for name, s in scenes.shading_scenes(dpi=SHADING_DPI).items():
        ys = [float(o["sphere"]["color"].get("shininess", 1.0)) for o in s["objects"]
              if "sphere" in o and "color" in o["sphere"]]
        if all(pow_spec_takes(y) for y in ys) == integer:
            out.append(name)
    return sorted(out)


def test_the_split_of_the_shading_scenes():
    odd = shading_scene_names(False)
    assert odd == sorted(n for n in scenes.shading_scenes(dpi=SHADING_DPI) if n.startswith("exponents_"))
    assert len(shading_scene_names(True)) >= 30


# --------------------------------------------------------- 1. the power itself
def test_mode1_power_is_the_correctly_rounded_integer_power(rt):
    x, k, exact = _pow_int_cases()
    libm = rt.oracle_spec_pow(x, k)
    with rt.oracle_pow(1):
        got = rt.oracle_spec_pow(x, k)
        got_any = rt.oracle_spec_pow(x, k, any_x=True)
    assert rt.oracle_lib().oracle_get_pow() == 0
    assert np.array_equal(libm, np.array([pow(float(a), float(b)) for a, b in zip(x, k)]))   # mode 0 is libm
    big = exact >= TINY
    bad = np.flatnonzero(big & (got != exact))
    print(f"  {len(x)} integer cases, {int(big.sum())} with x^k >= 2^-1000: {len(bad)} not correctly rounded; "
          f"{int((~big & (got != exact)).sum())} differ below 2^-1000; libm differs from exact on "
          f"{int((libm != exact).sum())}")
    assert len(x) > 13000
    assert len(bad) == 0, [(x[i].hex(), int(k[i]), got[i].hex(), exact[i].hex()) for i in bad[:8]]
    small = got[~big]
    assert np.all((small >= 0.0) & (small <= 2.0 ** -999))
    assert np.array_equal(got.view(np.uint64), got_any.view(np.uint64))   # |x| <= 1 here: the same branch


def test_mode1_power_is_libm_outside_the_condition(rt):
    rng = np.random.default_rng(41)
    xs, ys = [], []
    for y in POW_OTHER_Y + (1024.0, 1025.0, -1.0, 3.5, 1e300, float("inf"), float("nan")):
        a, b = _pow_x_families(rng, 64)
        for v in list(a) + list(b) + [0.0, 1.0, 0.5]:
            xs.append(float(v))
            ys.append(float(y))
    x, y = np.array(xs), np.array(ys)
    libm = rt.oracle_spec_pow(x, y)
    with rt.oracle_pow(1):
        got = rt.oracle_spec_pow(x, y)
        # the shading queries' condition: beyond |x| = 2 an integer exponent is libm's too
        bx = np.array([2.0, 2.0000000000000004, 3.0, 10.0, 1e200, np.inf, np.nan, -3.0] * 4)
        by = np.repeat([2.0, 3.0, 64.0, 1023.0], 8)
        any_x, trace = rt.oracle_spec_pow(bx, by, any_x=True), rt.oracle_spec_pow(bx, by)
    with np.errstate(all="ignore"):
        lib_b = rt.oracle_spec_pow(bx, by)
    assert np.array_equal(got.view(np.uint64), libm.view(np.uint64))
    beyond = ~(np.abs(bx) <= 2.0)
    assert np.array_equal(any_x[beyond].view(np.uint64), lib_b[beyond].view(np.uint64))
    assert any_x[0] == 4.0 and trace[0] == 4.0
    # exponent 0 is 1 for every x, as pow's
    with rt.oracle_pow(1):
        one = rt.oracle_spec_pow(np.array([0.0, -0.0, 0.5, np.nan, np.inf, 3.0]), np.zeros(6), any_x=True)
    assert np.array_equal(one, np.ones(6))


def test_the_mode_is_restored_after_an_exception(rt):
    lib = rt.oracle_lib()
    with pytest.raises(ZeroDivisionError):
        with rt.oracle_pow(1):
            assert lib.oracle_get_pow() == 1
            1 / 0
    assert lib.oracle_get_pow() == 0
    with rt.oracle_pow(1):
        with pytest.raises(RuntimeError):
            with rt.oracle_pow(1):
                pass
    assert lib.oracle_get_pow() == 0


# ------------------------------------------------------ 2. frames, mode 1 / mode 0
def _frame_scenes():
    out = {k: (lambda rt, f=f: rt.load_scene_from_json_text(f())) for k, f in SMALL.items()}
    sh = scenes.shading_scenes(dpi=SHADING_DPI)
    for name in shading_scene_names(True):
        out["shading/" + name] = lambda rt, name=name: scenes.shading_load(rt, name, sh[name])
    return out


FRAMES = _frame_scenes()


def _render(rt, sc):
    fb, st = rt.oracle_render(sc, sc.width, sc.height, 0, threads=8)
    return fb, (int(st.rays_intersect), int(st.rays_occluded))


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_mode1_frames_against_mode0(rt, name):
    """Only the rounding of a power moves: equal ray counts, a difference of a
    few ulps of a colour at most, and the reference's frame again afterwards."""
    sc = FRAMES[name](rt)
    assert integer_exponents(sc)
    before, counts0 = _render(rt, sc)
    with rt.oracle_pow(1):
        dev, counts1 = _render(rt, sc)
    after, counts2 = _render(rt, sc)
    assert rt.oracle_lib().oracle_get_pow() == 0
    assert after.tobytes() == before.tobytes() and counts2 == counts0
    assert counts1 == counts0
    differ = dev != before
    size = float(np.abs(dev - before).max())
    print(f"  {name}: {dev.shape[1]}x{dev.shape[0]}, {int(differ.sum())} of {differ.size} channels differ "
          f"({100.0 * differ.mean():.4f} %), by at most {size:.3g}; rays {counts1}")
    # the correctly rounded power and glibc's (< 1 ulp) are within an ulp, 2.2e-16 relative; the term reaches a
    # channel multiplied by ks * I_L, below 1e3 in any scene here (the bar of test_gpu_numerics' pow_general
    # test rests on the same factor), and through factors of at most 1 after that: 2.2e-13, rounded up
    assert size <= 1e-12


# ---------------------------------------------------------- 3. oracle_shade_hits
HITS = sorted(SCENES) + ["shading/" + n for n in SHADING] + [f"override/{a}/{b}" for a, b in OVERRIDES]


@pytest.mark.parametrize("key", HITS)
def test_oracle_shade_hits_is_the_oracles_own_shading(rt, key):
    """Bit for bit the colour and the Scene::occluded count of the oracle's
    Tracer::trace at recursion limit 1, which returns shade_lambert_phong of the
    closest hit with wo = (-r.d).normalized() (tracer.cpp:26-38), through
    oracle_trace_rays: the ray built once.  oracle_trace cannot judge bits: its
    ray passes through the camera and is normalised a second time, and its
    colour is the sum of 8 equal samples times 1/8, both of which round; it
    agrees in the counts and within 1e-9.  And oracle_shade, the numpy
    restatement, stays within its 1e-9 of the oracle's own shading."""
    r = shade_ref(rt, key)
    tsc = r.trace_scene(rt)
    wo = rt.rays_wo(rt.make_rays(r.o, r.d))
    rgb, no = rt.oracle_shade_hits(r.sc, r.H, wo, r.hit.astype(np.uint8), r.lights)
    t_rgb, t_ni, t_no = rt.oracle_trace_rays(tsc, r.o, r.d)
    assert np.array_equal(t_ni, np.ones(len(r), dtype=np.int64))
    assert np.array_equal(no, t_no) and np.array_equal(no, r.no)
    assert rgb.tobytes() == t_rgb.tobytes(), (key, np.flatnonzero((rgb != t_rgb).any(axis=1))[:8])
    f_rgb, _, f_no = rt.oracle_trace(tsc, r.o, r.d)
    assert np.array_equal(f_no, no), key
    with np.errstate(invalid="ignore"):
        f_err = float(np.abs(np.where(np.isfinite(rgb), f_rgb - rgb, 0.0)).max(initial=0.0))
    assert np.array_equal(np.isfinite(f_rgb), np.isfinite(rgb)) and f_err <= BAR, (key, f_err)
    # the restatement at its own bar
    fin = np.isfinite(rgb)
    assert np.array_equal(fin, np.isfinite(r.rgb))
    with np.errstate(invalid="ignore"):
        err = float(np.abs(np.where(fin, r.rgb - rgb, 0.0)).max(initial=0.0))
    assert np.array_equal(r.rgb[~fin], rgb[~fin], equal_nan=True)
    print(f"  {key}: {len(r)} entries, {int(r.hit.sum())} shaded, {int(no.sum())} occluded calls, bit-equal to the "
          f"oracle's trace; oracle_shade within {err:.3g}")
    assert err <= BAR
    # the scene's own lights spelt out as an override give the same bytes
    if r.lights is None:
        d = r.sc.desc
        own = [(list(d.lights[i].pos), list(d.lights[i].intensity)) for i in range(d.n_lights)]
        again, no2 = rt.oracle_shade_hits(r.sc, r.H, wo, r.hit.astype(np.uint8), own)
        assert again.tobytes() == rgb.tobytes() and np.array_equal(no2, no)


def test_oracle_shade_hits_mask_miss_colour_and_null_materials(rt):
    r = shade_ref(rt, "config4")
    wo = rt.rays_wo(rt.make_rays(r.o, r.d))
    rgb, no = rt.oracle_shade_hits(r.sc, r.H, wo, r.hit.astype(np.uint8), miss_rgb=(1.0, 1.0, 1.0))
    assert (~r.hit).any() and np.array_equal(rgb[~r.hit], np.ones((int((~r.hit).sum()), 3))) and not no[~r.hit].any()
    H = r.H[r.hit][:4].copy()
    H["mat"] = [-1, -2, r.sc.desc.n_materials, 2**31 - 1]
    rgb, no = rt.oracle_shade_hits(r.sc, H, wo[r.hit][:4])
    assert np.array_equal(rgb, np.tile([1.0, 0.0, 1.0], (4, 1))) and not no.any()
    with pytest.raises(ValueError):
        rt.oracle_shade_hits(r.sc, r.H, wo[:5])
