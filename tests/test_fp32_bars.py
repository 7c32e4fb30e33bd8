"""The FP32 bars themselves (tests/fp32_bars.py), without a device: they are
deterministic, their reference frame is the oracle's, every scene the GPU
tests use is within its cap of unconstrained / unstable pixels, a float32
stand-in for a correct FP32 trace passes them, and three small shading
mistakes that the whole-frame bars of tests/test_gpu_fp32.py let through do
not.  tests/test_gpu_fp32_bars.py holds the rtf kernels to the same bars.

Run with -s: the shares per scene (profiles/fp32_bars/cpu_caps.txt)."""
import numpy as np
import pytest

import fp32_bars as B
import scenes
from test_gpu_edges import _cfg4, _frame as edge_frame
from test_gpu_parity import SMALL
from test_kernel_table import RECIPES

RTF = [r for r in RECIPES if r.row.startswith("rtf::")]
RECIPE_SCENES = sorted({r.scene_name for r in RTF})
CASES = ["small/" + k for k in sorted(SMALL)] + ["recipe/" + k for k in RECIPE_SCENES]
EDGES = ["edge/cfg4@3x17", "edge/cfg4@1x1"]   # frames of partial waves only (tests/test_gpu_edges.py): held, not capped

# share of a frame's pixels that may be unconstrained (standard, bar > 1e-3) / unstable (paper): conditions on
# the inputs, measured on the reference alone.  Measured: standard <= 0.44 % on every SMALL scene but cfg5
# (2.4 %); paper <= 0.95 %.
CAP_SMALL, CAP_RECIPE, CAP_PAPER, CAP_MOST = 0.03, 0.05, 0.02, 0.10
# a recipe scene over CAP_RECIPE: its own measured share plus one point (none may exceed CAP_MOST)
CAP_NAMED = {}
assert all(v <= CAP_MOST for v in CAP_NAMED.values())

MISTAKES = ("specular x 0.99", "lights moved 1e-3", "shininess + 1")
MISTAKE_SCENES = ("cfg4", "snorlax", "penguin")


def scene_of(case):
    """(JSON text, directional lights or None, seed) of "small/<name>", "recipe/<scene_name>" or "edge/cfg4@WxH"."""
    fam, _, key = case.partition("/")
    if fam == "edge":
        assert key.startswith("cfg4@")
        text, lights = edge_frame(_cfg4(), *(int(v) for v in key[5:].split("x"))), None
    else:
        text, lights = (SMALL[key](), None) if fam == "small" else scenes.recipe_scene(key)
    return text, lights, B.seed_of(case)


def cap_of(case):
    return CAP_SMALL if case.startswith("small/") else CAP_NAMED.get(case, CAP_RECIPE)


def test_scene32_rounds_every_real_number():
    text, lights = B.scene32('{"a": [0.1, 1, {"b": 1e-3, "c": true, "d": "x"}], "e": 16777216}', [((0.1, 0.2, 0.3), (1, 2, 0.7))])
    assert text == '{"a": [%r, 1, {"b": %r, "c": true, "d": "x"}], "e": 16777216}' % (float(np.float32(0.1)), float(np.float32(1e-3)))
    assert lights == [([float(np.float32(v)) for v in (0.1, 0.2, 0.3)], [1.0, 2.0, float(np.float32(0.7))])]
    with pytest.raises(AssertionError):
        B.scene32('{"e": 16777217}')
    again, _ = B.scene32(text)
    assert again == text


def test_bars_are_deterministic_for_a_seed(rt):
    text, lights, seed = scene_of("small/cfg4")
    a, p = B.standard_bars(rt, text, lights, seed), B.paper_stable(rt, text, lights, seed)
    B._standard.clear()
    B._paper.clear()
    b, q = B.standard_bars(rt, text, lights, seed), B.paper_stable(rt, text, lights, seed)
    assert a[0] is not b[0] and all(np.array_equal(x, y) for x, y in zip(a + p, b + q))
    assert not a[1].flags.writeable and not p[1].flags.writeable
    c = B.standard_bars(rt, text, lights, seed + 1)
    assert np.array_equal(c[0], a[0]) and not np.array_equal(c[1], a[1])   # (the seed moves the probes only)


@pytest.mark.parametrize("case", CASES)
def test_reference_and_caps(rt, case):
    """ref is oracle_render's frame to 1e-12 with its ray counts; the frame is
    within its cap in both modes; the bar is never below its floor."""
    text, lights, seed = scene_of(case)
    r = B.standard_case(rt, text, lights, seed)
    sc = B.load(rt, text, lights)
    fb, ost = rt.oracle_render(sc, sc.width, sc.height, 0, threads=8)
    pref, stable = B.paper_stable(rt, text, lights, seed)
    unc, uns = float(r.unconstrained.mean()), float(np.mean(~stable))
    print(f"  {case}: {r.W}x{r.H}, unconstrained {unc:.4%} (cap {cap_of(case):.0%}), unstable {uns:.4%} (cap {CAP_PAPER:.0%}), "
          f"|ref - oracle_render| {np.abs(r.ref - fb).max():.2g}, largest V {r.V.max():.3g}, median bar {np.median(r.bar):.3g}"
          f"{', no colour moves with its ray' if r.ray_free else ''}")
    assert np.abs(r.ref - fb).max() <= 1e-12
    assert r.counts == (int(ost.rays_intersect), int(ost.rays_occluded))
    assert (r.bar >= B.FLOOR).all() and r.bar.shape == (r.H, r.W)
    assert unc <= cap_of(case)
    assert uns <= CAP_PAPER
    assert np.array_equal(pref, rt.oracle_render(sc, sc.width, sc.height, 1, threads=8)[0])


def test_the_frames_no_ray_moves(rt):
    """inside_camera, recursion0 and csg_groups_inside: no sample's colour moves with its ray, which is
    where the GPU test holds the ray counts to the oracle's as well."""
    for name in ("inside_camera", "recursion0", "csg_groups_inside"):
        assert B.standard_case(rt, *scene_of("small/" + name)).ray_free, name
    assert not B.standard_case(rt, *scene_of("small/cfg4")).ray_free


def standin(rt, case):
    """A correct float trace of the oracle's rays, as far as FP64 can stand in for one: every scene number
    and every ray rounded to float32, each ray moved again by 8 u, traced in FP64."""
    text, lights, seed = scene_of(case)
    r = B.standard_case(rt, text, lights, seed)
    rng = np.random.default_rng(seed + 1)
    o, d = r.o.astype(np.float32).astype(np.float64), r.d.astype(np.float32).astype(np.float64)
    d = d + 8 * B.U * B.unit_vectors(rng, len(d))
    o = o + 8 * B.U * np.maximum(1.0, np.sqrt((o * o).sum(axis=1)))[:, None] * B.unit_vectors(rng, len(o))
    rgb, _, _ = B.trace(rt, B.load(rt, *B.scene32(text, lights)), o, d)
    return B.resolve(rgb, r.H, r.W)


@pytest.mark.parametrize("case", CASES + EDGES)
def test_float32_standin_passes(rt, case):
    text, lights, seed = scene_of(case)
    ref, bar, _ = B.standard_bars(rt, text, lights, seed)
    assert B.held32("stand-in " + case, standin(rt, case), ref, bar) <= 1.0
    pref, stable = B.paper_stable(rt, text, lights, seed)
    sc32 = B.load(rt, *B.scene32(text, lights))
    B.held32_paper("stand-in paper " + case, rt.oracle_render(sc32, sc32.width, sc32.height, 1, threads=8)[0], pref, stable)


def mistaken(rt, sc, which):
    if which == "specular x 0.99":
        return B.copy_desc(rt, sc, materials=lambda m: setattr(m, "ks", m.ks * 0.99))
    if which == "shininess + 1":
        return B.copy_desc(rt, sc, materials=lambda m: setattr(m, "shininess", m.shininess + 1.0))
    assert which == "lights moved 1e-3"

    def move(l):
        l.pos[:] = [v + 1e-3 / np.sqrt(3.0) for v in l.pos]
    return B.copy_desc(rt, sc, lights=move)


@pytest.mark.parametrize("name", MISTAKE_SCENES)
@pytest.mark.parametrize("which", MISTAKES)
def test_a_small_mistake_fails_the_bar_and_passes_the_old_ones(rt, which, name):
    """What the per-pixel bar adds: the frame's own rays traced (in FP64) on a scene with one small mistake."""
    text, lights, seed = scene_of("small/" + name)
    r = B.standard_case(rt, text, lights, seed)
    bad = mistaken(rt, B.load(rt, text, lights), which)
    rgb, ni, no = B.trace(rt, bad, r.o, r.d)
    fb = B.resolve(rgb, r.H, r.W)
    d = np.abs(fb - r.ref)
    print(f"  {name}, {which}: far {float(np.mean(d > 1e-3)):.4f} mean {d.mean():.2e}, "
          f"{float(np.mean(d.max(axis=2) > r.bar)):.2%} of the pixels over the bar")
    assert d.max() > 0
    assert B.old_bars_pass(fb, r.ref, (int(ni.sum()), int(no.sum())), r.counts)
    with pytest.raises(AssertionError):
        B.held32(f"mistake {name} {which}", fb, r.ref, r.bar)


def test_every_exception_is_shown_on_the_reference(rt):
    """Each row of fp32_bars.EXCEPTIONS, without a device: at every pixel it lists, DENSE_PROBES seeded
    direction probes of the cause's magnitude on the pixel's own 8 rays give a bar of at least the row's
    multiplier times the pixel's bar.  The pixel sits next to a decision edge that the three draws of
    standard_bars() missed, and the allowance is what the same model gives when it is sampled densely.
    The rows together stay under the 0.5 % that held32() allows a frame."""
    for pattern, cause, mult, case, pixels in B.EXCEPTIONS:
        text, lights, seed = scene_of(case)
        r = B.standard_case(rt, text, lights, seed)
        sc = B.load(rt, text, lights)
        assert len(set(pixels)) == len(pixels) <= B.EXCEPTED_SHARE * r.bar.size, pattern
        for y, x in pixels:
            i = (y * r.W + x) * 8
            o, d, rgb = r.o[i:i + 8], r.d[i:i + 8], r.rgb[i:i + 8]
            rng = np.random.default_rng([seed, y, x])
            V = np.array(r.V[y, x])
            for _ in range(B.DENSE_PROBES):
                c, _, _ = rt.oracle_trace_rays(sc, o, d + B.CAUSE_PROBE[cause] * B.unit_vectors(rng, 8))
                V = np.maximum(V, np.abs(c - rgb).max(axis=1))
            dense = float((2.0 * V + B.FLOOR).mean())
            print(f"  {pattern} ({y}, {x}): bar {r.bar[y, x]:.3g}, under {B.DENSE_PROBES} probes {dense:.3g} = "
                  f"{dense / r.bar[y, x]:.3g} bars (multiplier {mult:g})")
            assert dense >= mult * r.bar[y, x], (pattern, y, x)


def test_the_rules_themselves(monkeypatch):
    """held32() and held32_paper() on made-up arrays: what passes and what does not."""
    ref = np.full((10, 40, 3), 0.5)
    bar = np.full((10, 40), B.FLOOR)
    bar[0, 0] = 0.25
    ok = ref.copy()
    ok[1, 1, 2] += B.FLOOR * 0.999
    ok[2, 2, 0] -= B.FLOOR * 0.5
    ok[0, 0, 1] += 0.249
    assert B.held32("rules/pass", ok, ref, bar) == pytest.approx(0.999, rel=1e-6)
    assert B.held32("rules/equal", ref, ref, bar) == 0.0
    for y, x, v in ((1, 1, 0.5 + B.FLOOR * 1.01), (0, 0, 0.76), (3, 3, np.nan), (3, 3, np.inf), (9, 39, 0.5 - 2 * B.FLOOR)):
        bad = ref.copy()
        bad[y, x, 1] = v
        with pytest.raises(AssertionError):
            B.held32("rules/fail", bad, ref, bar)
    with pytest.raises(AssertionError):
        B.held32("rules/shape", ref[:, :-1], ref, bar)
    with pytest.raises(AssertionError):
        B.held32("rules/bar below the floor", ref, ref, bar * 0.5)
    # an exception: at its listed pixels only, within its multiplier, for the cases its pattern names, and on
    # at most 0.5 % of the frame's pixels (2 of 400)
    row = ("rules/named*", "named: V undersampled", 4.0, "made up", ((5, 5), (5, 6), (5, 7)))
    monkeypatch.setattr(B, "EXCEPTIONS", (row,))
    two = ref.copy()
    two[5, 5, 0] += 3.9 * B.FLOOR
    two[5, 6, 0] += 2 * B.FLOOR
    assert B.held32("rules/named/f4", two, ref, bar) == pytest.approx(3.9, rel=1e-6)
    with pytest.raises(AssertionError):
        B.held32("rules/other", two, ref, bar)
    three = two.copy()
    three[5, 7, 0] += 2 * B.FLOOR
    with pytest.raises(AssertionError):
        B.held32("rules/named/f4", three, ref, bar)   # (three excepted pixels of 400)
    elsewhere = two.copy()
    elsewhere[6, 6, 0] += 2 * B.FLOOR
    with pytest.raises(AssertionError):
        B.held32("rules/named/f4", elsewhere, ref, bar)   # (a pixel the row does not list)
    two[5, 5, 0] += 0.2 * B.FLOOR
    with pytest.raises(AssertionError):
        B.held32("rules/named/f4", two, ref, bar)   # (over the multiplier)
    # paper frames
    pref = np.where(np.arange(40)[None, :, None] < 20, 1.0, 0.0) * np.ones((10, 40, 3))
    stable = np.ones((10, 40), dtype=bool)
    stable[4, 19:21] = False
    fb = pref.copy()
    fb[4, 19] = 0.0
    assert B.held32_paper("rules/paper pass", fb, pref, stable) == 1
    for y, x, v in ((4, 18, 0.2), (0, 39, -0.0), (9, 0, np.nextafter(1.0, 0.0)), (2, 2, np.nan)):
        bad = fb.copy()
        bad[y, x, 2] = v
        with pytest.raises(AssertionError):
            B.held32_paper("rules/paper fail", bad, pref, stable)
