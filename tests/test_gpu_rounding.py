"""The FP64 kernels against the oracle BIT FOR BIT (DESIGN.md Numerics: device
code is built without contraction and with IEEE division and square root, and
every expression keeps the reference's operation order, "so the GPU rounds
exactly like the x86-64 reference except inside pow()").

The reference is the oracle in mode 1 (rtamd.oracle_pow(1)): libm everywhere
but in the two pow(rdotv, shininess) calls of shade(), which return the
correctly rounded x^k wherever the device takes pow_spec
(tests/test_oracle_rounding.py holds that oracle on the CPU).  Every output is
compared through held(): every byte of every frame channel, hit record and
colour; no ray, hit or pixel is left out.  The 1e-5 tests stay beside this file
as they are: that bar is the published contract, this one guards the rule the
kernels were written to.

Exceptions exist only through EXCEPTIONS below, each (case, cause, bar).

Nothing computed under mode 1 is stored in another module's cache: inputs
(scenes, rays, hits) are built first, in mode 0, and only the oracle call whose
answer this file compares runs inside `with rt.oracle_pow(1)`.

Run with -s: every case prints its element count, how many elements differ
from the oracle outside the exceptions (0), and what the exceptions measured
(profiles/rounding/gpu_tests.txt).

Measured on an MI355X: of the 300 cases here every one is bit-equal to the
oracle except the ten with a power from the device library (the pow_general
entries and one named entry below, 0.5 to 6 ulp); no other exception was
needed, and neither general rule (tiny, non-finite) was used by any case.  The
same file on a build whose FP64 trace objects were compiled with
-ffp-contract=fast fails 288 of the 300 (about half the channels of a frame
move, by hundreds of ulps), while every standard-mode 1e-5 assertion of
tests/test_gpu_parity.py still passes (profiles/rounding/contract_demo.txt)."""
import json

import numpy as np
import pytest

import scenes
import test_graph_scenes as G
import test_leaf_scenes as L
import test_placed_scenes as P
from test_gpu_node_query import kats_rays, logged
from test_gpu_parity import SMALL
from test_gpu_query import SCENES, case, q_isect
from test_gpu_radiance import recipe_rays
from test_kernel_table import RECIPES, recipe_id
from test_node_query_plan import load as node_load
from test_oracle_rounding import SHADING_DPI, integer_exponents, shading_scene_names
from test_shade_plan import override_lights, shade_ref

pytestmark = pytest.mark.gpu

TINY = 2.0 ** -990

# ---------------------------------------------------------------- exceptions
# (case, cause, bar).  case: the id held() is called with ("*": every case).
#   tiny        the oracle's value is below 2^-990 in magnitude (bar): the GPU's must be below it too
#               (pow_spec promises nothing below 2^-1000; a zero's sign is not compared)
#   non-finite  the oracle's value is an infinity or a NaN: the GPU's is the same infinity, or a NaN
#               (payloads are not compared)
#   pow_general a shininess outside pow_spec's range (12.5, 0.5, -2, 1024, 2000): the device library's
#               pow against libm's.  bar in ulps of max(1, |oracle|): four times the largest value
#               measured on an MI355X against the mode-1 oracle (written beside each bar); both powers
#               are within about an ulp of exact, so the channels differ by a few ulps of the specular
#               term, and the factor covers inputs not drawn
#   named: ... any other cause that was found sound, at the narrowest bar that holds (DESIGN.md Numerics)
EXCEPTIONS = (
    ("*", "tiny", TINY),
    ("*", "non-finite", None),
    # exponents_few0 (0, 7, 1024) and exponents_few1 (1, 127, 2000) measured 0 differing channels: no entry
    ("frame shading/exponents_few2", "pow_general", 2.0),    # measured 0.5 (3 of 12096 channels; 2, 255, 12.5)
    ("frame shading/exponents_few3", "pow_general", 4.0),    # measured 1 (10 of 12096; 3, 1000, 0.5)
    ("frame shading/exponents_few4", "pow_general", 24.0),   # measured 6 (143 of 12096; 5, 1023, -2)
    ("frame shading/exponents_wave", "pow_general", 16.0),   # measured 4 (156 of 63504; all fifteen)
    ("shade shading/exponents_wave wo=-d", "pow_general", 8.0),          # measured 2 (3 of 1152)
    ("shade shading/exponents_wave random wo", "pow_general", 12.0),     # measured 3 (9 of 1152)
    ("shade shading/exponents_wave override", "pow_general", 8.0),       # measured 2 (7 of 1152)
    ("shade shading/exponents_wave thinned mask", "pow_general", 8.0),   # measured 2 (3 of 1152)
    # a wo three units long: rdotv exceeds 2, where the shading kernels hand every power, integer exponents
    # included, to the device library's pow (pow_spec's overflow rule) and the oracle to libm: the same two
    # libraries as above, through another door.  Measured 4 (91 of 2304 colours, which reach 2^78 there)
    ("shade config4 wo x3", "named: pow_general beyond |rdotv| = 2", 4.0),
)
_NAMED = {c: (cause, bar) for c, cause, bar in EXCEPTIONS if c != "*"}
assert all(cause in ("pow_general", "unexplained") or cause.startswith("named: ") for cause, _ in _NAMED.values())


def held(case_id, got, ref):
    """got against ref (float64 arrays of one shape) bit for bit, but for
    EXCEPTIONS; prints the case's line and returns the largest difference of a
    named exception in ulps of max(1, |ref|)."""
    got = np.ascontiguousarray(got, dtype=np.float64)
    ref = np.ascontiguousarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (case_id, got.shape, ref.shape)
    g, r = got.reshape(-1), ref.reshape(-1)
    idx = np.flatnonzero(g.view(np.uint64) != r.view(np.uint64))
    gi, ri = g[idx], r[idx]
    with np.errstate(all="ignore"):
        nonfinite = ~np.isfinite(ri) & ((np.isnan(gi) & np.isnan(ri)) | (np.isinf(ri) & (gi == ri)))
        tiny = np.isfinite(ri) & (np.abs(ri) < TINY) & (np.abs(gi) < TINY)
        ulps = np.abs(gi - ri) / np.spacing(np.maximum(1.0, np.abs(ri)))
    rest = ~(nonfinite | tiny)
    cause, bar = _NAMED.get(case_id, (None, 0.0))
    with np.errstate(invalid="ignore"):
        wrong = idx[rest][~(ulps[rest] <= bar)]
    named = int(rest.sum()) - len(wrong)
    measured = float(np.nan_to_num(ulps[rest], nan=np.inf).max(initial=0.0))
    line = f"  {case_id}: {g.size} elements, {len(wrong)} differ"
    if nonfinite.any() or tiny.any():
        line += f"; exceptions: {int(tiny.sum())} tiny, {int(nonfinite.sum())} non-finite of the oracle's kind"
    if cause is not None:
        line += f"; {cause}: {named} within the bar of {bar:g} ulp, largest {measured:.3g} ulp"
    elif rest.any():
        line += f", by at most {measured:.3g} ulp of max(1, |oracle|)"
    print(line)
    assert len(wrong) == 0, (case_id, f"{len(wrong)} of {g.size} elements differ, largest {measured:.3g} ulp of max(1, |ref|)",
                             [(int(k), float(g[k]).hex(), float(r[k]).hex()) for k in wrong[:6]])
    return measured


def held_records(case_id, got_ok, got, ref_ok, ref):
    """rt_hit records: the flags, mat and front_face equal, t, p, n through
    held(); a miss is mat -1 and zeros on both sides."""
    got_ok, ref_ok = np.asarray(got_ok, dtype=bool), np.asarray(ref_ok, dtype=bool)
    ref = ref.copy()
    ref[~ref_ok] = np.zeros(1, dtype=ref.dtype)
    ref["mat"][~ref_ok] = -1
    assert np.array_equal(got_ok, ref_ok), (case_id, np.flatnonzero(got_ok != ref_ok)[:8])
    assert np.array_equal(got["mat"], ref["mat"]) and np.array_equal(got["front_face"], ref["front_face"]), case_id
    pack = lambda h: np.concatenate([h["t"][:, None], h["p"], h["n"]], axis=1)   # noqa: E731
    return held(case_id, pack(got), pack(ref))


def test_the_exception_rules_themselves():
    """held() on made-up values: what passes and what does not (no device)."""
    nan2 = np.array([0x7ff8000000000001], dtype=np.uint64).view(np.float64)[0]
    ok_ref = np.array([1.0, np.inf, -np.inf, np.nan, 0.0, 1e-300, 2.0 ** -991])
    ok_got = np.array([1.0, np.inf, -np.inf, nan2, -0.0, 0.0, -(2.0 ** -995)])
    assert held("rules/pass", ok_got, ok_ref) == 0.0
    for g, r in ((np.nextafter(1.0, 2.0), 1.0), (np.inf, -np.inf), (np.nan, np.inf), (np.inf, np.nan), (1.0, np.nan),
                 (np.nan, 1.0), (2.0 ** -989, 0.0), (0.0, 2.0 ** -989), (np.inf, 1e308), (0.1 + 0.2, 0.3)):
        with pytest.raises(AssertionError):
            held("rules/fail", np.array([1.0, g]), np.array([1.0, r]))


# -------------------------------------------------------------------- frames
def _render(rt, sc, flags=0):
    st = rt.Stats()
    fb, rows = logged(rt, lambda: rt.Tracer(sc, sc.width, sc.height, 0, flags=flags).render(st))
    return fb, (int(st.rays_intersect), int(st.rays_occluded)), rows


def _frame(rt, case_id, sc, flags=0):
    """One standard frame of a loaded scene against the mode-1 oracle's: every
    channel through held(), the ray counts equal.  Returns the kernels launched."""
    fb, counts, rows = _render(rt, sc, flags)
    with rt.oracle_pow(1):
        ref, ost = rt.oracle_render(sc, sc.width, sc.height, 0, threads=8)
    held(case_id, fb, ref)
    assert counts == (int(ost.rays_intersect), int(ost.rays_occluded)), case_id
    return rows


def _load_recipe(rt, name):
    text, lights = scenes.recipe_scene(name)
    sc = rt.load_scene_from_json_text(text)
    return rt.with_dir_lights(sc, lights) if lights else sc


STD_ROWS = [r for r in RECIPES if r.query < 0 and r.mode == 0 and r.row.startswith(("rtd::", "rtdb::"))]


@pytest.mark.parametrize("r", STD_ROWS, ids=recipe_id)
def test_every_standard_row(gpu, r):
    """Every rtd and rtdb row of the standard tables through its recipe, the row asserted in the launch log."""
    assert r.frame == 0
    rows = _frame(gpu, "row " + recipe_id(r), _load_recipe(gpu, r.scene_name), r.flags)
    assert rows == [r.row]


def test_the_standard_rows_are_all_here(gpu):
    have = {r.row for r in STD_ROWS}
    for t, name in enumerate(gpu.KERNEL_TABLES):
        if name in ("rtd std", "rtdb std"):
            rows = gpu.kernel_rows(t)
            assert rows and set(rows) <= have, name


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_and_torture_frames(gpu, name):
    _frame(gpu, "frame " + name, gpu.load_scene_from_json_text(SMALL[name]()))


@pytest.mark.parametrize("key", G.NAMED)
def test_graph_case_frames(gpu, key):
    _frame(gpu, "frame graph/" + key, G.load(gpu, key))


@pytest.mark.parametrize("key", L.NAMED)
def test_leaf_case_frames(gpu, key):
    _frame(gpu, "frame leaf/" + key, L.load(gpu, key))


@pytest.mark.parametrize("name", sorted(scenes.bvh_scenes(16)))
def test_bvh_frames(gpu, name):
    sc = gpu.load_scene_from_json_text(json.dumps(scenes.bvh_scenes(16)[name]))
    _frame(gpu, "frame bvh/" + name, sc)
    for f in (gpu.RT_FLAG_NO_BVH, gpu.RT_FLAG_FORCE_BVH):
        _frame(gpu, f"frame bvh/{name}/f{f}", gpu.load_scene_from_json_text(json.dumps(scenes.bvh_scenes(16)[name])), f)


@pytest.mark.parametrize("name", sorted(scenes.dir_light_cases()))
def test_dir_light_frames(gpu, name):
    text, lights = scenes.dir_light_cases()[name]
    _frame(gpu, "frame dir/" + name, gpu.with_dir_lights(gpu.load_scene_from_json_text(text), lights))


PLACED = ("mid", "far", "x24_far")   # one unit-scale placement and two far ones


@pytest.mark.parametrize("pl", PLACED)
@pytest.mark.parametrize("name", P.FRAME_SCENES)
def test_placed_frames(gpu, name, pl):
    scene, lights = P.scene_dict(name)
    _frame(gpu, f"frame placed/{name}/{pl}", P.load(gpu, scenes.placed(scene, *P.PL[pl]), lights))


SHADING_INT, SHADING_ODD = shading_scene_names(True), shading_scene_names(False)


@pytest.mark.parametrize("name", SHADING_INT)
def test_shading_frames_integer_exponents(gpu, name):
    sc = scenes.shading_load(gpu, name, scenes.shading_scenes(dpi=SHADING_DPI)[name])
    assert integer_exponents(sc)
    _frame(gpu, "frame shading/" + name, sc)


@pytest.mark.parametrize("name", SHADING_ODD)
def test_shading_frames_other_exponents(gpu, name):
    """Exponents outside pow_spec's range: the pow_general exception of this case."""
    sc = scenes.shading_load(gpu, name, scenes.shading_scenes(dpi=SHADING_DPI)[name])
    assert not integer_exponents(sc)
    _frame(gpu, "frame shading/" + name, sc)


# --------------------------------------------------------- intersect queries
@pytest.mark.parametrize("name", sorted(SCENES))
def test_intersect_records(gpu, name):
    """The 768 shuffled camera and surface rays of tests/test_gpu_query.py (every wave a mix), with and
    without RT_FLAG_NO_CULL."""
    c = case(gpu, name)   # (rays and Scene::intersect records: no power in them, the cache is mode 0's and stays so)
    for flags, tag in ((0, ""), (gpu.RT_FLAG_NO_CULL, " NO_CULL")):
        got = q_isect(gpu, c.scene, c.rays, flags=flags)
        held_records(f"intersect {name}{tag}", got.hit, got.records, c.ref_hit, c.ref_rec)
    assert c.ref_hit.sum() >= len(c.rays) // 4


@pytest.mark.parametrize("key", L.NAMED)
def test_intersect_records_leaf_cases(gpu, key):
    c = L.leaf_case(gpu, key)
    got = q_isect(gpu, c.scene, c.rays)
    held_records(f"intersect leaf/{key}", got.hit, got.records, c.ref_hit, c.ref_rec)


@pytest.mark.parametrize("recipe", scenes.node_recipes(), ids=lambda r: r.row)
def test_node_records(gpu, recipe):
    """rt_query_node_intersect and rt_query_node_interval of every node row's recipe."""
    sc = node_load(gpu, recipe.scene_name)
    node = int(sc.desc.objects[recipe.obj])
    o, d = kats_rays(11)
    ref_hit, ref_rec = gpu.oracle_node_intersect(sc, node, o, d)
    ref_enter, ref_exit, ref_ok = gpu.oracle_node_interval(sc, node, o, d)
    for flags, tag in ((0, ""), (gpu.RT_FLAG_NO_CULL, " NO_CULL")):
        (got, (enter, ex, ok)), rows = logged(gpu, lambda: (gpu.query_node_intersect(sc, node, o, d, flags=flags),
                                                            gpu.query_node_interval(sc, node, o, d, flags=flags)))
        assert rows[recipe.kind] == recipe.row
        held_records(f"node intersect {recipe.row}{tag}", got.hit, got.records, ref_hit, ref_rec)
        held_records(f"node enter {recipe.row}{tag}", ok, enter, ref_ok, ref_enter)
        held_records(f"node exit {recipe.row}{tag}", ok, ex, ref_ok, ref_exit)
    assert ref_hit.any() and ref_ok.any()


@pytest.mark.parametrize("sname", sorted(scenes.torture_scenes()))
def test_node_records_every_torture_node(gpu, sname):
    """Every node of a torture scene, 64 rays each; the nodes' records side by side in one comparison."""
    sc = node_load(gpu, "torture/" + sname)
    o, d = kats_rays(23, 64)
    got, ref = [[] for _ in range(6)], [[] for _ in range(6)]
    for node in range(sc.desc.n_nodes):
        ref_hit, ref_rec = gpu.oracle_node_intersect(sc, node, o, d)
        ref_enter, ref_exit, ref_ok = gpu.oracle_node_interval(sc, node, o, d)
        h = gpu.query_node_intersect(sc, node, o, d)
        enter, ex, ok = gpu.query_node_interval(sc, node, o, d)
        for k, v in enumerate((h.hit, h.records, ok, enter, ok, ex)):
            got[k].append(v)
        for k, v in enumerate((ref_hit, ref_rec, ref_ok, ref_enter, ref_ok, ref_exit)):
            ref[k].append(v)
    got, ref = [np.concatenate(v) for v in got], [np.concatenate(v) for v in ref]
    for k, tag in enumerate(("intersect", "enter", "exit")):
        held_records(f"node {tag} torture/{sname}, {sc.desc.n_nodes} nodes", got[2 * k], got[2 * k + 1], ref[2 * k],
                     ref[2 * k + 1])


# ------------------------------------------------------------------ radiance
def _radiance(rt, case_id, sc, o, d, flags=0):
    """rt_query_radiance of Ray(o, (o + d) - o) - the rays of tests/test_gpu_radiance.py - against the
    mode-1 oracle's Tracer::trace of the same rays, built once (oracle_trace_rays): every colour through
    held(), the batch's counts the sums of the oracle's, nothing left out."""
    o = np.ascontiguousarray(o, dtype=np.float64)
    d = rt.oracle_trace_dirs(o, d)
    st = rt.Stats()
    got, rows = logged(rt, lambda: rt.query_radiance(sc, o, d, flags, st))
    with rt.oracle_pow(1):
        rgb, ni, no = rt.oracle_trace_rays(sc, o, d)
    held(case_id, got, rgb)
    assert (st.rays_intersect, st.rays_occluded) == (int(ni.sum()), int(no.sum())), case_id
    return rows


@pytest.mark.parametrize("name", sorted(SCENES))
def test_radiance(gpu, name):
    c = case(gpu, name)
    _radiance(gpu, "radiance " + name, c.scene, c.rays["o"], c.rays["d"])


@pytest.mark.parametrize("name", ["lights65_csg", "near_light_wave", "far_skip_few", "null_mat_csg"])
def test_radiance_shading_inputs(gpu, name):
    sc = scenes.shading_load(gpu, name, scenes.shading_scenes(dpi=16)[name])
    _radiance(gpu, "radiance shading/" + name, sc, *recipe_rays(gpu, sc, 192, 192, 7100 + len(name)))


@pytest.mark.parametrize("recipe", scenes.radiance_recipes(), ids=lambda r: r.row)
def test_radiance_rows(gpu, recipe):
    sc = _load_recipe(gpu, recipe.scene_name)
    rows = _radiance(gpu, "radiance row " + recipe.row, sc, *recipe_rays(gpu, sc, 128, 128, 4242), flags=recipe.flags)
    assert rows == [recipe.row]


@pytest.mark.parametrize("key", L.NAMED)
def test_radiance_leaf_cases(gpu, key):
    """The leaf cases' own 768 rays, huge_enclosing's included.  Ray 476 of that case is the one
    tests/test_gpu_leaves.py leaves out as oracle-unstable: a surface ray that starts on the sphere of
    radius 1e6 and travels t = 1e6 to a point near the origin.  There the reference of that file,
    oracle_trace, is 2.2e-4 away from the kernel and from oracle_trace_rays alike: its ray passes
    through a camera and is normalised a second time, one ulp of direction that t = 1e6 turns into 1e-4
    of hit point.  The kernel traces the ray built once, as Tracer::trace does, and equals that trace
    bit for bit: the rule holds on that ray, the allowance covered the reference call's own rounding."""
    c = L.leaf_case(gpu, key)
    _radiance(gpu, "radiance leaf/" + key, c.scene, c.rays["o"], c.rays["d"])


# ------------------------------------------------------------------- shading
def _random_wo(r, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(len(r), 3))
    v /= np.sqrt((v * v).sum(axis=1))[:, None]
    return np.where(((v * r.H["n"]).sum(axis=1) < 0)[:, None], -v, v)   # (into the normal's hemisphere)


def _shade(rt, case_id, r, wo, mask, lights, flags=0):
    """rt_query_shade against oracle_shade_hits in mode 1: colours through held(), the count equal."""
    st = rt.Stats()
    got, rows = logged(rt, lambda: rt.query_shade(r.sc, r.H, wo, mask, lights, None, flags, st))
    with rt.oracle_pow(1):
        rgb, no = rt.oracle_shade_hits(r.sc, r.H, wo, mask, lights)
    held(case_id, got, rgb)
    assert (st.rays_intersect, st.rays_occluded) == (0, int(no.sum())), case_id
    return rows


def _shade_forms(rt, what, r, seed, n_override=3):
    """wo = -d, a random wo, the light override, and a mask that also drops every third hit."""
    wo = rt.rays_wo(rt.make_rays(r.o, r.d))
    mask = r.hit.astype(np.uint8)
    thin = mask.copy()
    thin[::3] = 0
    forms = [("wo=-d", wo, mask, r.lights), ("random wo", _random_wo(r, seed), mask, r.lights),
             ("override", wo, mask, override_lights(what, n_override)), ("thinned mask", wo, thin, r.lights)]
    if r.hit.all():
        forms.append(("no mask", wo, None, r.lights))
    rows, failed = [], []
    for tag, *args in forms:   # (every form prints its line before the first failure is raised)
        try:
            rows.append(_shade(rt, f"shade {what} {tag}", r, *args))
        except AssertionError as e:
            failed.append(e)
    if failed:
        raise failed[0]
    assert all(v == rows[0] for v in rows)
    return rows[0]


@pytest.mark.parametrize("recipe", scenes.shade_recipes(), ids=lambda r: r.row)
def test_shade_rows(gpu, recipe):
    r = shade_ref(gpu, "census/" + recipe.scene_name)   # (its hits and rays; its mode-0 colours are not read)
    rows = _shade_forms(gpu, "row " + recipe.row, r, 31)
    assert rows == [recipe.row]
    assert r.hit.sum() >= len(r) // 4


@pytest.mark.parametrize("name", sorted(SCENES))
def test_shade_every_scene(gpu, name):
    _shade_forms(gpu, name, shade_ref(gpu, name), 47)


@pytest.mark.parametrize("name", ["lights65_csg", "near_light_wave", "far_skip_few", "null_mat_csg", "extremes_few",
                                  "extremes_csg", "lights33_xform"])
def test_shade_shading_inputs(gpu, name):
    _shade_forms(gpu, "shading/" + name, shade_ref(gpu, "shading/" + name), 515 + len(name), n_override=33)


def test_shade_other_exponents(gpu):
    """shading/exponents_wave: the pow_general exception of these cases."""
    _shade_forms(gpu, "shading/exponents_wave", shade_ref(gpu, "shading/exponents_wave"), 515 + len("exponents_wave"))


def test_shade_a_long_wo(gpu):
    """wo of length 1.5: rdotv reaches (1, 2], still pow_spec in the shading kernels, bit-equal.  Of
    length 3: beyond 2 the power is the device library's (the named exception of this case)."""
    r = shade_ref(gpu, "config4")
    wo = gpu.rays_wo(gpu.make_rays(r.o, r.d))
    mask = r.hit.astype(np.uint8)
    _shade(gpu, "shade config4 wo x1.5", r, wo * 1.5, mask, None)
    _shade(gpu, "shade config4 wo x3", r, wo * 3.0, mask, None)
