"""The scene-graph scenes on the CPU (no device is touched): the named edge
cases of scenes.graph_cases and the seeded grammar scenes.graph_scene, held
here before tests/test_gpu_graph.py relies on them.

Coverage: over the named cases and SEEDS, every bin of the compiled-form
histogram (rt_test_compile_forms) that the compiler can emit is non-zero:
every object kind and opcode, OP_NEVER in interval mode, a fold and an
OP_IVL_GROUP of each operator, chains under 0, 1, 2 and >= 3 transforms, the
last over a leaf and over a CSG core, an eager program with ray depth >= 3.
OP_NEVER in hit mode (top 0 and 1) cannot be emitted: emit_isect reaches a
degenerate Scaling only along the transform chain above an object's core, and
run() has by then made the whole object OBJ_NEVER (a degenerate chain has an
Empty bound).  The test holds both bins at zero, so that a compiler change
which makes them reachable has to bring a scene for them.

Pinned to the reference: tests/golden/graph.npz (make_golden.py graph) holds
the frames and ray counts of the reference's own code for every case and seed
in both modes, and its intersect / interval answers for every top-level object
of the named cases; the oracle reproduces all of it bit for bit.

Stability: with test_gpu_query.Case's ray recipe (384 camera rays, 384
surface-to-surface rays, dpi 24 for the named cases, 16 for the seeds) the
oracle-unstable rays stay within the GPU files' caps: 1 % for intersect and
occluded, 15 of 768 for radiance.  Measured: intersect and occluded 0 of 768
on all 14 cases and 6 seeds; the named cases have 443 to 765 oracle hits;
radiance 0 to 4 of 768 on the named cases, 5 to 13 on the seeds.
Every test prints its counts."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import scenes
from test_gpu_query import Case
from test_gpu_radiance import TOL, Ref

SEEDS = [2, 3, 8, 9, 10, 12]
NAMED = sorted(scenes.graph_cases())
KEYS = NAMED + [f"seed{s}" for s in SEEDS]
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph.npz")
QUERY_SEED = 20251020
_dp = C.POINTER(C.c_double)
_cases, _refs, _frames = {}, {}, {}


# ------------------------------------------------------------------ helpers
def scene_dict(key, dpi=None):
    """The scene dict of a named case (default dpi 24) or "seed<N>" (16)."""
    if key.startswith("seed"):
        return scenes.graph_scene(int(key[4:]), dpi=dpi or 16)
    return scenes.graph_cases(dpi=dpi or 24)[key]


def load(rt, key, dpi=None):
    return scenes.graph_load(rt, key, scene_dict(key, dpi))


def gold():
    return np.load(GOLD)   # data only (allow_pickle stays False)


class GraphCase(Case):
    """test_gpu_query.Case of a graph scene: its rays and the oracle's answers, computed once."""

    def __init__(self, rt, key):
        self._build(rt, load(rt, key), QUERY_SEED + KEYS.index(key), key)
        for a in (self.rays, self.seg_rays, self.ref_hit, self.ref_rec, self.ref_occ):
            a.setflags(write=False)


def graph_case(rt, key):
    if key not in _cases:
        _cases[key] = GraphCase(rt, key)
    return _cases[key]


def graph_ref(rt, key):
    """test_gpu_radiance.Ref of the case's rays (the oracle's trace of them), computed once."""
    if key not in _refs:
        c = graph_case(rt, key)
        _refs[key] = Ref(rt, c.scene, c.rays["o"], c.rays["d"])
    return _refs[key]


def oracle_frame(rt, key, mode):
    """(oracle frame, counts) of the scene at the fixture's dpi, computed once."""
    if (key, mode) not in _frames:
        sc = load(rt, key, int(gold()["dpi"]))
        fb, st = rt.oracle_render(sc, sc.width, sc.height, mode, threads=8)
        fb.setflags(write=False)
        _frames[key, mode] = (fb, (int(st.rays_intersect), int(st.rays_occluded)))
    return _frames[key, mode]


def fallback_rays(c):
    """Indices of the rays of big_scale_fallback's case whose oracle hit lies on
    the scaled sphere (its material) while their world line misses the image
    of that sphere - the ball a bound would give it: centre (0, 1e6, 0),
    radius 8e5 - passing its centre at more than its radius."""
    obj = scene_dict("big_scale_fallback")["objects"][1]["scaling"]
    s, sph = np.array(obj["factors"]), obj["subject"]["sphere"]
    centre, radius = s * np.array(sph["position"]), float(s.max()) * sph["radius"]
    mat = int(c.scene.desc.nodes[c.scene.desc.nodes[c.scene.desc.objects[1]].a].mat)
    d = c.rays["d"] / np.sqrt((c.rays["d"] ** 2).sum(axis=1))[:, None]
    w = centre - c.rays["o"]
    dist = np.sqrt(((w - (w * d).sum(axis=1)[:, None] * d) ** 2).sum(axis=1))
    return np.flatnonzero(c.ref_hit & (c.ref_rec["mat"] == mat) & (dist > radius))


# ----------------------------------------------------------------- coverage
# bins that no scene can reach: OP_NEVER in hit mode (the module docstring says why)
UNREACHABLE = ("never_top/0", "never_top/1")


def test_every_compiled_form_is_covered(rt):
    rt.amd_lib()
    total = {}
    for key in KEYS:
        forms = rt.compile_forms(load(rt, key))
        for k, v in forms.items():
            total[k] = max(total.get(k, 0), v) if k.startswith("max_") else total.get(k, 0) + v
    print("  " + ", ".join(f"{k} {v}" for k, v in total.items()))
    assert len(total) == 37
    missing = [k for k, v in total.items() if v == 0 and k not in UNREACHABLE]
    assert not missing, missing
    assert [total[k] for k in UNREACHABLE] == [0, 0]
    assert total["never_top/2"] > 0 and total["chain_m3+/leaf"] > 0 and total["chain_m3+/csg"] > 0
    assert total["max_ray_depth"] >= 3 and total["max_ivl_depth"] >= 3


def test_named_cases_compile_to_their_forms(rt):
    rt.amd_lib()
    forms = {name: rt.compile_forms(load(rt, name)) for name in NAMED}
    f = forms["never_top"]
    assert f["obj/never"] == 1 and sum(v for k, v in f.items() if k.startswith("obj/")) == 3
    assert forms["never_mid_chain"]["obj/never"] == 1 and forms["never_mid_chain"]["obj/chain"] == 0
    # union / difference keep their other operand, intersection and a degenerate left operand do not
    f = forms["never_in_csg"]
    assert (f["obj/never"], f["obj/eager"], f["never_top/2"]) == (2, 2, 2)
    assert forms["scale_threshold"]["obj/never"] == 1 and forms["scale_threshold"]["obj/chain"] == 1
    for name in NAMED:
        assert (forms[name]["obj/eager"] > 0) == (name in scenes.GRAPH_EAGER_CASES), name
    assert forms["null_mat_eager"]["op/xpush"] == 0   # (eager through the null material alone)
    f = forms["csg_self"]
    assert (f["fold/union"], f["fold/intersection"], f["fold/difference"]) == (1, 1, 1)
    assert set(scenes.GRAPH_XFORM_CASES) <= set(NAMED)


def test_scalings_the_reference_answers_off_their_image_have_no_bound(rt):
    """scene_compile.cpp xform_ball: a Scaling with a factor of 1e6 or more can
    hand its subject the (0, 1, 0) fallback direction (core.h:278), and one
    whose factors differ by more than 16 (multiplied along nested Scalings)
    makes the reference's sphere test answer for rays that miss the image by
    more than the cull margins.  The compiled object then carries no bound, no
    prefilter balls and no cull group above it, whatever stands above or below
    the Scaling; factors 9e5 (|d_local| >= 1 / 9e5 > 1e-6) and ratios up to 16
    keep them."""
    rt.amd_lib()

    def sph(x):
        return scenes._sph([x, 0.5, 0], 0.4, scenes._mat([0.9, 0.5, 0.1]))

    pair = {"union": [sph(0.0), sph(0.3)]}
    one = lambda f: (lambda sub: scenes._sc(f, sub))   # noqa: E731
    two = lambda f, g: (lambda sub: scenes._sc(f, scenes._rot(30, 1, scenes._sc(g, sub))))   # noqa: E731
    for wrap, bounded in ((one([9e5] * 3), True), (one([1e6] * 3), False), (one([-3e7, 3e7, 3e7]), False),
                          (one([1e-3] * 3), True), (one([16, 1, -1]), True), (one([17, 1, 1]), False),
                          (one([1e-6, 1, 1]), False), (one([0.1, 2, 1]), False), (two([4, 1, 1], [1, 4, 1]), True),
                          (two([4, 1, 1], [1, 5, 1]), False),
                          # (every level's ray is normalised anew: no fallback from a product of factors)
                          (two([2e3] * 3, [1e3] * 3), True)):
        for sub in (sph(0.0), pair, scenes._tr([0.1, 0, 0], sph(0.0))):
            objs = [wrap(sub), scenes._tr([0, 0, 1], wrap(sub)), {"union": [sph(2.0), wrap(sub)]}]
            f = rt.compile_forms(rt.load_scene_from_json_text(json.dumps(scenes._base(objs))))
            assert f["obj/chain"] == 2 and f["obj/eager"] == 1 and f["obj/never"] == 0
            assert f["bounded"] == (3 if bounded else 0), (wrap(0), f)
            assert f["prefilter"] == (2 if bounded and sub is pair else 0), (wrap(0), f)
            assert bounded or f["obj/group"] == 0


# ------------------------------------------------- pinned to the reference
def test_fixture_complete():
    z = gold()
    assert [int(s) for s in z["seeds"]] == SEEDS and 1 <= int(z["dpi"]) <= 24
    assert os.path.getsize(GOLD) < 1000000
    for key in KEYS:
        for mode in (0, 1):
            assert f"{key}/{mode}/fb" in z.files and f"{key}/{mode}/counts" in z.files, key
    assert {k.split("/")[0] for k in z.files} - {"dpi", "seeds"} == set(KEYS)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("key", KEYS)
def test_oracle_matches_reference_fixture(rt, key, mode):
    z = gold()
    fb, counts = oracle_frame(rt, key, mode)
    assert counts == tuple(int(v) for v in z[f"{key}/{mode}/counts"])
    assert np.array_equal(fb, z[f"{key}/{mode}/fb"], equal_nan=True)
    off_bg = int((np.abs(fb - fb[0, 0]).max(axis=2) > 0).sum())
    print(f"  {key} mode {mode}: {fb.shape[1]}x{fb.shape[0]}, counts {counts}, {off_bg} pixels differ from the corner's")


def _hit_row(h):
    return np.array([h.t, *h.p, *h.n, float(h.mat), float(h.front_face)])


@pytest.mark.parametrize("name", NAMED)
def test_oracle_matches_reference_objects(rt, name):
    """Primitive::intersect and ::interval of every top-level object's root node."""
    z, lib = gold(), rt.oracle_lib()
    sc = load(rt, name, int(z["dpi"]))
    o, d = z[f"{name}/o"], z[f"{name}/d"]
    n_hit = n_ivl = 0
    for k in range(sc.desc.n_objects):
        node = int(sc.desc.objects[k])
        ok_g, hit_g = z[f"{name}/{k}/isect/ok"], z[f"{name}/{k}/isect/hit"]
        ivl_g, rec_g = z[f"{name}/{k}/ivl/ok"], z[f"{name}/{k}/ivl/rec"]
        for i in range(len(o)):
            oi, di = np.ascontiguousarray(o[i]).ctypes.data_as(_dp), np.ascontiguousarray(d[i]).ctypes.data_as(_dp)
            h = rt.OracleHit()
            ok = lib.oracle_node_intersect(sc.desc_ptr, node, oi, di, 1e-4, float("inf"), C.byref(h))
            assert ok == ok_g[i], (name, k, "isect", i)
            if ok:
                n_hit += 1
                assert np.array_equal(_hit_row(h), hit_g[i], equal_nan=True), (name, k, "isect", i)
            t0, t1 = C.c_double(), C.c_double()
            h0, h1 = rt.OracleHit(), rt.OracleHit()
            ok = lib.oracle_node_interval(sc.desc_ptr, node, oi, di, C.byref(t0), C.byref(t1), C.byref(h0), C.byref(h1))
            assert ok == ivl_g[i], (name, k, "ivl", i)
            if ok:
                n_ivl += 1
                got = np.concatenate([[t0.value, t1.value], _hit_row(h0), _hit_row(h1)])
                assert np.array_equal(got, rec_g[i], equal_nan=True), (name, k, "ivl", i)
    print(f"  {name}: {sc.desc.n_objects} objects x {len(o)} rays, {n_hit} hits, {n_ivl} intervals")
    assert n_hit > 0 and n_ivl > 0


# ---------------------------------------------------------------- stability
@pytest.mark.parametrize("key", KEYS)
def test_oracle_queries_are_stable(rt, key):
    c = graph_case(rt, key)
    n_i = sum(c.oracle_unstable(r, False) for r in c.rays)
    n_o = sum(c.oracle_unstable(r, True) for r in c.seg_rays)
    print(f"  {key}: {int(c.ref_hit.sum())} hits, {int(c.ref_occ.sum())} occluded, oracle-unstable: intersect {n_i}, "
          f"occluded {n_o} of {len(c.rays)}")
    assert len(c.rays) == 768 and c.ref_hit.sum() >= len(c.rays) // 4 and c.ref_occ.any()
    assert n_i <= len(c.rays) // 100 and n_o <= len(c.rays) // 100


@pytest.mark.parametrize("key", KEYS)
def test_oracle_radiance_is_stable(rt, key):
    r = graph_ref(rt, key)
    n, unstable = len(r), np.zeros(len(r), dtype=bool)
    for ax in range(3):
        for sgn in (1.0, -1.0):
            o = r.o.copy()
            o[:, ax] += sgn * 1e-7
            rgb, ni, no = rt.oracle_trace(r.sc, o, r.d)
            unstable |= (np.abs(rgb - r.rgb).max(axis=1) > TOL) | (ni != r.ni) | (no != r.no)
    hits = int((np.abs(r.rgb - r.background).max(axis=1) > 0).sum())
    print(f"  {key}: {hits} of {n} rays off the background, oracle-unstable (colour at 1e-5 or counts): "
          f"{int(unstable.sum())}")
    assert np.isfinite(r.rgb).all() and hits >= n // 4
    assert int(unstable.sum()) <= n * 15 // 768


def test_big_scale_fallback_tests_the_fallback(rt):
    """At least 64 rays of the batch hit the scaled sphere although their world
    line misses its image (it passes the centre at more than the radius): the case is there
    for the (0, 1, 0) fallback of the local direction and must keep reaching it."""
    c = graph_case(rt, "big_scale_fallback")
    k = fallback_rays(c)
    print(f"  big_scale_fallback: {len(k)} of {len(c.rays)} rays hit the scaled sphere off its image")
    assert len(k) >= 64
    assert np.allclose(c.ref_rec["p"][k][:, 1], 2e5)   # the sphere's lowest point, seen from below along (0, 1, 0)
