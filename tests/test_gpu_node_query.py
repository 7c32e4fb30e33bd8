"""Batched node queries on the GPU (rt_query_node_intersect /
rt_query_node_interval and their *_device forms: Primitive::intersect and
Primitive::interval of ONE node of the scene graph, geometry.h:62-75).

References: the reference's own answers in tests/golden/kats.npz (128 rays on
every node of the ten torture scenes, intersect at two ranges and interval) and
tests/golden/graph.npz (64 rays on every top-level object of the 14 named graph
cases), which need no oracle in the loop; elsewhere the CPU oracle's
oracle_node_intersect / oracle_node_interval, which tests/test_node_query_plan.py
holds to those fixtures.

Bar (tests/test_gpu_query.py): mask, mat and front_face equal for every ray; t
and p within 1e-5 relative to max(1, |ref|), n within 1e-5 absolute; NaN for
NaN and the same infinity where the reference is non-finite (same_value).  An
interval's t is tEnter / tExit, the call's out-parameters: the fixtures' own
Hit::t column of h0 / h1 is not compared.  A ray may be left out only when the
ORACLE alone is unstable on it (its ok, mats or front faces change when the
origin moves +-1e-7 along an axis), at most 1 % per case; on the fixtures'
rays that is none (test_node_query_plan.py), so there a left-out ray fails.

Measured on an MI355X (profiles/node_queries/gpu_tests.txt): every compared
value of every test equal to the reference's, max differences 0, left out 0.
Every test prints its largest differences and its left-out count."""
import ctypes as C
import json

import numpy as np
import pytest

import scenes
from test_gpu_query import SCENES, TOL, case, q_isect, same_value
from test_leaf_scenes import odd_base_rays
from test_node_query_plan import (GRAPH_CASES, INF, ISECT, IVL, KATS_SCENES, graph, graph_case, is_leaf, isect_key,
                                  ivl_key, kats, kats_case, kernel, kind_of, load, unstable)

pytestmark = pytest.mark.gpu

RT_ERR_UNSUPPORTED = -6


# ------------------------------------------------------------------ helpers
def kats_rays(seed, n=128):
    """The fixtures' ray recipe (tests/golden/make_golden.py _random_rays):
    origins around (0, 0, 2.8), targets around (0, 0, -1.2), the first tenth
    starting inside the objects, eight axis-parallel; directions unnormalised."""
    rng = np.random.default_rng(seed)
    center, spread = np.array([0.0, 0.0, -1.2]), 1.5
    o = center + rng.normal(size=(n, 3)) * spread + np.array([0.0, 0.0, 4.0])
    d = center + rng.normal(size=(n, 3)) * spread * 0.6 - o
    o[: n // 10] = center + rng.normal(size=(n // 10, 3)) * 0.2
    d[n // 10: n // 10 + 8] = np.array([1.0, 0.0, 0.0])
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def n_isect(rt, sc, node, o, d, tmin=1e-4, tmax=INF, flags=0, stats=None):
    return rt.query_node_intersect(sc, node, o, d, tmin, tmax, flags, stats)


def n_ivl(rt, sc, node, o, d, flags=0, stats=None):
    return rt.query_node_interval(sc, node, o, d, flags, stats)


def logged(rt, fn):
    rt.launch_log(True)
    try:
        out = fn()
        rows = rt.launch_log_get()
    finally:
        rt.launch_log(False)
    return out, rows


def misses_are_zero(rec, ok):
    m = rec[~ok]
    return bool(np.all(m["mat"] == -1) and not m["t"].any() and not m["p"].any() and not m["n"].any()
                and not m["front_face"].any())


def compare(got_ok, got, ref_ok, ref, what, probe=None):
    """One record array against the reference's at the file's bar, every ray;
    probe(indices) -> which of those rays the oracle alone is unstable on
    (None: no ray may be left out).  Returns (max rel dt, max rel dp, max abs
    dn, left out) over the compared finite values."""
    assert len(got) == len(ref) == len(got_ok) == len(ref_ok)
    assert misses_are_zero(got, got_ok), what
    both = got_ok & ref_ok
    bad = got_ok != ref_ok
    bad |= both & ((got["mat"] != ref["mat"]) | (got["front_face"] != ref["front_face"]))
    bad |= both & ~(same_value(got["t"], ref["t"]) & same_value(got["p"], ref["p"]).all(axis=1)
                    & same_value(got["n"], ref["n"], relative=False).all(axis=1))
    idx = np.flatnonzero(bad)
    left = idx[probe(idx)] if (probe is not None and len(idx)) else idx[:0]
    wrong = sorted(set(idx.tolist()) - set(left.tolist()))
    keep = both.copy()
    keep[left] = False

    def largest(f, rel):
        a, b = got[f][keep].reshape(-1), ref[f][keep].reshape(-1)
        k = np.isfinite(a) & np.isfinite(b)
        return float((np.abs(a[k] - b[k]) / (np.maximum(1.0, np.abs(b[k])) if rel else 1.0)).max(initial=0.0))

    mx = (largest("t", True), largest("p", True), largest("n", False))
    assert not wrong, (what, wrong[:8], [(got[k], ref[k], bool(got_ok[k]), bool(ref_ok[k])) for k in wrong[:2]])
    assert len(left) <= len(got) // 100, (what, left)
    return mx + (len(left),)


class Tally:
    """The largest differences of one test, printed at its end."""

    def __init__(self, what):
        self.what, self.mx, self.left, self.rays, self.ok = what, np.zeros(3), 0, 0, 0

    def add(self, r, n, n_ok):
        self.mx = np.maximum(self.mx, r[:3])
        self.left += r[3]
        self.rays += n
        self.ok += n_ok

    def show(self, extra=""):
        print(f"  {self.what}: {self.rays} rays, {self.ok} hits / intervals, max rel dt={self.mx[0]:.3g} "
              f"dp={self.mx[1]:.3g} abs dn={self.mx[2]:.3g}, left out {self.left}{extra}")


def check_case(rt, sc, node, c, tally, what, strict=True):
    """Node `node` against one case in kats_case's form: intersect at the case's
    ranges, interval.  strict: the case's rays are known to be oracle-stable
    (the fixtures'), so none may be left out; else the probe decides."""
    o, d = c["o"], c["d"]
    for tag in ("isect", "isect_win"):
        if tag not in c:
            continue
        (tmin, tmax), ref_ok, ref = c[tag]
        got = n_isect(rt, sc, node, o, d, tmin, tmax)
        probe = None if strict else (lambda i, a=tmin, b=tmax: unstable(lambda p: isect_key(rt, sc, node, p, d[i], a, b), o[i]))
        tally.add(compare(got.hit, got.records, ref_ok, ref, f"{what} {tag}", probe), len(o), int(ref_ok.sum()))
    ref_ok, ref_enter, ref_exit = c["ivl"]
    enter, ex, ok = n_ivl(rt, sc, node, o, d)
    probe = None if strict else (lambda i: unstable(lambda p: ivl_key(rt, sc, node, p, d[i]), o[i]))
    tally.add(compare(ok, enter, ref_ok, ref_enter, f"{what} enter", probe), len(o), int(ref_ok.sum()))
    tally.add(compare(ok, ex, ref_ok, ref_exit, f"{what} exit", probe), 0, 0)
    return enter, ex, ok


def oracle_case(rt, sc, node, o, d, ranges=((1e-4, INF),)):
    """The oracle's answers for rays (o, d) on a node, in kats_case's form."""
    c = {"o": o, "d": d}
    for tag, (tmin, tmax) in zip(("isect", "isect_win"), ranges):
        hit, rec = rt.oracle_node_intersect(sc, node, o, d, tmin, tmax)
        c[tag] = ((tmin, tmax), hit, rec)
    enter, ex, ok = rt.oracle_node_interval(sc, node, o, d)
    c["ivl"] = (ok, enter, ex)
    return c


# ------------------------------------------------- the reference's own answers
_seen = {"inf_end": 0, "inside": 0, "flipped": 0}


def _difference_nodes(sc):
    return [n for n in range(sc.desc.n_nodes) if kind_of(sc, n) == 6 and int(sc.desc.nodes[n].op) == 2]


@pytest.mark.parametrize("sname", KATS_SCENES)
def test_every_node_of_the_torture_scenes_is_the_reference(gpu, sname):
    z = kats()
    sc = gpu.load_scene_from_json_text(bytes(z[f"{sname}/scene"]).decode())
    tally = Tally(sname)
    diff = set(_difference_nodes(sc))

    def odd(node, ok, enter, ex):
        """(intervals with an infinite end, origin-inside entries, re-faced entries) of one node's records.  A
        difference entered through its subtrahend's far wall (csg.cpp:139-150) is the one entry with front_face 0."""
        return np.array([int((np.isinf(enter["t"][ok]) | np.isinf(ex["t"][ok])).sum()),
                         int((ok & (enter["n"] == 0).all(axis=1)).sum()),
                         int((ok & (enter["front_face"] == 0)).sum()) if node in diff else 0])

    seen, want = np.zeros(3, dtype=int), np.zeros(3, dtype=int)
    for node in range(sc.desc.n_nodes):
        c = kats_case(gpu, z, sname, node)
        enter, ex, ok = check_case(gpu, sc, node, c, tally, f"{sname} node {node}")
        seen += odd(node, ok, enter, ex)                                # (the device's own, checked, output)
        want += odd(node, c["ivl"][0], c["ivl"][1], c["ivl"][2])        # (the fixture)
    tally.show(f"; {sc.desc.n_nodes} nodes, {seen[0]} intervals with an infinite end, {seen[1]} origin-inside "
               f"entries, {seen[2]} re-faced entries of a difference")
    assert list(seen) == list(want)
    for k, v in zip(("inf_end", "inside", "flipped"), seen):
        _seen[k] += int(v)
    assert tally.ok > 0 and tally.left == 0


def test_the_run_saw_the_odd_intervals(gpu):
    """Over the ten torture scenes (the test above, which holds each scene's
    counts to the fixture's): intervals with an infinite end, origin-inside
    entries (n == 0) and re-faced entries of a difference all occurred."""
    if not any(_seen.values()):   # (run alone: make the counts)
        for sname in KATS_SCENES:
            test_every_node_of_the_torture_scenes_is_the_reference(gpu, sname)
    print(f"  seen over {len(KATS_SCENES)} scenes: {_seen}")
    assert _seen["inf_end"] > 0 and _seen["inside"] > 0 and _seen["flipped"] > 0


@pytest.mark.parametrize("name", GRAPH_CASES)
def test_every_object_of_the_graph_cases_is_the_reference(gpu, name):
    z = graph()
    sc = scenes.graph_load(gpu, name, scenes.graph_cases(dpi=int(z["dpi"]))[name])
    tally = Tally(name)
    nonfinite = 0
    for k in range(sc.desc.n_objects):
        c = graph_case(gpu, z, name, k)
        check_case(gpu, sc, int(sc.desc.objects[k]), c, tally, f"{name} object {k}")
        ok, enter, ex = c["ivl"]
        nonfinite += int((ok & ~(np.isfinite(enter["t"]) & np.isfinite(ex["t"]))).sum())
    tally.show(f"; {sc.desc.n_objects} objects, {nonfinite} intervals with a non-finite t")
    assert tally.ok > 0 and tally.left == 0


# ------------------------------------------------------ leaves and odd rays
_leaf_refs = {}


def _leaf_ref(rt, key):
    """Every node of a leaf case with 128 rays of the kats recipe and the oracle's answers, computed once."""
    if key not in _leaf_refs:
        sc = rt.load_scene_from_json_text(json.dumps(scenes.leaf_cases()[key]))
        o, d = kats_rays(20251020 + sorted(scenes.leaf_cases()).index(key))
        _leaf_refs[key] = (sc, [oracle_case(rt, sc, node, o, d) for node in range(sc.desc.n_nodes)])
    return _leaf_refs[key]


@pytest.mark.parametrize("key", sorted(scenes.leaf_cases()))
def test_every_node_of_the_leaf_cases(gpu, key):
    """Negative, zero, 1e-7 and 1e6 radii, degenerate half-space normals, the
    pokeball's parameter edges: every node, leaves and the CSG / transform nodes
    above them."""
    sc, refs = _leaf_ref(gpu, key)
    tally = Tally(key)
    rows = set()
    for node, c in enumerate(refs):
        _, r = logged(gpu, lambda: check_case(gpu, sc, node, c, tally, f"{key} node {node}", strict=False))
        rows |= set(r)
        assert all(("<false>" in x) == is_leaf(sc, node) for x in r), (key, node, r)
    tally.show(f"; {sc.desc.n_nodes} nodes, rows {sorted(rows)}")
    assert tally.ok > 0


ODD_SCENE = "torture/xform_in_csg"


def _odd_nodes(sc):
    """One sphere, one half-space, one CSG (a difference with a transformed half-space) and one transformed node."""
    d = sc.desc
    sph = next(n for n in range(d.n_nodes) if kind_of(sc, n) == 0)
    half = next(n for n in range(d.n_nodes) if kind_of(sc, n) == 1)
    csg = next(n for n in range(d.n_nodes) if kind_of(sc, n) == 6 and int(d.nodes[n].op) == 2)
    xf = next(n for n in range(d.n_nodes) if kind_of(sc, n) == 5)   # a rotation over a scaling over a sphere
    return {"sphere": sph, "halfspace": half, "csg": csg, "transformed": xf}


def _interleave(a, b):
    m = min(len(a), len(b))
    mix = np.empty((2 * m,) + a.shape[1:], dtype=a.dtype)
    mix[0::2], mix[1::2] = a[:m], b[:m]
    return mix, m


@pytest.mark.parametrize("which", ["sphere", "halfspace", "csg", "transformed"])
def test_odd_rays(gpu, which):
    """scenes.odd_ray_groups (a NaN or an infinity in o, d, tmin or tmax, a
    direction that overflows, underflows or sits at the 1e-6 edge) on one node
    of each kind: the reference's answer for every ray, alone and interleaved
    lane by lane with ordinary rays, whose bytes are those of the batch without
    the odd ones."""
    sc = gpu.load_scene_from_json_text(json.dumps(scenes.torture_scenes(dpi=24)[ODD_SCENE[8:]]))
    node = _odd_nodes(sc)[which]
    po, pd = kats_rays(77, 64)
    plain = n_isect(gpu, sc, node, po, pd)
    plain_ivl = n_ivl(gpu, sc, node, po, pd)
    tally = Tally(f"{ODD_SCENE} {which} node {node}")
    nonfinite = 0
    for tag, (o, d, tmin, tmax) in scenes.odd_ray_groups(*odd_base_rays(gpu, sc)).items():
        what = f"{which} {tag}"
        hit, rec = gpu.oracle_node_intersect(sc, node, o, d, tmin, tmax)
        got = n_isect(gpu, sc, node, o, d, tmin, tmax)
        tally.add(compare(got.hit, got.records, hit, rec, what + " isect"), len(o), int(hit.sum()))
        ref_enter, ref_exit, ref_ok = gpu.oracle_node_interval(sc, node, o, d)
        enter, ex, ok = n_ivl(gpu, sc, node, o, d)
        tally.add(compare(ok, enter, ref_ok, ref_enter, what + " enter"), len(o), int(ref_ok.sum()))
        tally.add(compare(ok, ex, ref_ok, ref_exit, what + " exit"), 0, 0)
        nonfinite += int((hit & ~np.isfinite(rec["t"])).sum()) + int((ref_ok & ~np.isfinite(ref_enter["t"])).sum())
        nc = n_isect(gpu, sc, node, o, d, tmin, tmax, flags=gpu.RT_FLAG_NO_CULL)
        assert nc.records.tobytes() == got.records.tobytes() and np.array_equal(nc.hit, got.hit), what
        # interleaved with ordinary rays, lane by lane
        mo, m = _interleave(o, po)
        md, _ = _interleave(d, pd)
        mtmin, _ = _interleave(tmin, np.full(64, 1e-4))
        mtmax, _ = _interleave(tmax, np.full(64, INF))
        both = n_isect(gpu, sc, node, mo, md, mtmin, mtmax)
        assert both.records[0::2].tobytes() == got.records[:m].tobytes() and np.array_equal(both.hit[0::2], got.hit[:m]), what
        assert both.records[1::2].tobytes() == plain.records[:m].tobytes() and np.array_equal(both.hit[1::2], plain.hit[:m]), what
        be, bx, bok = n_ivl(gpu, sc, node, mo, md)
        for mixed, odd, ordinary in ((be, enter, plain_ivl[0]), (bx, ex, plain_ivl[1]), (bok, ok, plain_ivl[2])):
            assert mixed[0::2].tobytes() == odd[:m].tobytes() and mixed[1::2].tobytes() == ordinary[:m].tobytes(), what
    tally.show(f"; {nonfinite} reference answers with a non-finite t")
    assert plain.hit.any() or plain_ivl[2].any()


# ---------------------------------------------------------------- big stacks
@pytest.mark.parametrize("name", ["deep/xform_nest12", "deep/csg_right12"])
def test_big_stack_nodes(gpu, name):
    """The 12-transform chain (and the CSG above it) and the right-nested CSG of
    12 leaves: their own programs need the big stacks; nodes further down take
    the common ones, leaves the leaf rows."""
    sc = load(gpu, name)
    tally = Tally(name)
    big = 0
    o, d = kats_rays(31 + len(name))
    for node in range(sc.desc.n_nodes):
        want = (kernel(gpu, sc, node, ISECT), kernel(gpu, sc, node, IVL))
        if is_leaf(sc, node) and node > 2:
            continue   # (the leaves: three of them stand for all)
        c = oracle_case(gpu, sc, node, o, d, ((1e-4, INF), (0.5, 4.0)))
        _, rows = logged(gpu, lambda: check_case(gpu, sc, node, c, tally, f"{name} node {node}", strict=False))
        assert rows == [want[0], want[0], want[1]], (name, node, rows)
        big += want[1].startswith("rtdb::")
    tally.show(f"; {big} nodes on rtdb rows")
    assert big >= 4 and tally.ok > 0


def test_a_node_beyond_the_big_stacks_is_refused_before_any_launch(gpu):
    obj = scenes._sph([0, 0, -1], 0.5, scenes._mat([1, 1, 1]))
    for k in range(70):
        obj = scenes._tr([0.001 * k, 0, 0], obj)
    sc = gpu.load_scene_from_json_text(json.dumps(scenes._base([obj])))
    root = int(sc.desc.objects[0])
    o, d = kats_rays(5, 8)

    def refused():
        for fn in (lambda: n_isect(gpu, sc, root, o, d), lambda: n_ivl(gpu, sc, root, o, d)):
            with pytest.raises(gpu.RTError) as e:
                fn()
            assert e.value.code == RT_ERR_UNSUPPORTED and "transform nesting inside CSG operands 70" in str(e.value)

    _, rows = logged(gpu, refused)
    assert rows == []
    # the scene itself renders and answers scene queries (a stackless chain), and a node 64 levels down is served
    hit, rec = gpu.oracle_node_intersect(sc, root, o, d)
    got = gpu.query_intersect(sc, o, d)
    compare(got.hit, got.records, hit, rec, "chain70 scene query")
    node = root
    for _ in range(6):
        node = int(sc.desc.nodes[node].a)
    got, rows = logged(gpu, lambda: n_isect(gpu, sc, node, o, d))
    assert rows == ["rtdb::k_node_isect<true>"]
    compare(got.hit, got.records, *gpu.oracle_node_intersect(sc, node, o, d), "chain70 node 64 levels deep")


# ------------------------------------------------------------------- census
@pytest.mark.parametrize("recipe", scenes.node_recipes(), ids=lambda r: r.row)
def test_every_row_runs_and_matches_the_oracle(gpu, recipe):
    sc = load(gpu, recipe.scene_name)
    node = int(sc.desc.objects[recipe.obj])
    o, d = kats_rays(11)
    c = oracle_case(gpu, sc, node, o, d)
    tally = Tally(recipe.row)
    _, rows = logged(gpu, lambda: check_case(gpu, sc, node, c, tally, recipe.row, strict=False))
    tally.show(f"; rows {rows}")
    assert rows[0 if recipe.kind == ISECT else 1] == recipe.row


# --------------------------------------- consistency with the scene queries
def _only_object(rt, sc, node):
    """The scene whose only object is node `node` of sc (rt_scene_from_desc)."""
    d = rt.SceneDesc.from_buffer_copy(sc.desc)
    objs = (C.c_int32 * 1)(node)
    d.objects = C.cast(objs, type(d.objects))
    d.n_objects = 1
    return rt.scene_from_desc(d)


def _largest_csg_object(rt, sc):
    """The top-level object with the longest program among those that hold a CSG (config 4: the snorlax's body,
    transforms over a CSG tree)."""
    d = sc.desc
    progs = {int(d.objects[k]): rt.node_program(sc, int(d.objects[k]), IVL)[0] for k in range(d.n_objects)}
    return max((n for n, ops in progs.items() if any(o[0] == "csg" for o in ops)), key=lambda n: len(progs[n]))


def _csg_core(sc, node):
    """The CSG node under the transforms of `node`."""
    while kind_of(sc, node) in (3, 4, 5):
        node = int(sc.desc.nodes[node].a)
    assert kind_of(sc, node) == 6
    return node


def _consistency_nodes(rt, name, sc):
    d = sc.desc
    if name == "config4":
        return [_largest_csg_object(rt, sc)]
    return [int(d.objects[k]) for k in range(d.n_objects)]


@pytest.mark.parametrize("name", ["torture/csg_ops", "torture/xform_in_csg", "config4"])
def test_node_intersect_is_the_scene_query_of_a_one_object_scene(gpu, name):
    """rt_query_intersect on the scene whose only object is node k - the frames'
    path: a bare leaf, a compact chain or an eager object - and
    rt_query_node_intersect(k) on the original scene: the same bytes on the
    768 rays of tests/test_gpu_query.py."""
    c = case(gpu, name)
    for node in _consistency_nodes(gpu, name, c.scene):
        one = _only_object(gpu, c.scene, node)
        want = q_isect(gpu, one, c.rays)
        got = n_isect(gpu, c.scene, node, c.rays["o"], c.rays["d"], c.rays["tmin"], c.rays["tmax"])
        forms = {k: v for k, v in gpu.compile_forms(one).items() if k.startswith("obj/") and v}
        print(f"  {name} node {node}: {int(want.hit.sum())} of {len(c.rays)} rays hit, one-object scene {forms}")
        assert len(c.rays) == 768 and want.hit.any()
        assert got.records.tobytes() == want.records.tobytes() and np.array_equal(got.hit, want.hit), (name, node)


# ------------------------------------------- intersect derives from interval
@pytest.mark.parametrize("name", ["torture/csg_ops", "torture/xform_in_csg", "config4"])
def test_csg_intersect_derives_from_interval(gpu, name):
    """CSG::intersect (csg.cpp:169-185): hit == ok && max(t0, tmin) < t1 &&
    max(t0, tmin) < tmax, at t = that max, with the enter record's n, mat and
    front_face and p = o + t d."""
    sc = case(gpu, name).scene
    nodes = [n for n in range(sc.desc.n_nodes) if kind_of(sc, n) == 6]
    if name == "config4":
        nodes = [_csg_core(sc, _largest_csg_object(gpu, sc))]
    o, d = kats_rays(3 + len(name))
    hits = 0
    for node in nodes:
        enter, ex, ok = n_ivl(gpu, sc, node, o, d)
        for tmin, tmax in ((1e-4, INF), (0.5, 4.0)):
            got = n_isect(gpu, sc, node, o, d, tmin, tmax)
            t = np.where(enter["t"] < tmin, tmin, enter["t"])   # std::max(t0, tmin)
            want = ok & (t < ex["t"]) & (t < tmax)
            assert np.array_equal(got.hit, want), (name, node, tmin, np.flatnonzero(got.hit != want))
            assert np.array_equal(got.t[want], t[want])
            for f in ("n", "mat", "front_face"):
                assert np.array_equal(got.records[f][want], enter[f][want]), (name, node, f)
            hits += int(want.sum())
    print(f"  {name}: {len(nodes)} CSG nodes x {len(o)} rays x 2 ranges, {hits} hits")
    assert hits > 0


# ---------------------------------------------------------------- mechanics
def _mech(gpu):
    """A CSG node with transforms in its operands and a batch with hits, misses and intervals."""
    sc = case(gpu, "torture/xform_in_csg").scene
    node = int(sc.desc.objects[1])
    return sc, node


def _dev_run(rt, sc, node, rays, n, cap, stream=None, flags=0, outputs=(True, True, True), kind=IVL):
    """The *_device form on the first n rays into buffers of cap records filled
    with 0xAB; outputs: which of (enter / hits, exit, mask) are given."""
    d_rays = rt.DeviceBuffer(max(1, len(rays)) * 64)
    d_rays.from_host(rays)
    bufs = []
    for given, size in zip(outputs, (cap * 64, cap * 64, cap)):
        b = rt.DeviceBuffer(size) if given else None
        if b is not None:
            b.from_host(np.full(size, 0xAB, dtype=np.uint8))
        bufs.append(b)
    st = rt.Stats()
    if kind == IVL:
        rt.query_node_interval_device(sc, node, d_rays, n, bufs[0], bufs[1], bufs[2], flags, stream, st)
    else:
        rt.query_node_intersect_device(sc, node, d_rays, n, bufs[0], bufs[2], flags, stream, st)
    return [b.to_host(np.uint8) if b is not None else None for b in bufs], st


def _rays_of(rt, n, seed=9):
    o, d = kats_rays(seed, max(n, 16))
    return rt.make_rays(o[:n], d[:n], 0.5, 40.0)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_wave_tails(gpu, n):
    sc, node = _mech(gpu)
    rays = _rays_of(gpu, n)
    hits = n_isect(gpu, sc, node, rays["o"], rays["d"], rays["tmin"], rays["tmax"])
    enter, ex, ok = n_ivl(gpu, sc, node, rays["o"], rays["d"])
    ref_hit, ref_rec = gpu.oracle_node_intersect(sc, node, rays["o"], rays["d"], 0.5, 40.0)
    compare(hits.hit, hits.records, ref_hit, ref_rec, f"n={n}")
    cap = n + 200
    (e_b, x_b, m_b), st = _dev_run(gpu, sc, node, rays, n, cap)
    assert (st.rays_intersect, st.rays_occluded, st.rays_traced, st.pixels, st.n_gpus) == (n, 0, n, 0, 1)
    assert e_b[:n * 64].tobytes() == enter.tobytes() and x_b[:n * 64].tobytes() == ex.tobytes()
    assert np.array_equal(m_b[:n], ok.astype(np.uint8))
    assert np.all(e_b[n * 64:] == 0xAB) and np.all(x_b[n * 64:] == 0xAB) and np.all(m_b[n:] == 0xAB)
    (h_b, _, m_b), st = _dev_run(gpu, sc, node, rays, n, cap, kind=ISECT, outputs=(True, False, True))
    assert (st.rays_intersect, st.rays_occluded, st.rays_traced) == (n, 0, n)
    assert h_b[:n * 64].tobytes() == hits.records.tobytes() and np.array_equal(m_b[:n], hits.hit.astype(np.uint8))
    assert np.all(h_b[n * 64:] == 0xAB) and np.all(m_b[n:] == 0xAB)
    if n == 1000:
        assert ok.any() and not ok.all() and hits.hit.any()


def test_device_forms_on_a_stream_with_optional_outputs(gpu):
    sc, node = _mech(gpu)
    n = 300
    rays = _rays_of(gpu, n)
    enter, ex, ok = n_ivl(gpu, sc, node, rays["o"], rays["d"])
    hits = n_isect(gpu, sc, node, rays["o"], rays["d"], rays["tmin"], rays["tmax"])
    stream = gpu.Stream()
    try:
        for outputs in ((True, True, True), (True, False, False), (False, True, False), (False, False, True),
                        (True, False, True)):
            (e_b, x_b, m_b), _ = _dev_run(gpu, sc, node, rays, n, n, stream=stream, outputs=outputs)
            assert e_b is None or e_b.tobytes() == enter.tobytes()
            assert x_b is None or x_b.tobytes() == ex.tobytes()
            assert m_b is None or np.array_equal(m_b, ok.astype(np.uint8))
        (h_b, _, m_b), _ = _dev_run(gpu, sc, node, rays, n, n, stream=stream, kind=ISECT, outputs=(True, False, False))
        assert h_b.tobytes() == hits.records.tobytes() and m_b is None
    finally:
        stream.destroy()
    # the host forms' optional outputs
    lib = gpu.amd_lib()
    a, m = np.zeros(n, dtype=gpu.HIT_DTYPE), np.zeros(n, dtype=np.uint8)
    rp = rays.ctypes.data_as(C.c_void_p)
    assert lib.rt_query_node_interval(sc.handle, node, rp, n, 0, None, a.ctypes.data_as(C.c_void_p), None, None) == 0
    assert a.tobytes() == ex.tobytes()
    assert lib.rt_query_node_interval(sc.handle, node, rp, n, 0, None, None, m.ctypes.data_as(C.c_void_p), None) == 0
    assert np.array_equal(m, ok.astype(np.uint8))
    assert lib.rt_query_node_intersect(sc.handle, node, rp, n, 0, a.ctypes.data_as(C.c_void_p), None, None) == 0
    assert a.tobytes() == hits.records.tobytes()


def test_small_host_chunks_and_no_cull_and_stats(gpu):
    """The host forms' chunk forced to 100 rays: 1000 rays cross ten chunks, each
    ending in a partial wave; the same bytes and stats as at the default chunk.
    RT_FLAG_NO_CULL, NO_BVH and FORCE_BVH: the same bytes."""
    sc, node = _mech(gpu)
    n = 1000
    rays = _rays_of(gpu, n)

    def run(flags=0):
        si, sv = gpu.Stats(), gpu.Stats()
        hits = n_isect(gpu, sc, node, rays["o"], rays["d"], rays["tmin"], rays["tmax"], flags, si)
        enter, ex, ok = n_ivl(gpu, sc, node, rays["o"], rays["d"], flags, sv)
        for s in (si, sv):
            assert s.ms_kernel > 0.0 and s.ms_total >= s.ms_kernel
        return (hits.records.tobytes(), hits.hit.tobytes(), enter.tobytes(), ex.tobytes(), ok.tobytes(),
                [(s.rays_intersect, s.rays_occluded, s.rays_traced, s.pixels, s.n_gpus) for s in (si, sv)])

    want, rows = logged(gpu, run)
    assert rows == ["rtd::k_node_isect<true>", "rtd::k_node_ivl<true>"]
    assert want[5] == [(n, 0, n, 0, 1)] * 2
    gpu.camera_chunk_rays(100)
    try:
        got, rows = logged(gpu, run)
    finally:
        gpu.camera_chunk_rays(0)
    assert rows == ["rtd::k_node_isect<true>"] * 10 + ["rtd::k_node_ivl<true>"] * 10
    assert got == want
    for f in (gpu.RT_FLAG_NO_CULL, gpu.RT_FLAG_NO_BVH, gpu.RT_FLAG_FORCE_BVH):
        assert run(f) == want, f


def test_errors_on_the_device_path(gpu):
    """The flags are refused with a launchable batch too, and an error leaves the next call working."""
    sc, node = _mech(gpu)
    rays = _rays_of(gpu, 64)
    for flag, word in ((gpu.RT_FLAG_FP32, "FP32"), (gpu.RT_FLAG_COUNT_OPS, "COUNT_OPS")):
        with pytest.raises(gpu.RTError) as e:
            n_ivl(gpu, sc, node, rays["o"], rays["d"], flag)
        assert e.value.code == RT_ERR_UNSUPPORTED and word in str(e.value)
    with pytest.raises(gpu.RTError):
        n_ivl(gpu, sc, sc.desc.n_nodes, rays["o"], rays["d"])
    enter, ex, ok = n_ivl(gpu, sc, node, rays["o"], rays["d"])
    compare(ok, enter, *[gpu.oracle_node_interval(sc, node, rays["o"], rays["d"])[k] for k in (2, 0)], "after errors")


# ---------------------------------------------------------------- residency
def test_node_queries_share_the_resident_scene(gpu):
    """On a fresh handle: a node query, a frame, a scene query, the same node
    query and another node.  rt_setup_times[0] grows at most at the first use
    of the scene and of each new node, not at the repeat; the frame matches
    the oracle with equal counts; both repeats are byte-equal."""
    lib = gpu.amd_lib()
    c = case(gpu, "config4")
    sc = gpu.load_scene_from_json_text(SCENES["config4"][0])   # a handle no frame or query has seen
    node, other = _largest_csg_object(gpu, sc), int(sc.desc.objects[1])
    o, d = c.rays["o"], c.rays["d"]
    t = (C.c_double * 4)()

    def scene_ms():
        assert lib.rt_setup_times(t, 4) == 0
        return t[0]

    ms0 = scene_ms()
    (e1, x1, k1), rows = logged(gpu, lambda: n_ivl(gpu, sc, node, o, d))
    ms1 = scene_ms()
    assert ms1 > ms0 and rows == ["rtd::k_node_ivl<true>"]
    W, H = sc.width, sc.height
    st = gpu.Stats()
    fb = gpu.Tracer(sc, W, H, 0).render(st)
    q1 = q_isect(gpu, sc, c.rays)
    assert scene_ms() == ms1   # (the frame and the scene query found the scene resident)
    e2, x2, k2 = n_ivl(gpu, sc, node, o, d)
    assert scene_ms() == ms1   # (and the repeat its program)
    h1 = n_isect(gpu, sc, node, o, d)
    ms2 = scene_ms()           # (the intersect program of the same node is a new program)
    e3, x3, k3 = n_ivl(gpu, sc, other, o, d)
    ms3 = scene_ms()
    assert ms3 >= ms2 >= ms1
    h2 = n_isect(gpu, sc, node, o, d)
    e4, x4, k4 = n_ivl(gpu, sc, other, o, d)
    fb2 = gpu.Tracer(sc, W, H, 0).render()
    q2 = q_isect(gpu, sc, c.rays)
    assert scene_ms() == ms3
    ref, ost = gpu.oracle_render(sc, W, H, 0, threads=8)
    assert float(np.abs(fb - ref).max()) <= TOL
    assert (st.rays_intersect, st.rays_occluded) == (ost.rays_intersect, ost.rays_occluded)
    assert np.array_equal(fb, fb2)
    assert q1.records.tobytes() == q2.records.tobytes() and np.array_equal(q1.hit, q2.hit)
    assert e1.tobytes() == e2.tobytes() and x1.tobytes() == x2.tobytes() and np.array_equal(k1, k2)
    assert e3.tobytes() == e4.tobytes() and x3.tobytes() == x4.tobytes() and np.array_equal(k3, k4)
    assert h1.records.tobytes() == h2.records.tobytes() and np.array_equal(h1.hit, h2.hit)
    ref_enter, ref_exit, ref_ok = gpu.oracle_node_interval(sc, node, o, d)
    r = compare(k1, e1, ref_ok, ref_enter, "config4 largest CSG enter (fresh handle)")
    compare(k1, x1, ref_ok, ref_exit, "config4 largest CSG exit (fresh handle)")
    print(f"  config4 node {node}: {int(ref_ok.sum())} intervals of {len(o)} rays, max {r[:3]}, "
          f"setup ms {ms0:.3f} -> {ms1:.3f} -> {ms2:.3f} -> {ms3:.3f}")
    assert ref_ok.any()
    # another scene evicts the programs with the scene; coming back compiles them again, same bytes
    other_sc = case(gpu, "torture/csg_ops").scene
    n_ivl(gpu, other_sc, int(other_sc.desc.objects[1]), o[:64], d[:64])
    e5, x5, k5 = n_ivl(gpu, sc, node, o, d)
    assert e5.tobytes() == e1.tobytes() and x5.tobytes() == x1.tobytes() and np.array_equal(k5, k1)


# -------------------------------------------------------------- composition
def test_enter_records_are_shaded_as_they_are(gpu):
    """rt_query_node_interval_device's enter records and ok mask straight into
    rt_query_shade_device: shade_lambert_phong of the same records by the
    oracle; rays whose interval is false get the miss colour."""
    c = case(gpu, "config4")
    sc = c.scene
    node = _largest_csg_object(gpu, sc)
    n = len(c.rays)
    dn = c.rays["d"] / np.sqrt((c.rays["d"] ** 2).sum(axis=1))[:, None]
    wo = np.ascontiguousarray(-dn)
    miss = (0.25, 0.5, 0.75)
    d_rays, d_enter, d_mask = gpu.DeviceBuffer(n * 64), gpu.DeviceBuffer(n * 64), gpu.DeviceBuffer(n)
    d_wo, d_rgb = gpu.DeviceBuffer(n * 24), gpu.DeviceBuffer(n * 24)
    d_rays.from_host(c.rays)
    d_wo.from_host(wo)
    gpu.query_node_interval_device(sc, node, d_rays, n, d_enter, None, d_mask)
    gpu.query_shade_device(sc, d_enter, d_wo, d_mask, n, d_rgb, miss_rgb=miss)
    rgb = d_rgb.to_host(np.float64, (n, 3))
    enter = d_enter.to_host(np.uint8).view(gpu.HIT_DTYPE)
    ok = d_mask.to_host(np.uint8).astype(bool)
    ref_enter, _, ref_ok = gpu.oracle_node_interval(sc, node, c.rays["o"], c.rays["d"])
    compare(ok, enter, ref_ok, ref_enter, "config4 largest CSG enter")
    want, _ = gpu.oracle_shade(sc, ref_enter, wo)
    err = float(np.abs(rgb[ok] - want[ok]).max())
    inside = int((ok & (enter["n"] == 0).all(axis=1)).sum())
    print(f"  config4 node {node}: {int(ok.sum())} of {n} enter records shaded ({inside} origin-inside), max|d|={err:.3g}")
    assert ok.sum() >= 64 and not ok.all()
    assert same_value(rgb[ok], want[ok], TOL, relative=False).all()
    assert np.array_equal(rgb[~ok], np.tile(miss, (int((~ok).sum()), 1)))
