"""Node queries on the CPU (no device is touched): a node's own program
(scene_compile.cpp compile_node_program through rt_test_node_program), the
kernel a node query launches (frame_plan.cpp pick_node_variant + the node table
of rt_node_kernels.hpp through rt_test_node_kernel_name), the census list
scenes.node_recipes() against the tables, the argument checks of
rt_query_node_intersect / rt_query_node_interval that come before any device
work, and the reference data the GPU tests use: the oracle's
oracle_node_intersect / oracle_node_interval reproduce tests/golden/kats.npz
and graph.npz, and none of those rays is one the oracle alone is unstable on.
The kernels' results are checked by tests/test_gpu_node_query.py, which
imports this file's helpers."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import scenes
from conftest import GOLDEN

RT_ERR_INVALID_ARG, RT_ERR_UNSUPPORTED = -1, -6
ISECT, IVL = 0, 1
INF = float("inf")


# ------------------------------------------------------------------ helpers
def load(rt, name):
    text, lights = scenes.recipe_scene(name)
    sc = rt.load_scene_from_json_text(text)
    return rt.with_dir_lights(sc, lights) if lights else sc


def scene_of(rt, objects):
    return rt.load_scene_from_json_text(json.dumps(scenes._base(objects)))


def kind_of(sc, node):
    return int(sc.desc.nodes[node].kind)


def is_leaf(sc, node):
    return kind_of(sc, node) in (0, 1, 2)   # RT_NODE_SPHERE / HALFSPACE / POKEBALL


def kernel(rt, sc, node, kind, flags=0):
    rc, name = rt.node_kernel_name(sc, node, kind, flags)
    assert rc == 0, rt.last_error()
    return name


def hit_records(rt, rows):
    """The fixtures' hit rows (t, p, n, mat, front_face as floats) as an rt_hit array."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 9)
    rec = np.zeros(len(rows), dtype=rt.HIT_DTYPE)
    rec["t"], rec["p"], rec["n"] = rows[:, 0], rows[:, 1:4], rows[:, 4:7]
    rec["mat"], rec["front_face"] = rows[:, 7].astype(np.int32), rows[:, 8].astype(np.int32)
    return rec


def kats():
    return np.load(os.path.join(GOLDEN, "kats.npz"))


def graph():
    return np.load(os.path.join(GOLDEN, "graph.npz"))


KATS_SCENES = sorted(scenes.torture_scenes())
GRAPH_CASES = sorted(scenes.graph_cases())


def kats_case(rt, z, sname, node):
    """One (scene, node) case of kats.npz: rays and the reference's answers, as
    the node queries report them (interval t = the out-parameters; the
    records' own t column is not compared)."""
    p = f"{sname}/{node}/"
    c = {"o": z[p + "o"], "d": z[p + "d"]}
    for tag in ("isect", "isect_win"):
        c[tag] = (tuple(float(v) for v in z[p + tag + "/range"]), z[p + tag + "/ok"].astype(bool),
                  hit_records(rt, z[p + tag + "/hit"]))
    ok = z[p + "ivl/ok"].astype(bool)
    enter, ex = hit_records(rt, z[p + "ivl/h0"]), hit_records(rt, z[p + "ivl/h1"])
    enter["t"], ex["t"] = z[p + "ivl/t"][:, 0], z[p + "ivl/t"][:, 1]
    c["ivl"] = (ok, enter, ex)
    return c


def graph_case(rt, z, name, k):
    """One (case, top-level object) of graph.npz, in kats_case's form (one range)."""
    p = f"{name}/{k}/"
    c = {"o": z[f"{name}/o"], "d": z[f"{name}/d"]}
    c["isect"] = ((1e-4, INF), z[p + "isect/ok"].astype(bool), hit_records(rt, z[p + "isect/hit"]))
    rec = z[p + "ivl/rec"]
    enter, ex = hit_records(rt, rec[:, 2:11]), hit_records(rt, rec[:, 11:20])
    enter["t"], ex["t"] = rec[:, 0], rec[:, 1]
    c["ivl"] = (z[p + "ivl/ok"].astype(bool), enter, ex)
    return c


def same_records(a, b, ok, t_too=True):
    """Bit for bit (NaN equal to NaN) where ok."""
    fields = ("t", "p", "n", "mat", "front_face") if t_too else ("p", "n", "mat", "front_face")
    return all(np.array_equal(a[f][ok], b[f][ok], equal_nan=f in ("t", "p", "n")) for f in fields)


def isect_key(rt, sc, node, o, d, tmin, tmax):
    hit, rec = rt.oracle_node_intersect(sc, node, o, d, tmin, tmax)
    return np.stack([hit, np.where(hit, rec["mat"], -1), np.where(hit, rec["front_face"], 0)], axis=1)


def ivl_key(rt, sc, node, o, d):
    enter, ex, ok = rt.oracle_node_interval(sc, node, o, d)
    return np.stack([ok, np.where(ok, enter["mat"], -1), np.where(ok, ex["mat"], -1),
                     np.where(ok, enter["front_face"], 0), np.where(ok, ex["front_face"], 0)], axis=1)


def unstable(key, o, step=1e-7):
    """Rays whose oracle answer (ok, mats, front faces) changes when the origin
    moves +-step along an axis: key(o) -> one row per ray."""
    base = key(o)
    out = np.zeros(len(o), dtype=bool)
    for ax in range(3):
        for sgn in (1.0, -1.0):
            s = np.array(o, dtype=np.float64, copy=True)
            s[:, ax] += sgn * step
            out |= (key(s) != base).any(axis=1)
    return out


# ----------------------------------------------------------------- programs
SPH = scenes._sph([0.2, 0.1, -1.0], 0.5, scenes._mat([0.9, 0.5, 0.1]))
SPH2 = scenes._sph([0.5, 0.1, -1.0], 0.5, scenes._mat([0.1, 0.5, 0.9]))


def _root(rt, obj):
    sc = scene_of(rt, [obj])
    return sc, int(sc.desc.objects[0])


def _codes(ops):
    return [(o[0], o[2]) for o in ops]   # (opcode, top)


def test_a_leaf_is_one_op(rt):
    rt.amd_lib()
    for obj in (SPH, scenes._half([0, -1, 0], [0, 1, 0], scenes._mat([0.5, 0.5, 0.5])), scenes._poke([0, 0, -1], 0.5)):
        sc, node = _root(rt, obj)
        ops, depths = rt.node_program(sc, node, ISECT)
        assert ops == [("leaf_isect", node, 1, 0)] and depths == (0, 0)
        ops, depths = rt.node_program(sc, node, IVL)
        assert ops == [("leaf_ivl", node, 0, 0)] and depths == (0, 1)
        assert kernel(rt, sc, node, ISECT) == "rtd::k_node_isect<false>"
        assert kernel(rt, sc, node, IVL) == "rtd::k_node_ivl<false>"


def test_a_transform_over_a_leaf(rt):
    rt.amd_lib()
    sc, node = _root(rt, scenes._tr([0.1, 0, 0], SPH))
    leaf = int(sc.desc.nodes[node].a)
    ops, depths = rt.node_program(sc, node, ISECT)
    assert ops == [("xpush", node, 1, 0), ("leaf_isect", leaf, 0, 0), ("xpop_hit", node, 1, 0)] and depths == (1, 0)
    ops, depths = rt.node_program(sc, node, IVL)
    assert ops == [("xpush", node, 0, 0), ("leaf_ivl", leaf, 0, 0), ("xpop_ivl", node, 0, 0)] and depths == (1, 1)
    # a frame needs no stack for this object (a chain), the node's program one ray
    f = rt.compile_forms(sc)
    assert (f["obj/chain"], f["max_ray_depth"]) == (1, 0)
    assert kernel(rt, sc, node, IVL) == "rtd::k_node_ivl<true>"
    assert kernel(rt, sc, leaf, IVL) == "rtd::k_node_ivl<false>"


@pytest.mark.parametrize("op", ["union", "intersection", "difference"])
def test_a_csg_of_two_leaves(rt, op):
    rt.amd_lib()
    sc, node = _root(rt, {"csg": {"operator": op, "left": SPH, "right": SPH2}})
    a, b = int(sc.desc.nodes[node].a), int(sc.desc.nodes[node].b)
    code = rt.CSG_OPS.index(op)
    assert int(sc.desc.nodes[node].op) == code
    ivl = [("leaf_ivl", a, 0, 0), ("leaf_ivl", b, 0, 0), ("csg", node, 0, code)]
    assert rt.node_program(sc, node, IVL) == (ivl, (0, 2))
    assert rt.node_program(sc, node, ISECT) == (ivl + [("csg_isect", node, 1, 0)], (0, 2))
    assert kernel(rt, sc, node, ISECT) == "rtd::k_node_isect<true>"


def test_a_transform_inside_a_csg_operand(rt):
    rt.amd_lib()
    sc, node = _root(rt, {"csg": {"operator": "difference", "left": SPH,
                                  "right": scenes._rot(30, 1, scenes._sc([0.5, 2, 1], SPH2))}})
    ops, depths = rt.node_program(sc, node, IVL)
    assert [o[0] for o in ops] == ["leaf_ivl", "xpush", "xpush", "leaf_ivl", "xpop_ivl", "xpop_ivl", "csg"]
    assert depths == (2, 2)
    rot = int(sc.desc.nodes[node].b)
    assert (ops[1][1], ops[5][1]) == (rot, rot) and ops[2][1] == ops[4][1] == int(sc.desc.nodes[rot].a)
    ops, depths = rt.node_program(sc, node, ISECT)
    assert _codes(ops)[-1] == ("csg_isect", 1) and all(t == 0 for _, t in _codes(ops)[:-1]) and depths == (2, 2)
    # the operand alone: its own, smaller program
    assert rt.node_program(sc, rot, IVL)[1] == (2, 1)


def test_a_degenerate_scaling_is_op_never(rt):
    """top 1 in hit mode (the bin no frame can reach: tests/test_graph_scenes.py)
    and top 2 in interval mode."""
    rt.amd_lib()
    for f in ([1, 0, 1], [1e-7, 1, 1]):
        sc, node = _root(rt, scenes._sc(f, SPH))
        assert rt.node_program(sc, node, ISECT) == ([("never", node, 1, 0)], (0, 0))
        assert rt.node_program(sc, node, IVL) == ([("never", node, 2, 0)], (0, 1))
        assert kernel(rt, sc, node, ISECT) == "rtd::k_node_isect<true>"
    # under a transform: top 0, between the transform's ops
    sc, node = _root(rt, scenes._tr([1, 0, 0], scenes._sc([1, 0, 1], SPH)))
    assert _codes(rt.node_program(sc, node, ISECT)[0]) == [("xpush", 1), ("never", 0), ("xpop_hit", 1)]
    assert _codes(rt.node_program(sc, node, IVL)[0]) == [("xpush", 0), ("never", 2), ("xpop_ivl", 0)]


def test_program_hook_arguments(rt):
    lib = rt.amd_lib()
    sc, node = _root(rt, scenes._tr([0.1, 0, 0], SPH))
    buf = (C.c_int32 * 8)()
    assert lib.rt_test_node_program(sc.handle, node, IVL, buf, 2, None) == 3   # (the count, two ops written)
    assert list(buf[:4]) == [rt.OP_CODES.index("xpush"), node, 0, 0] and list(buf[4:8])[0] == rt.OP_CODES.index("leaf_ivl")
    assert lib.rt_test_node_program(None, node, IVL, None, 0, None) == RT_ERR_INVALID_ARG
    assert lib.rt_test_node_program(sc.handle, node, IVL, None, 1, None) == RT_ERR_INVALID_ARG
    assert lib.rt_test_node_program(sc.handle, -1, IVL, None, 0, None) == RT_ERR_INVALID_ARG
    assert lib.rt_test_node_program(sc.handle, sc.desc.n_nodes, IVL, None, 0, None) == RT_ERR_INVALID_ARG
    assert lib.rt_test_node_program(sc.handle, node, 2, None, 0, None) == RT_ERR_INVALID_ARG


# ------------------------------------------------------------ kernel choice
def test_every_row_has_exactly_one_recipe(rt):
    recipes = scenes.node_recipes()
    assert len(rt.NODE_TABLES) == 2
    assert rt.node_rows(0) == ["rtd::k_node_isect<true>", "rtd::k_node_ivl<true>", "rtd::k_node_isect<false>",
                               "rtd::k_node_ivl<false>"]
    assert rt.node_rows(1) == ["rtdb::k_node_isect<true>", "rtdb::k_node_ivl<true>"]
    assert sorted(r.row for r in recipes) == sorted(rt.node_rows(0) + rt.node_rows(1))


@pytest.mark.parametrize("recipe", scenes.node_recipes(), ids=lambda r: r.row)
def test_each_recipes_node_picks_its_row(rt, recipe):
    sc = load(rt, recipe.scene_name)
    node = int(sc.desc.objects[recipe.obj])
    assert kernel(rt, sc, node, recipe.kind) == recipe.row
    # the flags a node query accepts change nothing
    for f in (rt.RT_FLAG_NO_CULL, rt.RT_FLAG_NO_BVH, rt.RT_FLAG_FORCE_BVH):
        assert kernel(rt, sc, node, recipe.kind, f) == recipe.row


def test_the_node_tables_are_not_the_query_tables(rt):
    for t in range(len(rt.KERNEL_TABLES)):
        assert not any("k_node_" in r for r in rt.kernel_rows(t))


def test_deep_nodes_take_the_big_stacks_and_their_leaves_the_leaf_rows(rt):
    """The depths that decide are the node's own program's: a bare chain of 12
    transforms is a stackless chain in a frame, its programs push 12 rays."""
    rt.amd_lib()
    sc = load(rt, "deep/xform_nest12")
    chain = [int(n) for n in sc.desc.objects[:sc.desc.n_objects] if kind_of(sc, int(n)) in (3, 4, 5)]
    assert len(chain) == 1
    node, depth = chain[0], 0
    assert rt.node_program(sc, node, ISECT)[1] == (12, 0) and rt.node_program(sc, node, IVL)[1] == (12, 1)
    while not is_leaf(sc, node):
        want = "rtdb" if 12 - depth > 8 else "rtd"   # kMaxRayStack = 8
        assert kernel(rt, sc, node, ISECT) == f"{want}::k_node_isect<true>", depth
        assert kernel(rt, sc, node, IVL) == f"{want}::k_node_ivl<true>", depth
        node, depth = int(sc.desc.nodes[node].a), depth + 1
    assert depth == 12 and kernel(rt, sc, node, ISECT) == "rtd::k_node_isect<false>"
    assert kernel(rt, sc, node, IVL) == "rtd::k_node_ivl<false>"

    sc = load(rt, "deep/csg_right12")
    root = [int(n) for n in sc.desc.objects[:sc.desc.n_objects] if kind_of(sc, int(n)) == 6]
    assert len(root) == 1
    node, left = root[0], 12
    assert rt.node_program(sc, node, IVL)[1] == (0, 12)
    while not is_leaf(sc, node):
        want = "rtdb" if left > 8 else "rtd"   # kMaxIvlSpill + 2 = 8
        assert rt.node_program(sc, node, IVL)[1] == (0, left)
        assert kernel(rt, sc, node, IVL) == f"{want}::k_node_ivl<true>", left
        assert kernel(rt, sc, node, ISECT) == f"{want}::k_node_isect<true>", left
        assert kernel(rt, sc, int(sc.desc.nodes[node].a), IVL) == "rtd::k_node_ivl<false>"
        node, left = int(sc.desc.nodes[node].b), left - 1
    assert left == 1


def _frame_kernel(rt, sc):
    buf = C.create_string_buffer(160)
    return rt.amd_lib().rt_test_kernel_name(sc.handle, 0, 0, buf, 160)


def test_a_node_beyond_the_big_stacks_is_refused_with_the_frames_message(rt):
    leaves = [{"sphere": {"position": [0.01 * i, 0, -2], "radius": 0.5, "color": {"diffuse": [1, 1, 1]}}}
              for i in range(80)]
    node = leaves[-1]
    for leaf in reversed(leaves[:-1]):
        node = {"csg": {"operator": "union", "left": leaf, "right": node}}
    sc = scene_of(rt, [node])
    root = int(sc.desc.objects[0])
    assert _frame_kernel(rt, sc) == RT_ERR_UNSUPPORTED
    frame_msg = rt.last_error()
    for kind in (ISECT, IVL):
        rc, _ = rt.node_kernel_name(sc, root, kind)
        assert rc == RT_ERR_UNSUPPORTED and "CSG operand depth 80" in rt.last_error()
        assert rt.last_error() == frame_msg
    # a subtree of it within the stacks is served, whatever its scene is
    n, left = root, 80
    while left > 64:
        n, left = int(sc.desc.nodes[n].b), left - 1
    assert kernel(rt, sc, n, IVL) == "rtdb::k_node_ivl<true>"
    # a bare chain of 70 transforms renders (a stackless chain); its own programs need 70 rays
    obj = SPH
    for k in range(70):
        obj = scenes._tr([0.001 * k, 0, 0], obj)
    sc = scene_of(rt, [obj])
    assert _frame_kernel(rt, sc) == 0
    rc, _ = rt.node_kernel_name(sc, int(sc.desc.objects[0]), IVL)
    assert rc == RT_ERR_UNSUPPORTED and "transform nesting inside CSG operands 70" in rt.last_error()


def test_kernel_name_hook_arguments(rt):
    lib = rt.amd_lib()
    sc = load(rt, "torture/csg_ops")
    n = sc.desc.n_nodes
    for node in (-1, n):
        rc, _ = rt.node_kernel_name(sc, node, ISECT)
        assert rc == RT_ERR_INVALID_ARG
    rc, _ = rt.node_kernel_name(sc, 0, 2)
    assert rc == RT_ERR_INVALID_ARG
    rc, _ = rt.node_kernel_name(sc, 0, ISECT, rt.RT_FLAG_FP32)
    assert rc == RT_ERR_UNSUPPORTED and "FP32" in rt.last_error()
    rc, _ = rt.node_kernel_name(sc, 0, IVL, rt.RT_FLAG_COUNT_OPS)
    assert rc == RT_ERR_UNSUPPORTED and "COUNT_OPS" in rt.last_error()
    buf = C.create_string_buffer(160)
    assert lib.rt_test_node_kernel_row(2, 0, buf, 160) == RT_ERR_INVALID_ARG
    assert lib.rt_test_node_kernel_row(0, 4, buf, 160) == RT_ERR_INVALID_ARG
    assert lib.rt_test_node_kernel_row(1, 2, buf, 160) == RT_ERR_INVALID_ARG
    assert lib.rt_test_node_kernel_row(0, 0, None, 160) == RT_ERR_INVALID_ARG


# ------------------------------------- argument checks come before the device
def test_argument_errors_are_refused_without_a_device(rt):
    lib = rt.amd_lib()
    sc = load(rt, "torture/csg_ops")
    n_nodes, n = sc.desc.n_nodes, 4
    rays = rt.make_rays(np.zeros((n, 3)), np.tile([0.0, 0.0, -1.0], (n, 1)))
    a, b = np.zeros(n, dtype=rt.HIT_DTYPE), np.zeros(n, dtype=rt.HIT_DTYPE)
    m = np.zeros(n, dtype=np.uint8)
    rp, ap, bp, mp = (x.ctypes.data_as(C.c_void_p) for x in (rays, a, b, m))
    h = sc.handle

    def calls(node=3, s=h, r=rp, cnt=n, flags=0, enter=ap, ex=bp, mask=mp):
        return (lib.rt_query_node_intersect(s, node, r, cnt, flags, enter, mask, None),
                lib.rt_query_node_interval(s, node, r, cnt, flags, enter, ex, mask, None),
                lib.rt_query_node_intersect_device(s, node, r, cnt, flags, enter, mask, None, None),
                lib.rt_query_node_interval_device(s, node, r, cnt, flags, enter, ex, mask, None, None))

    for node in (-1, n_nodes, 1 << 30):
        assert calls(node=node) == (RT_ERR_INVALID_ARG,) * 4 and "node" in rt.last_error()
        assert calls(node=node, cnt=0) == (RT_ERR_INVALID_ARG,) * 4   # (also at n == 0)
    assert calls(s=None) == (RT_ERR_INVALID_ARG,) * 4 and "NULL" in rt.last_error()
    assert calls(r=None) == (RT_ERR_INVALID_ARG,) * 4 and "NULL" in rt.last_error()
    assert calls(enter=None, ex=None, mask=None) == (RT_ERR_INVALID_ARG,) * 4 and "NULL" in rt.last_error()
    # intersect needs its hits; interval any one of its three outputs
    assert lib.rt_query_node_intersect(h, 3, rp, n, 0, None, mp, None) == RT_ERR_INVALID_ARG
    for flag, word in ((rt.RT_FLAG_FP32, "FP32"), (rt.RT_FLAG_COUNT_OPS, "COUNT_OPS")):
        assert calls(flags=flag) == (RT_ERR_UNSUPPORTED,) * 4 and word in rt.last_error()
        assert calls(flags=flag, cnt=0) == (RT_ERR_UNSUPPORTED,) * 4
    assert calls(flags=1 << 20) == (RT_ERR_INVALID_ARG,) * 4
    # n == 0: RT_OK without a launch, whatever the pointers; the stats are zeroed
    st = rt.Stats()
    st.rays_traced = 123
    assert lib.rt_query_node_intersect(h, 3, None, 0, 0, None, None, C.byref(st)) == 0
    assert (st.rays_intersect, st.rays_traced, st.ms_kernel, st.n_gpus) == (0, 0, 0.0, 1)
    assert calls(r=None, cnt=0, enter=None, ex=None, mask=None) == (0,) * 4
    for f in (rt.RT_FLAG_NO_CULL, rt.RT_FLAG_NO_BVH, rt.RT_FLAG_FORCE_BVH):
        assert calls(cnt=0, flags=f) == (0,) * 4
    assert len(rt.query_node_intersect(sc, 3, np.zeros((0, 3)), np.zeros((0, 3)))) == 0
    enter, ex, ok = rt.query_node_interval(sc, 3, np.zeros((0, 3)), np.zeros((0, 3)))
    assert len(enter) == len(ex) == len(ok) == 0


# ------------------------------------------------ the reference's reference
def _probe(rt, sc, node, c, what):
    """The oracle on one fixture case: its answers are the fixture's, and the
    count of rays it alone is unstable on (intersect at the first range,
    interval)."""
    o, d = c["o"], c["d"]
    for tag in ("isect", "isect_win"):
        if tag not in c:
            continue
        (tmin, tmax), ok_g, rec_g = c[tag]
        hit, rec = rt.oracle_node_intersect(sc, node, o, d, tmin, tmax)
        assert np.array_equal(hit, ok_g) and same_records(rec, rec_g, hit), (what, tag)
    ok_g, enter_g, ex_g = c["ivl"]
    enter, ex, ok = rt.oracle_node_interval(sc, node, o, d)
    assert np.array_equal(ok, ok_g) and same_records(enter, enter_g, ok) and same_records(ex, ex_g, ok), (what, "ivl")
    (tmin, tmax) = c["isect"][0]
    ui = unstable(lambda p: isect_key(rt, sc, node, p, d, tmin, tmax), o)
    uv = unstable(lambda p: ivl_key(rt, sc, node, p, d), o)
    assert ui.sum() <= len(o) // 100 and uv.sum() <= len(o) // 100, (what, np.flatnonzero(ui), np.flatnonzero(uv))
    return int(ui.sum()), int(uv.sum()), int(c["isect"][1].sum()), int(ok_g.sum())


@pytest.mark.parametrize("sname", KATS_SCENES)
def test_oracle_is_the_fixture_and_stable_on_kats(rt, sname):
    z = kats()
    sc = rt.load_scene_from_json_text(bytes(z[f"{sname}/scene"]).decode())
    tot = np.zeros(4, dtype=int)
    for node in range(sc.desc.n_nodes):
        tot += _probe(rt, sc, node, kats_case(rt, z, sname, node), (sname, node))
    print(f"  {sname}: {sc.desc.n_nodes} nodes x 128 rays, {tot[2]} hits, {tot[3]} intervals, oracle-unstable: "
          f"intersect {tot[0]}, interval {tot[1]}")
    assert tot[2] > 0 and tot[3] > 0


@pytest.mark.parametrize("name", GRAPH_CASES)
def test_oracle_is_the_fixture_and_stable_on_graph(rt, name):
    z = graph()
    sc = scenes.graph_load(rt, name, scenes.graph_cases(dpi=int(z["dpi"]))[name])
    tot = np.zeros(4, dtype=int)
    for k in range(sc.desc.n_objects):
        tot += _probe(rt, sc, int(sc.desc.objects[k]), graph_case(rt, z, name, k), (name, k))
    print(f"  {name}: {sc.desc.n_objects} objects x 64 rays, {tot[2]} hits, {tot[3]} intervals, oracle-unstable: "
          f"intersect {tot[0]}, interval {tot[1]}")
    assert tot[2] > 0 and tot[3] > 0


def test_the_fixtures_hold_the_odd_intervals():
    """What the GPU tests count on: intervals with an infinite end, origin-inside
    entries (n == 0) and flipped difference faces are in kats.npz."""
    z = kats()
    inf_end = inside = n_ivl = 0
    cases = 0
    for sname in KATS_SCENES:
        node = 0
        while f"{sname}/{node}/o" in z.files:
            ok = z[f"{sname}/{node}/ivl/ok"].astype(bool)
            t, h0 = z[f"{sname}/{node}/ivl/t"], z[f"{sname}/{node}/ivl/h0"]
            inf_end += int(np.isinf(t[ok]).sum())
            n_ivl += int(ok.sum())
            inside += int((ok & (h0[:, 4:7] == 0).all(axis=1)).sum())
            node += 1
            cases += 1
    print(f"  kats.npz: {cases} cases, {n_ivl} intervals, {inf_end} infinite ends, {inside} origin-inside entries")
    assert (cases, n_ivl, inf_end) == (157, 6298, 1712) and inside > 0
