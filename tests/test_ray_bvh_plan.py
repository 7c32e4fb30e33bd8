"""The per-ray BVH of RT_FLAG_RAY_BVH on the host: the tree scene_compile.cpp
builds (rt_test_ray_bvh), the kernels' walk restated on the host
(rt_test_ray_bvh_walk, the node test of ray_bvh_rules.hpp) held to the CPU
oracle alone, and the kernel a flagged query launches
(rt_test_ray_bvh_kernel_name).  No device is touched; the kernels themselves
are held to the flat kernels' bytes by tests/test_gpu_ray_bvh.py.

The cull check: an object the walk does not reach on a ray's segment must be
a miss of the oracle's Primitive::intersect of that object on the same,
inclusive, range - with the range's end at the oracle's own closest t, so
that a coincident object tying at exactly t may never be skipped."""
import ctypes as C
import json

import numpy as np
import pytest

import scenes
from test_bvh import _bvh
from test_gpu_query import Case, case
from test_placed_scenes import PL, load, map_rays, placed_any_scale

ISECT, OCCL = 0, 1
RT_ERR_UNSUPPORTED = -6
_dp = C.POINTER(C.c_double)
SEED = 20250301
PLACEMENTS = ("far", "huge_far", "e39")
_scenes, _cases = {}, {}


def scene_dict(name):
    if name == "bvh/perf300":
        return scenes.bvh_perf_scene(300, dpi=16)
    if name == "perf4096":
        return scenes.bvh_perf_scene(4096, dpi=16)
    if name.startswith("bvh/"):
        return scenes.bvh_scenes(16)[name[4:]]
    if name.startswith("leaf/"):
        return scenes.leaf_cases()[name[5:]]
    raise KeyError(name)


LEAF_BVH = tuple("leaf/" + k for k, v in sorted(scenes.LEAF_LAYOUT.items()) if v == "bvh")
TREE_SCENES = ("bvh/grid", "bvh/ties", "bvh/perf300", "perf4096") + LEAF_BVH
WALK_SCENES = ("bvh/ties", "bvh/grid", "perf4096")


def scene(rt, name):
    if name not in _scenes:
        _scenes[name] = rt.load_scene_from_json_text(json.dumps(scene_dict(name)))
    return _scenes[name]


def ray_case(rt, name):
    """test_gpu_query.Case of a walk scene: the 768 incoherent rays and the oracle's answers, once."""
    if name == "bvh/ties":
        return case(rt, name)
    if name not in _cases:
        c = Case.__new__(Case)
        c._build(rt, scene(rt, name), SEED + WALK_SCENES.index(name), name)
        _cases[name] = c
    return _cases[name]


# ---------------------------------------------------------------- structure
def _subtree_ok(nodes, i, end):
    """Pre-order nesting of [i, end): every child subtree ends inside its parent's; returns the leaves."""
    leaves = []
    j = i
    while j < end:
        s = int(nodes["skip"][j])
        assert j < s <= end, (j, s, end)
        if nodes["count"][j] > 0:
            assert s == j + 1, (j, s)   # a leaf has no children
            leaves.append(j)
        else:
            assert s > j + 1, (j, s)    # an inner node has some
            leaves += _subtree_ok(nodes, j + 1, s)
        j = s
    return leaves


@pytest.mark.parametrize("name", TREE_SCENES)
def test_tree_structure(rt, name):
    check_tree(rt, scene(rt, name), _bvh(rt, scene_dict(name)), name)


def check_tree(rt, sc, wave, name):
    """The structure of sc's ray tree over its wave list `wave` (test_bvh._bvh of the same scene)."""
    nodes, lead, n_wave = rt.ray_bvh_nodes(sc)
    n = len(nodes)
    assert n > 0 and 0 <= lead < n_wave
    assert wave["n"] == n_wave
    wctab, ctype = wave["wctab"], wave["wtype"]
    # the lead is the unbounded part of the wave list (and its padding): no ball records there, only balls behind
    assert not (ctype[:lead] == 2).any() and (ctype[lead:] == 2).all()
    # skips: forward, nested, the last one n_nodes; the root spans everything
    assert (nodes["skip"] > np.arange(n)).all() and nodes["skip"][0] == n and nodes["skip"][-1] == n
    leaves = _subtree_ok(nodes, 0, n)
    # every bounded object of the wave list in exactly one leaf, the leaves in list order
    seen = np.zeros(n_wave, dtype=np.int32)
    nxt = lead
    for j in leaves:
        f, c = int(nodes["first"][j]), int(nodes["count"][j])
        assert f == nxt and 0 < c
        seen[f:f + c] += 1
        nxt = f + c
    assert nxt == n_wave and (seen[lead:] == 1).all() and not seen[:lead].any()
    assert int((nodes["count"] == 0).sum()) + len(leaves) == n
    # containment in float64 from the stored floats: |c_node - c_obj| + r_obj <= r_node for every object below
    ball = wctab[:, :4].astype(np.float64)
    cn, rn = nodes["c"][:, :3].astype(np.float64), nodes["c"][:, 3].astype(np.float64)
    # start[j]: the first object of the first leaf at or after node j (pre-order: where node j's objects begin)
    start = np.full(n + 1, n_wave, dtype=np.int64)
    for j in range(n - 1, -1, -1):
        start[j] = nodes["first"][j] if nodes["count"][j] > 0 else start[j + 1]
    worst = 0.0
    for j in range(n):
        a, b = int(start[j]), int(start[int(nodes["skip"][j])])   # the objects below node j
        assert lead <= a < b <= n_wave
        with np.errstate(invalid="ignore", over="ignore"):
            d = ball[a:b, :3] - cn[j]
            reach = np.sqrt((d * d).sum(axis=1)) + ball[a:b, 3]
            assert (reach <= rn[j]).all(), (name, j, float(reach.max()), float(rn[j]))
            if np.isfinite(rn[j]):
                worst = max(worst, float((reach / rn[j]).max()))
    print(f"  {name}: {n} nodes, {len(leaves)} leaves over {n_wave - lead} objects (+{lead} lead), "
          f"tightest reach / r = {worst:.9f}")


def _eager_torture(rt):
    for k, v in sorted(scenes.torture_scenes(dpi=12).items()):
        sc = rt.load_scene_from_json_text(json.dumps(v))
        if rt.compile_forms(sc)["obj/eager"] > 0:
            return k, sc
    raise AssertionError("no torture scene with an eager program")


def test_no_tree_without_a_wave_list(rt):
    """config 4 (few objects), a scene with eager programs and a 200-object scene have no tree."""
    small = rt.load_scene_from_json_text(json.dumps(scenes.bvh_perf_scene(200, dpi=16)))
    _, eager = _eager_torture(rt)
    for sc in (rt.load_scene_from_json_text(scenes.config_json(4, dpi=24)[0]), eager, small):
        nodes, lead, n_wave = rt.ray_bvh_nodes(sc)
        assert len(nodes) == 0 and n_wave == 0 and lead == 0
        with pytest.raises(rt.RTError) as e:
            rt.ray_bvh_walk(sc, [[0, 0, 5]], [[0, 0, -1]])
        assert e.value.code == RT_ERR_UNSUPPORTED


# ------------------------------------------------------- the culls vs oracle
def _unreached_all_miss(rt, sc, rays, reached, what):
    """Every (ray, top-level object) the walk did not reach: a miss of the oracle's node intersect on the ray's range."""
    lib = rt.oracle_lib()
    desc, fn = sc.desc_ptr, lib.oracle_node_intersect
    objs = [int(sc.desc.objects[k]) for k in range(sc.desc.n_objects)]
    h = rt.OracleHit()
    hp = C.byref(h)
    n_skip = 0
    for k in range(len(rays)):
        o = np.ascontiguousarray(rays["o"][k])
        d = np.ascontiguousarray(rays["d"][k])
        op, dp = o.ctypes.data_as(_dp), d.ctypes.data_as(_dp)
        t0, t1 = float(rays["tmin"][k]), float(rays["tmax"][k])
        for j in np.flatnonzero(~reached[k]):
            assert not fn(desc, objs[j], op, dp, t0, t1, hp), (what, k, int(j), h.t, t0, t1)
            n_skip += 1
    return n_skip


def _closest_ranges(c, rays, ref_hit, ref_rec):
    """rays with tmax at the oracle's own closest t (a miss keeps its tmax)."""
    out = rays.copy()
    out["tmax"] = np.where(ref_hit, ref_rec["t"], rays["tmax"])
    return out


@pytest.mark.parametrize("pl", ("unplaced",) + PLACEMENTS)
@pytest.mark.parametrize("name", WALK_SCENES)
def test_culls_are_conservative_against_the_oracle(rt, name, pl):
    base = ray_case(rt, name)
    scale, offset = PL[pl]
    if pl == "unplaced":
        sc, rays, segs, ref_hit, ref_rec = base.scene, base.rays, base.seg_rays, base.ref_hit, base.ref_rec
    else:
        sc = load(rt, placed_any_scale(scene_dict(name), scale, offset))
        rays, segs = map_rays(base.rays, scale, offset), map_rays(base.seg_rays, scale, offset)
        pc = Case.__new__(Case)
        pc.scene, pc.rt, pc.olib, pc.desc = sc, rt, rt.oracle_lib(), sc.desc_ptr
        ref_hit, ref_rec = pc.oracle_intersect(rays)
    check_culls(rt, sc, rays, segs, ref_hit, ref_rec, f"{name} {pl}")


def check_culls(rt, sc, rays, segs, ref_hit, ref_rec, what):
    """The walk of `rays` up to the oracle's own closest t (ref_hit, ref_rec)
    and of the segments `segs`: every object it does not reach is an oracle miss."""
    assert ref_hit.sum() >= len(rays) // 4
    for kind, rr in (("closest", _closest_ranges(None, rays, ref_hit, ref_rec)), ("segment", segs)):
        reached, tests = rt.ray_bvh_walk(sc, rr["o"], rr["d"], rr["tmin"], rr["tmax"])
        n_skip = _unreached_all_miss(rt, sc, rr, reached, f"{what} {kind}")
        print(f"  {what} {kind}: {len(rr)} rays, reached {reached.sum(axis=1).mean():.1f} of {reached.shape[1]} "
              f"objects and {tests.mean():.1f} node tests per ray; {n_skip} skipped pairs are oracle misses")


def test_the_tree_culls_at_all(rt):
    """64 rays from (x, 100, z) along +y over the 4096 spheres reach only the
    unbounded lead (the floor): every sphere lies below y = 2.62 and within 20
    units of the lattice's centre, so the segment's nearest point to any
    enclosing ball is its origin, outside it."""
    sc = scene(rt, "perf4096")
    rng = np.random.default_rng(SEED)
    o = np.stack([rng.uniform(-6, 6, 64), np.full(64, 100.0), rng.uniform(-14, -1.5, 64)], axis=1)
    d = np.tile([0.0, 1.0, 0.0], (64, 1))
    reached, tests = rt.ray_bvh_walk(sc, o, d)
    nodes, lead, _ = rt.ray_bvh_nodes(sc)
    assert lead >= 1
    assert (reached.sum(axis=1) == 1).all() and reached[:, 0].all()   # object 0: the half-space floor
    assert (tests == 1).all()   # the root alone is tested
    # ... and a ray straight down through the lattice does reach spheres
    reached, tests = rt.ray_bvh_walk(sc, o, -d)
    assert (tests > 1).all() and reached[:, 0].all()


@pytest.mark.parametrize("name", WALK_SCENES + ("bvh/perf300",))
def test_recorded_walk_costs(rt, name):
    """Recorded, not asserted: reached objects and node tests per ray on shuffled centre camera rays."""
    sc = scene(rt, name)
    rng = np.random.default_rng(SEED + 1)
    W, H = sc.width, sc.height
    n = 512
    olib = rt.oracle_lib()
    o3, d3 = (C.c_double * 3)(), (C.c_double * 3)()
    o, d = np.empty((n, 3)), np.empty((n, 3))
    for k, (i, j) in enumerate(zip(rng.integers(0, W, n), rng.integers(0, H, n))):
        olib.oracle_camera_ray(sc.desc_ptr, int(i), int(j), 0.0, 0.0, 0, o3, d3)
        o[k], d[k] = list(o3), list(d3)
    reached, tests = rt.ray_bvh_walk(sc, o, d)
    nodes, lead, n_wave = rt.ray_bvh_nodes(sc)
    print(f"  {name}: {sc.desc.n_objects} objects, {len(nodes)} nodes; per ray on [1e-4, inf): "
          f"{reached.sum(axis=1).mean():.1f} objects reached, {tests.mean():.1f} node tests "
          f"(max {int(reached.sum(axis=1).max())} / {int(tests.max())})")
    assert reached.shape == (n, sc.desc.n_objects)


# -------------------------------------------------------------- kernel choice
def _name(rt, sc, kind, flags):
    rc, name = rt.ray_bvh_kernel_name(sc, kind, flags)
    assert rc == 0, rt.last_error()
    return name


def _flat(rt, sc, kind, flags=0):
    rc, name = rt.query_kernel_name(sc, kind, flags)
    assert rc == 0, rt.last_error()
    return name


def test_rows():
    import rtamd
    assert rtamd.ray_bvh_rows() == [
        "rtd::k_query_isect_bvh<true, false>", "rtd::k_query_occl_bvh<true, false>",
        "rtd::k_query_isect_bvh<false, false>", "rtd::k_query_occl_bvh<false, false>",
        "rtd::k_query_isect_bvh<false, true>", "rtd::k_query_occl_bvh<false, true>"]
    assert not any("bvh" in t for t in rtamd.KERNEL_TABLES)


def test_kernel_choice(rt):
    F = rt.RT_FLAG_RAY_BVH
    assert F == 32
    ties = scene(rt, "bvh/ties")
    sun = rt.with_dir_lights(ties, [([-0.4, -1.0, -0.3], [0.9, 0.85, 0.8])])
    perf = scene(rt, "bvh/perf300")
    for kind, k in ((ISECT, "isect"), (OCCL, "occl")):
        assert _name(rt, ties, kind, F) == f"rtd::k_query_{k}_bvh<false, false>"
        assert _name(rt, sun, kind, F) == f"rtd::k_query_{k}_bvh<true, false>"
        assert _name(rt, perf, kind, F) == f"rtd::k_query_{k}_bvh<false, true>"
        # the flag is accepted and changes nothing: RT_FLAG_NO_CULL, a small scene, a big-stack scene
        assert _name(rt, ties, kind, F | rt.RT_FLAG_NO_CULL) == _flat(rt, ties, kind, rt.RT_FLAG_NO_CULL)
        cfg3 = rt.load_scene_from_json_text(scenes.config_json(3, dpi=24)[0])
        assert _name(rt, cfg3, kind, F) == _flat(rt, cfg3, kind) == f"rtd::k_query_{k}<false, false, true>"
        deep = rt.load_scene_from_json_text(json.dumps(scenes.deep_scenes()["csg_right12"]))
        assert _name(rt, deep, kind, F) == _flat(rt, deep, kind) and _flat(rt, deep, kind).startswith("rtdb::")
        # the unflagged name is unchanged everywhere, through either hook, and ignores the bit
        for sc, want in ((ties, f"rtd::k_query_{k}<false, false, false>"), (sun, f"rtd::k_query_{k}<false, true, false>"),
                         (perf, f"rtd::k_query_{k}<false, false, true>")):
            assert _flat(rt, sc, kind) == _name(rt, sc, kind, 0) == want
            assert _flat(rt, sc, kind, F) == want
        for bad, word in ((rt.RT_FLAG_FP32, "FP32"), (rt.RT_FLAG_COUNT_OPS, "COUNT_OPS")):
            rc, _ = rt.ray_bvh_kernel_name(ties, kind, F | bad)
            assert rc == RT_ERR_UNSUPPORTED and word in rt.last_error()


def test_big_stack_scene_with_a_wave_list_keeps_the_flat_row(rt):
    """A scene of more than 256 objects whose CSG depth needs the big stacks: a wave list and a tree, but rtdb."""
    leaves = [{"sphere": {"position": [0.05 * i, 0, -3], "radius": 0.3, "color": {"diffuse": [1, 1, 1]}}}
              for i in range(12)]
    node = leaves[-1]
    for leaf in reversed(leaves[:-1]):
        node = {"csg": {"operator": "union", "left": leaf, "right": node}}
    s = scenes.bvh_perf_scene(300, dpi=16)
    s["objects"].append(node)
    sc = rt.load_scene_from_json_text(json.dumps(s))
    flat = _flat(rt, sc, ISECT)
    assert flat == "rtdb::k_query_isect<true, true, false>"
    assert len(rt.ray_bvh_nodes(sc)[0]) > 0
    assert _name(rt, sc, ISECT, rt.RT_FLAG_RAY_BVH) == flat
