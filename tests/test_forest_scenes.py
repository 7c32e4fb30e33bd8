"""The forest scenes on the CPU (no device is touched): scenes.forest_cases -
more than 256 top-level objects of every compiled form that a scene without
eager programs can hold, at the edges of the wave list and the ray tree - held
here before tests/test_gpu_forest.py relies on them.

Coverage: over the cases, transform chains of one and two levels over a leaf
and over a CSG core, folds and interval groups of each operator, pokeballs,
cull groups and prefilter balls all stand in a wave list; floors70 has two
unbounded chunks, rounds8300 131 chunks (three 64-chunk rounds of every device
chunk test), bare257 none but balls and its 256-object twin no list, eager301
no list and the general kernels; each case selects the kernel rows ROWS names.

Structure: test_bvh.check_wave_bvh on every list with strict containment
(reach <= r, no slack), test_ray_bvh_plan.check_tree and check_culls (every
(ray, object) pair the walk skips is an oracle miss) on every tree.

Pinned to the reference: tests/golden/forest.npz (make_golden.py forest) holds
the reference's frames and ray counts of every case in both modes and its own
Scene::intersect / Scene::occluded of the case's 768 query rays: flags, t and
material in full, and the SHA-256 of the full records (t, p, n, material,
face), which a file under 1 MB cannot hold for 18 cases; the oracle reproduces
all of it bit for bit.

Stability: with test_gpu_query.Case's ray recipe at the fixture's size the
oracle-unstable rays stay within the GPU files' caps: 1 % for intersect and
occluded, 15 of 768 for radiance.  Measured
(profiles/forest_scenes/cpu_tests.txt): intersect and occluded 0 of 768 on all
18 cases, 441 to 702 oracle hits; radiance 8 (mixed320), 2 (form_ties), 0
(mixed320+sun) and 4 (eager301) of 768.  Every test prints its counts."""
import hashlib
import json
import os

import numpy as np
import pytest

import scenes
from test_bvh import _bvh, check_wave_bvh
from test_gpu_query import Case
from test_gpu_radiance import TOL, Ref
from test_ray_bvh_plan import check_culls, check_tree

KEYS = sorted(scenes.forest_cases())
TREE_KEYS = [k for k in KEYS if k not in scenes.FOREST_TREELESS]
RADIANCE_KEYS = ("mixed320", "form_ties", "mixed320+sun", "eager301")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forest.npz")
DPI = 12   # the fixture's: 48 x 36 frames, rounds8300 32 x 24
QUERY_SEED = 20251101
# (standard frame, paper frame, intersect query, RT_FLAG_RAY_BVH intersect query) of the named cases
MIXED = ("rtd::k_std_secw<false, 2, false>", "rtd::k_paper_primary_lean<false, 2, false, false>",
         "rtd::k_query_isect<false, false, false>", "rtd::k_query_isect_bvh<false, false>")
ROWS = {
    "mixed320": MIXED, "partial330": MIXED, "floors70": MIXED, "bare257": MIXED, "rounds8300": MIXED,
    "eager301": ("rtd::k_std<true, true, true, false, false>", "rtd::k_paper_primary<true, true, false>",
                 "rtd::k_query_isect<true, true, false>", "rtd::k_query_isect<true, true, false>"),
    "mixed320+sun": ("rtd::k_std<false, true, true, false, false>", "rtd::k_paper_primary<false, true, false>",
                     "rtd::k_query_isect<false, true, false>", "rtd::k_query_isect_bvh<true, false>"),
    "form_ties": ("rtd::k_std_lean<false, 2, false>",) + MIXED[1:],
}
_dicts, _scenes, _cases, _refs, _frames = {}, {}, {}, {}, {}


# ------------------------------------------------------------------ helpers
def scene_dict(key):
    if not _dicts:
        _dicts.update(scenes.forest_cases(dpi=DPI))
    return _dicts[key]


def load(rt, key):
    """The case as a loaded scene, once (nothing changes a loaded scene)."""
    if key not in _scenes:
        _scenes[key] = scenes.forest_load(rt, key, scene_dict(key))
    return _scenes[key]


def fresh(rt, key):
    """The case as a scene handle that no frame or query has seen."""
    return scenes.forest_load(rt, key, scene_dict(key))


def gold():
    return np.load(GOLD)   # data only (allow_pickle stays False)


class ForestCase(Case):
    """test_gpu_query.Case of a forest scene: its rays and the oracle's answers, computed once."""

    def __init__(self, rt, key):
        self._build(rt, load(rt, key), QUERY_SEED + KEYS.index(key), key)
        for a in (self.rays, self.seg_rays, self.ref_hit, self.ref_rec, self.ref_occ):
            a.setflags(write=False)


def forest_case(rt, key):
    if key not in _cases:
        _cases[key] = ForestCase(rt, key)
    return _cases[key]


def forest_ref(rt, key):
    """test_gpu_radiance.Ref of the case's rays (the oracle's trace of them), computed once."""
    if key not in _refs:
        c = forest_case(rt, key)
        _refs[key] = Ref(rt, c.scene, c.rays["o"], c.rays["d"])
    return _refs[key]


def oracle_frame(rt, key, mode):
    """(oracle frame, counts) of the case, computed once."""
    if (key, mode) not in _frames:
        sc = load(rt, key)
        fb, st = rt.oracle_render(sc, sc.width, sc.height, mode, threads=16)
        fb.setflags(write=False)
        _frames[key, mode] = (fb, (int(st.rays_intersect), int(st.rays_occluded)))
    return _frames[key, mode]


def records_digest(hit, rec):
    """SHA-256 of a query's hit flags and full hit records (a miss is zeros), as 32 uint8."""
    rec = np.where(hit, rec, np.zeros(1, dtype=rec.dtype))
    h = hashlib.sha256(np.ascontiguousarray(hit, dtype=np.uint8).tobytes() + np.ascontiguousarray(rec).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def wave(rt, key):
    """test_bvh._bvh of the case (a directional light changes nothing in the list)."""
    return _bvh(rt, scene_dict(key))


# ----------------------------------------------------------------- coverage
FORMS = ("obj/sphere", "obj/half", "obj/poke", "obj/chain", "obj/group", "obj/never", "chain_core/leaf", "chain_core/csg",
         "chain_m/0", "chain_m/1", "chain_m/2", "fold/union", "fold/intersection", "fold/difference",
         "ivl_group/union", "ivl_group/intersection", "ivl_group/difference", "prefilter")


def test_every_form_stands_in_a_wave_list(rt):
    rt.amd_lib()
    total = {}
    for key in TREE_KEYS:
        forms = rt.compile_forms(load(rt, key))
        assert forms["obj/eager"] == 0, key
        for k, v in forms.items():
            total[k] = max(total.get(k, 0), v) if k.startswith("max_") else total.get(k, 0) + v
    f = rt.compile_forms(load(rt, "mixed320"))
    print("  mixed320: " + ", ".join(f"{k} {v}" for k, v in f.items() if v))
    print("  all lists: " + ", ".join(f"{k} {v}" for k, v in total.items() if v))
    for forms, what in ((f, "mixed320"), (total, "all")):
        missing = [k for k in FORMS if forms[k] == 0 and not (what == "mixed320" and k == "obj/never")]
        assert not missing, (what, missing)
    # every bounded object of mixed320 keeps its bound (the lead holds the floor alone)
    assert f["bounded"] == 320 and f["obj/half"] == 1
    f = rt.compile_forms(load(rt, "eager301"))
    assert f["obj/eager"] == 1 and f["obj/chain"] > 100 and f["obj/group"] > 0


def test_lists_reach_their_edges(rt):
    rt.amd_lib()
    b = {key: wave(rt, key) for key in KEYS}
    for key in KEYS:
        print(f"  {key}: {b[key]['n_objs']} objects, list {b[key]['n']}, {b[key]['chunks']} chunks, "
              f"{int((b[key]['ctype'] == 1).sum())} unbounded")
    assert (b["mixed320"]["n"], b["mixed320"]["chunks"]) == (384, 6)            # six full chunks
    assert b["partial330"]["n"] % 64 != 0 and int((b["partial330"]["wtype"] != 2).sum()) == 64
    assert int(((b["partial330"]["wtype"] == 1) | (b["partial330"]["wtype"] == 3)).sum()) == 3
    assert int((b["floors70"]["ctype"] == 1).sum()) >= 2
    assert b["bare257"]["n"] == 257 and np.all(b["bare257"]["wtype"] == 2)
    assert b["rounds8300"]["chunks"] >= 129
    assert b["eager301"]["n"] == 0 and b["eager301"]["n_objs"] - b["eager301"]["groups"] == 301
    # one object fewer than bare257: no list
    assert _bvh(rt, scenes.forest_scene(14, 256, 0, dpi=DPI))["n"] == 0
    for s in scenes.FOREST_SEEDS:
        assert b[f"seed/{s}"]["n"] > 256
    # the trees: a lead of whole chunks, none on eager301
    for key in KEYS:
        nodes, lead, n_wave = rt.ray_bvh_nodes(load(rt, key))
        assert (len(nodes) > 0) == (key in TREE_KEYS) and n_wave == b[key]["n"], key
    assert rt.ray_bvh_nodes(load(rt, "floors70"))[1] == 128


@pytest.mark.parametrize("key", sorted(ROWS))
def test_named_cases_select_their_rows(rt, key):
    rt.amd_lib()
    sc = load(rt, key)
    got = (rt.kernel_name(sc, 0), rt.kernel_name(sc, 1), rt.query_kernel_name(sc, 0),
           rt.ray_bvh_kernel_name(sc, 0, rt.RT_FLAG_RAY_BVH))
    assert all(rc == 0 for rc, _ in got)
    assert tuple(name for _, name in got) == ROWS[key]
    occl = rt.ray_bvh_kernel_name(sc, 1, rt.RT_FLAG_RAY_BVH)[1]
    assert occl == ROWS[key][3].replace("isect", "occl")


# ---------------------------------------------------------------- structure
@pytest.mark.parametrize("key", TREE_KEYS)
def test_wave_list_structure(rt, key):
    """check_wave_bvh with strict containment: each chunk ball holds its members' f32 balls, in float64."""
    b = wave(rt, key)
    assert b["n"] > 0
    with np.errstate(invalid="ignore", over="ignore"):
        worst = check_wave_bvh(b, slack=0.0)
    print(f"  {key}: list {b['n']}, {b['chunks']} chunks, tightest reach / r = {worst:.9f}")


@pytest.mark.parametrize("key", TREE_KEYS)
def test_tree_structure(rt, key):
    check_tree(rt, load(rt, key), wave(rt, key), key)


@pytest.mark.parametrize("key", TREE_KEYS)
def test_culls_are_conservative_against_the_oracle(rt, key):
    c = forest_case(rt, key)
    check_culls(rt, c.scene, c.rays, c.seg_rays, c.ref_hit, c.ref_rec, key)


# ------------------------------------------------- pinned to the reference
def test_fixture_complete():
    z = gold()
    assert int(z["dpi"]) == DPI and os.path.getsize(GOLD) < 1000000
    for key in KEYS:
        for what in ("0/fb", "0/counts", "1/fb", "1/counts", "q/hit", "q/occ", "q/t", "q/mat", "q/sha"):
            assert f"{key}/{what}" in z.files, (key, what)
        w, h = (32, 24) if key == "rounds8300" else (48, 36)
        assert z[f"{key}/0/fb"].shape == z[f"{key}/1/fb"].shape == (h, w, 3)
    assert {k.rsplit("/", 2)[0] for k in z.files} - {"dpi"} == set(KEYS)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("key", KEYS)
def test_oracle_matches_reference_fixture(rt, key, mode):
    z = gold()
    fb, counts = oracle_frame(rt, key, mode)
    assert counts == tuple(int(v) for v in z[f"{key}/{mode}/counts"])
    assert np.array_equal(fb, z[f"{key}/{mode}/fb"], equal_nan=True)
    off_bg = int((np.abs(fb - fb[0, 0]).max(axis=2) > 0).sum())
    print(f"  {key} mode {mode}: {fb.shape[1]}x{fb.shape[0]}, counts {counts}, {off_bg} pixels differ from the corner's")
    assert np.isfinite(fb).all()


@pytest.mark.parametrize("key", KEYS)
def test_oracle_matches_reference_queries(rt, key):
    """Scene::intersect and Scene::occluded of the case's 768 rays: the reference's answers, bit for bit."""
    z, c = gold(), forest_case(rt, key)
    n = len(c.rays)
    assert np.array_equal(np.packbits(c.ref_hit), z[f"{key}/q/hit"])
    assert np.array_equal(np.packbits(c.ref_occ), z[f"{key}/q/occ"])
    assert np.array_equal(np.where(c.ref_hit, c.ref_rec["t"], 0.0), z[f"{key}/q/t"], equal_nan=True)
    assert np.array_equal(np.where(c.ref_hit, c.ref_rec["mat"], -1), z[f"{key}/q/mat"])
    assert np.array_equal(records_digest(c.ref_hit, c.ref_rec), z[f"{key}/q/sha"])
    print(f"  {key}: {n} rays, {int(c.ref_hit.sum())} hits and {int(c.ref_occ.sum())} occluded, the reference's")


def test_form_tie_order_matters_in_the_reference(rt):
    """form_ties resolves its ties by the reference's object order: reversing
    the pairs of any one kind changes the oracle's image (so does reversing
    all), and the fixture pins the rule."""
    want, _ = oracle_frame(rt, "form_ties", 0)
    kinds = scenes.FOREST_TIE_KINDS
    for rev in [(k,) for k in kinds] + [kinds]:
        sc = rt.load_scene_from_json_text(json.dumps(scenes.forest_tie_scene(DPI, reverse=rev)))
        fb, _ = rt.oracle_render(sc, sc.width, sc.height, 0, threads=16)
        n = int((np.abs(fb - want).max(axis=2) > 0).sum())
        print(f"  form_ties with {'/'.join(rev) if len(rev) == 1 else 'every kind'} reversed: {n} pixels change")
        assert n > 0, rev
    assert len(scene_dict("form_ties")["objects"]) == len(scenes.bvh_scenes(DPI)["ties"]["objects"]) == 301


# ---------------------------------------------------------------- stability
@pytest.mark.parametrize("key", KEYS)
def test_oracle_queries_are_stable(rt, key):
    c = forest_case(rt, key)
    n_i = sum(c.oracle_unstable(r, False) for r in c.rays)
    n_o = sum(c.oracle_unstable(r, True) for r in c.seg_rays)
    print(f"  {key}: {int(c.ref_hit.sum())} hits, {int(c.ref_occ.sum())} occluded, oracle-unstable: intersect {n_i}, "
          f"occluded {n_o} of {len(c.rays)}")
    assert len(c.rays) == 768 and c.ref_hit.sum() >= len(c.rays) // 4 and c.ref_occ.any()
    assert n_i <= len(c.rays) // 100 and n_o <= len(c.rays) // 100


@pytest.mark.parametrize("key", RADIANCE_KEYS)
def test_oracle_radiance_is_stable(rt, key):
    r = forest_ref(rt, key)
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
