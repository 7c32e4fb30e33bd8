"""Batched radiance queries on the GPU (rt_query_radiance / rt_query_radiance_device:
Tracer::trace for caller-given rays, tracer.cpp:12-73) against the CPU oracle's
trace of the same rays (rtamd.oracle_trace, which tests/test_radiance_plan.py
holds to the oracle's own frames).

Rays: those of tests/test_gpu_query.py (per scene 384 pixel-centre camera rays
and 384 surface-to-surface rays, shuffled), or the same recipe on other scenes.
Both sides trace Ray(o, (o + d) - o): the oracle's zero-size screen sits at
o + d.

Bar: every channel |gpu - oracle| <= 1e-5, the project's parity bar, and the
Scene::intersect / Scene::occluded call counts of a batch exactly the sums of
the oracle's per-ray counts.  A ray may be left out only if the ORACLE alone is
unstable on it (its colour moves by more than 1e-5, or its ray counts change,
when the origin moves +-1e-7 along an axis): at most 15 of 768 rays of a scene.
The oracle's own unstable sets by that rule (CPU): deep/mirrors_rec24 9,
deep/csg_right12 7, config 5 2, one each on bvh/ties, config 3,
dir/pokeball_csg_sun, torture/csg_ops, torture/pokeball_csg,
torture/reflect_refract, torture/xform_in_csg, none on the other 8.
Measured on an MI355X: the largest difference over all of this file's rays is
5.0e-11, and no ray had to be left out."""
import ctypes as C
import json

import numpy as np
import pytest

import scenes
from test_gpu_query import SCENES, case

pytestmark = pytest.mark.gpu

TOL = 1e-5
_dp = C.POINTER(C.c_double)
_refs = {}


def _cap(n):
    return n * 15 // 768


# ---------------------------------------------------------------- reference
class Ref:
    """Rays (o, d as traced) of one scene and the oracle's trace of them, computed once."""

    def __init__(self, rt, sc, o, d):
        self.sc = sc
        self.o = np.ascontiguousarray(o, dtype=np.float64)
        self.d = rt.oracle_trace_dirs(self.o, d)
        self.rgb, self.ni, self.no = rt.oracle_trace(sc, self.o, self.d)
        self.rgb.setflags(write=False)
        self.ni.setflags(write=False)
        self.no.setflags(write=False)
        dsc = sc.desc
        self.background = np.array(list(dsc.background))

    def __len__(self):
        return len(self.o)


def ref_of(rt, name):
    """The rays of test_gpu_query's scene `name` and the oracle's trace of them."""
    if name not in _refs:
        c = case(rt, name)
        _refs[name] = Ref(rt, c.scene, c.rays["o"], c.rays["d"])
    return _refs[name]


def recipe_rays(rt, sc, n_cam, n_surf, seed):
    """test_gpu_query's ray recipe on any scene: pixel-centre camera rays at
    random pixels and surface-to-surface rays between their hits, shuffled."""
    olib, desc = rt.oracle_lib(), sc.desc_ptr
    rng = np.random.default_rng(seed)
    W, H = sc.width, sc.height
    cam_o, cam_d = np.empty((n_cam, 3)), np.empty((n_cam, 3))
    o3, d3 = (C.c_double * 3)(), (C.c_double * 3)()
    pp, pn = [], []
    h = rt.OracleHit()
    for k in range(n_cam):
        olib.oracle_camera_ray(desc, int(rng.integers(0, W)), int(rng.integers(0, H)), 0.0, 0.0, 0, o3, d3)
        cam_o[k], cam_d[k] = list(o3), list(d3)
        if olib.oracle_scene_intersect(desc, o3, d3, 1e-4, float("inf"), C.byref(h)):
            pp.append(list(h.p))
            pn.append(list(h.n))
    pp, pn = np.array(pp), np.array(pn)
    assert len(pp) >= 2
    a, b = rng.integers(0, len(pp), n_surf), rng.integers(0, len(pp), n_surf)
    so = pp[a] + 1e-3 * pn[a]
    sd = pp[b] + rng.normal(0.0, 0.05, (n_surf, 3)) - so
    order = rng.permutation(n_cam + n_surf)
    return np.concatenate([cam_o, so])[order], np.concatenate([cam_d, sd])[order]


def recipe_ref(rt, key, sc, n_cam, n_surf, seed):
    if key not in _refs:
        _refs[key] = Ref(rt, sc, *recipe_rays(rt, sc, n_cam, n_surf, seed))
    return _refs[key]


def oracle_unstable(rt, r, k, step=1e-7):
    """The oracle's own trace of ray k moves under a +-step shift of the origin."""
    for ax in range(3):
        for sgn in (1.0, -1.0):
            o = r.o[k:k + 1].copy()
            o[0, ax] += sgn * step
            rgb, ni, no = rt.oracle_trace(r.sc, o, r.d[k:k + 1])
            if float(np.abs(rgb[0] - r.rgb[k]).max()) > TOL or (ni[0], no[0]) != (r.ni[k], r.no[k]):
                return True
    return False


def check(rt, r, got, what, flags=0, step=1e-7):
    """got (n, 3) against the oracle at this file's bar, then the rays not left
    out once more as their own batch: the same colours and the oracle's counts.
    step: the instability probe's shift of the origin."""
    n = len(r)
    assert got.shape == (n, 3) and got.dtype == np.float64
    with np.errstate(invalid="ignore"):
        diff = np.abs(got - r.rgb).max(axis=1)
        bad = np.flatnonzero(~(diff <= TOL))
    left_out = [int(k) for k in bad if oracle_unstable(rt, r, k, step)]
    wrong = sorted(set(bad.tolist()) - set(left_out))
    keep = np.ones(n, dtype=bool)
    keep[left_out] = False
    mx = float(diff[keep].max(initial=0.0))
    print(f"  {what}: {n} rays, max|d|={mx:.3g}, left out {len(left_out)} (oracle unstable), "
          f"oracle counts ({int(r.ni[keep].sum())}, {int(r.no[keep].sum())})")
    assert not wrong, (what, wrong[:8], [(got[k], r.rgb[k]) for k in wrong[:3]])
    assert len(left_out) <= _cap(n), (what, left_out)
    st = rt.Stats()
    again = rt.query_radiance(r.sc, r.o[keep], r.d[keep], flags, st)
    assert again.tobytes() == got[keep].tobytes(), what
    assert (st.rays_intersect, st.rays_occluded) == (int(r.ni[keep].sum()), int(r.no[keep].sum())), what
    assert st.rays_traced == st.rays_intersect + st.rays_occluded and st.pixels == 0
    return keep


# ------------------------------------------------- 1. incoherent rays, every scene
@pytest.mark.parametrize("name", sorted(SCENES))
def test_radiance_matches_oracle(gpu, name):
    r = ref_of(gpu, name)
    assert len(r) == 768
    st = gpu.Stats()
    got = gpu.query_radiance(r.sc, r.o, r.d, stats=st)
    assert st.ms_kernel > 0.0 and st.ms_total >= st.ms_kernel and st.n_gpus == 1 and st.pixels == 0
    check(gpu, r, got, name)
    hits = (np.abs(r.rgb - r.background).max(axis=1) > 0).sum()
    assert hits >= len(r) // 4   # (the batch does exercise the objects)


# --------------------------------------------------- 2. the frame from its own rays
def _frame_scene(rt, name):
    if name.startswith("config"):
        return rt.load_scene_from_json_text(scenes.config_json(int(name[6:]), dpi=24)[0])
    text, lights = SCENES[name]
    sc = rt.load_scene_from_json_text(text)
    return rt.with_dir_lights(sc, lights) if lights else sc


@pytest.mark.parametrize("name", ["config3", "config4", "config5", "deep/mirrors_rec24", "dir/pokeball_csg_sun"])
def test_frame_from_its_own_rays(gpu, name):
    """The frame's 8 W H jittered rays queried in frame order, averaged per
    pixel in sample order: the oracle's frame and rt_render's, with the
    oracle frame's ray counts."""
    sc = _frame_scene(gpu, name)
    W, H = sc.width, sc.height
    o, d = gpu.oracle_frame_rays(sc)
    st = gpu.Stats()
    rgb = gpu.query_radiance(sc, o.reshape(-1, 3), d.reshape(-1, 3), stats=st).reshape(H, W, 8, 3)
    acc = np.zeros((H, W, 3))
    for s in range(8):
        acc += rgb[:, :, s]
    acc *= 1.0 / 8.0
    ref, ost = gpu.oracle_render(sc, W, H, 0, threads=8)
    fst = gpu.Stats()
    fb = gpu.Tracer(sc, W, H, 0).render(fst)
    e_or, e_fb = float(np.abs(acc - ref).max()), float(np.abs(acc - fb).max())
    print(f"  {name}: {W}x{H}, {8 * W * H} rays, max|d| oracle {e_or:.3g}, rt_render {e_fb:.3g}, "
          f"bit-identical to rt_render: {acc.tobytes() == fb.tobytes()}, kernel {st.ms_kernel:.3f} ms "
          f"(frame {fst.ms_kernel:.3f} ms)")
    assert e_or <= TOL and e_fb <= TOL
    assert (st.rays_intersect, st.rays_occluded) == (ost.rays_intersect, ost.rays_occluded)
    assert (fst.rays_intersect, fst.rays_occluded) == (ost.rays_intersect, ost.rays_occluded)


# ------------------------------------------------------------- 3. RT_FLAG_NO_CULL
@pytest.mark.parametrize("name", sorted(SCENES))
def test_no_cull_is_byte_identical(gpu, name):
    r = ref_of(gpu, name)
    sa, sb = gpu.Stats(), gpu.Stats()
    a = gpu.query_radiance(r.sc, r.o, r.d, stats=sa)
    b = gpu.query_radiance(r.sc, r.o, r.d, gpu.RT_FLAG_NO_CULL, sb)
    assert a.tobytes() == b.tobytes()
    assert (sa.rays_intersect, sa.rays_occluded) == (sb.rays_intersect, sb.rays_occluded)
    # the BVH flags have no effect
    for f in (gpu.RT_FLAG_NO_BVH, gpu.RT_FLAG_FORCE_BVH):
        assert gpu.query_radiance(r.sc, r.o, r.d, f).tobytes() == a.tobytes()


# ------------------------------------------------------------------ 4. wave tails
def _dev_radiance(rt, sc, o, d, n, cap, stream=None, flags=0):
    """rt_query_radiance_device on the first n rays into a buffer of cap colours filled with 0xAB."""
    rays = rt.make_rays(o, d)
    d_rays = rt.DeviceBuffer(max(1, len(rays)) * 64)
    d_rays.from_host(rays)
    d_rgb = rt.DeviceBuffer(cap * 24)
    d_rgb.from_host(np.full(cap * 24, 0xAB, dtype=np.uint8))
    st = rt.Stats()
    rt.query_radiance_device(sc, d_rays, n, d_rgb, flags, stream, st)
    return d_rgb.to_host(np.uint8), st


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("name", ["config4", "torture/csg_groups"])
def test_wave_tails(gpu, name, n):
    """The first n rays: the full batch's colours bit for bit, the oracle's
    counts over those n rays (a tail lane's replay of the last ray must not
    count), and nothing written past 3n doubles."""
    r = ref_of(gpu, name)
    full = gpu.query_radiance(r.sc, r.o, r.d)
    want = (int(r.ni[:n].sum()), int(r.no[:n].sum()))
    st = gpu.Stats()
    got = gpu.query_radiance(r.sc, r.o[:n], r.d[:n], stats=st)
    assert got.tobytes() == full[:n].tobytes()
    assert (st.rays_intersect, st.rays_occluded) == want
    cap = n + 50
    raw, st = _dev_radiance(gpu, r.sc, r.o, r.d, n, cap)
    assert raw[:n * 24].tobytes() == full[:n].tobytes()
    assert np.all(raw[n * 24:] == 0xAB)
    assert (st.rays_intersect, st.rays_occluded, st.rays_traced) == (want[0], want[1], want[0] + want[1])


# -------------------------------------------------------------- 5. shading inputs
@pytest.mark.parametrize("name", ["lights65_csg", "near_light_wave", "far_skip_few", "null_mat_csg"])
def test_shading_inputs(gpu, name):
    """More than 32 lights, a light nearer than the shadow epsilon / skipped
    lights, and null materials (built with with_null_materials)."""
    scene = scenes.shading_scenes(dpi=16)[name]
    sc = scenes.shading_load(gpu, name, scene)
    if name == "null_mat_csg":
        assert any(sc.desc.nodes[i].mat == -1 for i in gpu.sphere_nodes_at(sc, scenes.NULL_CENTRES))
    if name == "lights65_csg":
        assert sc.desc.n_lights > 32
    r = recipe_ref(gpu, "shading/" + name, sc, 192, 192, 7100 + len(name))
    check(gpu, r, gpu.query_radiance(sc, r.o, r.d), "shading/" + name)


# ------------------------------------------ 6. device entry point, large host batch
def test_device_entry_point_on_a_stream(gpu):
    r = ref_of(gpu, "torture/xform_in_csg")
    n = len(r)
    hs = gpu.Stats()
    host = gpu.query_radiance(r.sc, r.o, r.d, stats=hs)
    stream = gpu.Stream()
    try:
        raw, st = _dev_radiance(gpu, r.sc, r.o, r.d, n, n, stream=stream)
    finally:
        stream.destroy()
    assert raw.tobytes() == host.tobytes()
    assert (st.rays_intersect, st.rays_occluded) == (hs.rays_intersect, hs.rays_occluded)
    with pytest.raises(ValueError):
        gpu.query_radiance_device(r.sc, gpu.DeviceBuffer(64), 2, gpu.DeviceBuffer(48))


def test_host_batch_larger_than_one_chunk(gpu):
    """More rays than one host chunk (2^20): the chunks' colours in order, the counts scaled."""
    r = ref_of(gpu, "config3")
    n = (1 << 20) + 69
    reps, rest = divmod(n, len(r))
    s_all, s_rest = gpu.Stats(), gpu.Stats()
    small = gpu.query_radiance(r.sc, r.o, r.d, stats=s_all)
    gpu.query_radiance(r.sc, r.o[:rest], r.d[:rest], stats=s_rest)
    o, d = np.tile(r.o, (reps + 1, 1))[:n], np.tile(r.d, (reps + 1, 1))[:n]
    st = gpu.Stats()
    got = gpu.query_radiance(r.sc, o, d, stats=st)
    assert got.tobytes() == np.tile(small, (reps + 1, 1))[:n].tobytes()
    assert st.rays_intersect == reps * s_all.rays_intersect + s_rest.rays_intersect
    assert st.rays_occluded == reps * s_all.rays_occluded + s_rest.rays_occluded


def test_small_host_chunks_are_the_default_chunk(gpu):
    """The host form's chunk forced to 100 rays (rt_test_camera_chunk_rays sets
    the one chunk size of every batched call) on a scene that reflects and
    refracts: 1000 rays cross ten chunks, each ending in a partial wave whose
    tail lanes replay a ray and must neither store nor count, and the counters
    accumulate over the chunks and the bounces.  The same bytes and counts as
    at the default chunk, and the oracle's counts."""
    r = ref_of(gpu, "torture/reflect_refract")
    d = r.sc.desc
    assert any(d.materials[i].kr > 0.0 or d.materials[i].kt > 0.0 for i in range(d.n_materials))
    n = 1000
    reps = -(-n // len(r))
    o, dirs = np.tile(r.o, (reps, 1))[:n], np.tile(r.d, (reps, 1))[:n]
    s0, s1 = gpu.Stats(), gpu.Stats()
    want = gpu.query_radiance(r.sc, o, dirs, stats=s0)
    gpu.camera_chunk_rays(100)
    try:
        gpu.launch_log(True)
        got = gpu.query_radiance(r.sc, o, dirs, stats=s1)
        launches = gpu.launch_log_get()
    finally:
        gpu.launch_log(False)
        gpu.camera_chunk_rays(0)
    assert len(launches) == 10 and all("k_radiance" in k for k in launches)   # (ten chunks)
    assert got.tobytes() == want.tobytes()
    counts = (int(np.tile(r.ni, reps)[:n].sum()), int(np.tile(r.no, reps)[:n].sum()))
    for s in (s0, s1):
        assert (s.rays_intersect, s.rays_occluded, s.rays_traced) == (counts[0], counts[1], sum(counts))
    assert counts[0] > n   # (bounces were traced)


# ------------------------------------------------ 7. degenerate directions, ranges
def test_zero_length_direction_and_unread_ranges(gpu):
    """A direction of length <= 1e-6 is (0, 1, 0) (core.h:95-101, 278); tmin and
    tmax of rt_ray are not read."""
    c = case(gpu, "config5")
    lib = gpu.amd_lib()
    origins = np.array([[-3.5, -1.55, -2.0], [0.5, -1.58, -2.0], [2.5, -1.0, -4.0], [0.0, 0.0, 5.0], [0.0, -3.0, -2.0]])
    up = np.tile(np.array([0.0, 1.0, 0.0]), (len(origins), 1))
    want = gpu.query_radiance(c.scene, origins, up)
    ref, _, _ = gpu.oracle_trace(c.scene, origins, up)
    assert float(np.abs(want - ref).max()) <= TOL
    assert len({tuple(v) for v in want}) > 1   # (not all the background)
    for d in ([0.0, 0.0, 0.0], [1e-300, 0.0, 0.0], [0.0, -1e-300, 1e-300], [5e-7, 0.0, 0.0]):
        got = gpu.query_radiance(c.scene, origins, np.tile(np.array(d), (len(origins), 1)))
        assert got.tobytes() == want.tobytes(), d
    r = ref_of(gpu, "config5")
    base = gpu.query_radiance(r.sc, r.o, r.d)
    rays = gpu.make_rays(r.o, r.d, 0.0, 1e-9)   # nonsense ranges
    rgb = np.zeros((len(r), 3))
    assert lib.rt_query_radiance(r.sc.handle, rays.ctypes.data_as(C.c_void_p), len(r), 0, rgb.ctypes.data_as(C.c_void_p),
                                 None) == 0
    assert rgb.tobytes() == base.tobytes()


# ------------------------------------------------------------------ 8. residency
def test_frame_radiance_query_frame_share_the_resident_scene(gpu):
    """Frame -> radiance query -> intersect query -> frame of one scene: the
    scene is compiled and uploaded once (rt_setup_times[0] stops growing)."""
    lib = gpu.amd_lib()
    r = ref_of(gpu, "config4")
    c = case(gpu, "config4")
    sc = gpu.load_scene_from_json_text(SCENES["config4"][0])   # a scene handle no frame or query has seen
    t = (C.c_double * 4)()

    def scene_ms():
        assert lib.rt_setup_times(t, 4) == 0
        return t[0]

    ms0 = scene_ms()
    W, H = sc.width, sc.height
    fb = gpu.Tracer(sc, W, H, 0).render()
    ms1 = scene_ms()
    assert ms1 > ms0
    q1 = gpu.query_radiance(sc, r.o, r.d)
    h1 = gpu.query_intersect(sc, c.rays["o"], c.rays["d"])
    fb2 = gpu.Tracer(sc, W, H, 0).render()
    q2 = gpu.query_radiance(sc, r.o, r.d)
    assert scene_ms() == ms1
    assert np.array_equal(fb, fb2) and q1.tobytes() == q2.tobytes()
    assert h1.records.tobytes() == gpu.query_intersect(c.scene, c.rays["o"], c.rays["d"]).records.tobytes()
    assert q1.tobytes() == gpu.query_radiance(r.sc, r.o, r.d).tobytes()
    # and the reverse: a fresh handle's radiance query first, then its frame
    sc2 = gpu.load_scene_from_json_text(SCENES["config4"][0])
    q3 = gpu.query_radiance(sc2, r.o, r.d)
    ms2 = scene_ms()
    assert ms2 > ms1
    fb3 = gpu.Tracer(sc2, W, H, 0).render()
    assert scene_ms() == ms2 and np.array_equal(fb, fb3) and q3.tobytes() == q1.tobytes()


# --------------------------------------------------------------------- 9. errors
def test_errors(gpu):
    lib = gpu.amd_lib()
    r = ref_of(gpu, "config3")
    sc, n = r.sc, len(r)
    rays, rgb = gpu.make_rays(r.o, r.d), np.zeros((n, 3))
    rp, cp = rays.ctypes.data_as(C.c_void_p), rgb.ctypes.data_as(C.c_void_p)
    st = gpu.Stats()
    # n == 0: RT_OK without a launch, whatever the pointers
    st.rays_traced = 123
    gpu.launch_log(True)
    try:
        assert lib.rt_query_radiance(sc.handle, None, 0, 0, None, C.byref(st)) == 0
        assert lib.rt_query_radiance_device(sc.handle, None, 0, 0, None, None, None) == 0
        assert gpu.query_radiance(sc, np.zeros((0, 3)), np.zeros((0, 3))).shape == (0, 3)
        assert gpu.launch_log_get() == []
    finally:
        gpu.launch_log(False)
    assert (st.rays_intersect, st.rays_occluded, st.rays_traced, st.ms_kernel) == (0, 0, 0, 0.0)
    # NULL arguments
    for rc in (lib.rt_query_radiance(None, rp, n, 0, cp, None),
               lib.rt_query_radiance(sc.handle, None, n, 0, cp, None),
               lib.rt_query_radiance(sc.handle, rp, n, 0, None, None),
               lib.rt_query_radiance_device(None, rp, n, 0, cp, None, None),
               lib.rt_query_radiance_device(sc.handle, None, n, 0, cp, None, None),
               lib.rt_query_radiance_device(sc.handle, rp, n, 0, None, None, None)):
        assert rc == gpu.RT_ERR_INVALID_ARG
        assert "NULL" in gpu.last_error()
    # refused flags, with a message (also at n == 0); NULL stats are fine
    for flag, word in ((gpu.RT_FLAG_FP32, "FP32"), (gpu.RT_FLAG_COUNT_OPS, "COUNT_OPS")):
        assert lib.rt_query_radiance(sc.handle, rp, n, flag, cp, None) == gpu.RT_ERR_UNSUPPORTED
        assert word in gpu.last_error()
        assert lib.rt_query_radiance(sc.handle, None, 0, flag, None, None) == gpu.RT_ERR_UNSUPPORTED
        with pytest.raises(gpu.RTError) as e:
            gpu.query_radiance(sc, r.o, r.d, flag)
        assert e.value.code == gpu.RT_ERR_UNSUPPORTED
    assert lib.rt_query_radiance(sc.handle, rp, n, 1 << 20, cp, None) == gpu.RT_ERR_INVALID_ARG
    assert lib.rt_query_radiance(sc.handle, rp, n, 0, cp, None) == 0
    assert rgb.tobytes() == gpu.query_radiance(sc, r.o, r.d).tobytes()


def test_scene_beyond_the_big_stacks_is_refused(gpu):
    leaves = [{"sphere": {"position": [0.01 * i, 0, -2], "radius": 0.5, "color": {"diffuse": [1, 1, 1]}}}
              for i in range(80)]
    node = leaves[-1]
    for leaf in reversed(leaves[:-1]):
        node = {"csg": {"operator": "union", "left": leaf, "right": node}}
    sc = gpu.load_scene_from_json_text(json.dumps({"screen": {"dpi": 4, "dimensions": [2, 2], "position": [-1, -1, 0],
                                                              "observer": [0, 0, 3]}, "objects": [node]}))
    with pytest.raises(gpu.RTError) as e:
        gpu.query_radiance(sc, [[0, 0, 3]], [[0, 0, -1]])
    assert e.value.code == gpu.RT_ERR_UNSUPPORTED and "CSG operand depth 80" in str(e.value)
    # and the next query works
    r = ref_of(gpu, "config3")
    got = gpu.query_radiance(r.sc, r.o[:64], r.d[:64])
    assert float(np.abs(got - r.rgb[:64]).max()) <= TOL


# -------------------------------------------------------------------- 10. census
@pytest.mark.parametrize("recipe", scenes.radiance_recipes(), ids=lambda r: r.row)
def test_census(gpu, recipe):
    """Every row of the radiance tables: a 256-ray query of its recipe's scene
    launches exactly that row, and its colours and counts are the oracle's."""
    text, lights = scenes.recipe_scene(recipe.scene_name)
    sc = gpu.load_scene_from_json_text(text)
    if lights:
        sc = gpu.with_dir_lights(sc, lights)
    r = recipe_ref(gpu, "census/" + recipe.scene_name, sc, 128, 128, 4242)
    assert len(r) == 256
    gpu.launch_log(True)
    try:
        got = gpu.query_radiance(sc, r.o, r.d, recipe.flags)
        log = gpu.launch_log_get()
    finally:
        gpu.launch_log(False)
    assert log == [recipe.row]
    check(gpu, r, got, recipe.row, recipe.flags)
    assert (np.abs(r.rgb - r.background).max(axis=1) > 0).sum() >= len(r) // 4
    sec = recipe.row.split("<")[1].split(",")[2].strip() == "true"
    if sec:
        assert int(r.ni.sum()) > len(r), "no ray of this batch bounced"
