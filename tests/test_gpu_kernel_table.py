"""A launch census: every row of every launch table (rt_kernels.hpp kStdKernels /
kPaperKernels / kFinishKernels of rtd, rtf and rtdb, rt_query_kernels.hpp
kQueryKernels) is launched once through its recipe (scenes.kernel_recipes();
tests/test_kernel_table.py holds the list against the tables), the launch is
observed in the launch log (rt_test_launch_log: what the launchers were asked
for, BVH trial frames and timed paper builds included, which
rt_test_kernel_name cannot see), and the frame is compared with the CPU oracle.

Bars.  rtd / rtdb: per channel |d| <= 1e-5, ray counts equal to the oracle's,
paper mode bit-exact.  Op-counting rows: also bit-identical to the same frame
without RT_FLAG_COUNT_OPS.  rtf: the bars of tests/test_gpu_fp32.py.  A recipe
of frame 1 (the untimed paper kernels, what every frame but a scene's first
runs) also requires frame 0 to have launched the timed twin and both frames to
be bit-identical: the costliest-first launch order of warm frames changes no
pixel.  Query rows: 256 rays of tests/test_gpu_query.py's recipe at its bars.

The rtf wave-BVH rows render bvh/nested and bvh/nested_mirror, the lattice of
bvh/ties without a tie: in FP32 bvh/ties itself is 4.05 % far from the oracle
(whole spheres take the colour of their coincident twin once rounding breaks
the exact FP64 equality of t), which is the scene's doing and recorded in
profiles/kernel_table_fp32_culls.txt, not asserted.

FP32 culls (test_fp32_culls_move_only_silhouettes): every rtf row with wave
culls (WV = 1) or the wave BVH (WV = 2), and the 300-sphere perf scene whose
sub-pixel spheres make many rays graze a bound, against the same FP32 frame
with RT_FLAG_NO_CULL.  Measured on MI355X (same file): FP32 frames are not
invariant under culling.  On the lattice the k_std_lean and paper rows are
bit-identical to the unculled frame and the k_std_secw rows (trace_wave
against the general k_std<false, false, true>: other code) differ in the last
bit of 4.6 % of the channels.  On the perf scene the culls bite: one pixel
moves by 0.07 and one shadow query goes.  There the culled frame equals the
oracle to 9e-8 and the unculled one is 0.16 off: the cull removed a hit that
the FP32 discriminant invented for a ray that misses the sphere, it dropped no
real one.  So the test asserts the project's silhouette cap (at most FAR_FRAC
of the channels move by more than 1e-3) and that on the moved channels the
culled frame is no farther from the oracle than the unculled one."""
import numpy as np
import pytest

import scenes
from test_gpu_fp32 import FAR_FRAC, FAR_FRAC_SECONDARY, MEAN_TOL
from test_gpu_query import SCENES as QUERY_SCENES, case as query_case, check_hits, check_occluded, q_isect, q_occl
from test_kernel_table import RECIPES, recipe_id

pytestmark = pytest.mark.gpu

TOL = 1e-5
N_QUERY = 256

_oracle = {}


def _load(rt, r):
    """A fresh scene handle (its first paper frame is the timed one)."""
    text, lights = scenes.recipe_scene(r.scene_name)
    sc = rt.load_scene_from_json_text(text)
    return rt.with_dir_lights(sc, lights) if lights else sc


def _oracle_frame(rt, r, sc):
    key = (r.scene_name, r.mode, sc.width, sc.height)
    if key not in _oracle:
        ref, ost = rt.oracle_render(sc, sc.width, sc.height, r.mode, threads=8)
        ref.setflags(write=False)
        _oracle[key] = (ref, (int(ost.rays_intersect), int(ost.rays_occluded)))
    return _oracle[key]


def _frames(rt, sc, mode, flags, n):
    """n frames of one Tracer: [(frame, ray counts, kernels launched)]."""
    t = rt.Tracer(sc, sc.width, sc.height, mode, flags=flags)
    out = []
    for _ in range(n):
        st = rt.Stats()
        rt.launch_log(True)
        try:
            fb = t.render(st)
            log = rt.launch_log_get()
        finally:
            rt.launch_log(False)
        out.append((fb, (int(st.rays_intersect), int(st.rays_occluded)), log))
    return out


def _ns(rt, flags):
    return "rtf" if flags & rt.RT_FLAG_FP32 else "rtd"


def _finish_row(rt, sc, flags):
    # a one-GPU frame's finish kernel (big-stack frames finish with rtd's: the pass reads records only)
    return f"{_ns(rt, flags)}::k_paper_finish<false, {'true' if sc.width % 2 == 0 else 'false'}>"


def _secondary(sc):
    d = sc.desc
    return d.recursion_limit >= 2 and any(d.materials[i].kr > 0 or d.materials[i].kt > 0 for i in range(d.n_materials))


def _check_frame(rt, r, sc, fb, counts):
    ref, ocounts = _oracle_frame(rt, r, sc)
    d = np.abs(fb - ref)
    assert fb.shape == ref.shape and np.isfinite(fb).all()
    if r.flags & rt.RT_FLAG_FP32:
        far = float(np.mean(d > 1e-3))
        n_gpu, n_ref = sum(counts), sum(ocounts)
        print(f"  {recipe_id(r)} fp32 far={far:.5f} mean={d.mean():.2e} max={d.max():.3g} rays gpu={n_gpu} oracle={n_ref}")
        assert far <= (FAR_FRAC_SECONDARY if _secondary(sc) else FAR_FRAC)
        assert d.mean() <= MEAN_TOL
        assert abs(n_gpu - n_ref) <= 0.05 * n_ref + 16
    else:
        print(f"  {recipe_id(r)} max|d|={d.max():.3g} rays gpu={counts} oracle={ocounts}")
        assert d.max() <= TOL
        assert counts == ocounts
        if r.mode == 1:
            assert np.array_equal(fb, ref), "paper mode must be bit-exact"


TRACE = [r for r in RECIPES if r.query < 0 and "k_paper_finish" not in r.row]


@pytest.mark.parametrize("r", TRACE, ids=recipe_id)
def test_trace_row_launches_and_matches_oracle(gpu, r):
    sc = _load(gpu, r)
    frames = _frames(gpu, sc, r.mode, r.flags, r.frame + 1)
    fb, counts, log = frames[r.frame]
    print(f"  frame {r.frame} launched {log}")
    want = [r.row] + ([_finish_row(gpu, sc, r.flags)] if r.mode == 1 else [])
    assert log == want
    if r.frame == 1:
        fb0, counts0, log0 = frames[0]
        assert log0 == [scenes.row_timed(r.row, True), want[1]]
        assert counts0 == counts and np.array_equal(fb0, fb), "the warm frame's launch order changed the frame"
    _check_frame(gpu, r, sc, fb, counts)
    if r.flags & gpu.RT_FLAG_COUNT_OPS:
        (plain, pcounts, plog), = _frames(gpu, _load(gpu, r), r.mode, r.flags & ~gpu.RT_FLAG_COUNT_OPS, 1)
        assert plog[0] != r.row
        assert pcounts == counts and np.array_equal(plain, fb), "op counting changed the frame"


def _wv(row):   # the WV argument of k_std_lean / k_std_secw / k_paper_primary_lean<C, WV, ...>; other rows: 0
    head, _, args = row.partition("<")
    return int(args.split(",")[1]) if head.split("::")[1] in ("k_std_lean", "k_std_secw", "k_paper_primary_lean") else 0


# ... and a scene where the culls bite: bvh_perf_scene(300)'s spheres are 0.1 - 1.5 pixels wide at 64x48, so a
# large share of its rays graze a bound (not a row's recipe: at that size FP32 misses FAR_FRAC against the oracle)
FP32_CULLED = [r for r in TRACE if r.row.startswith("rtf::") and _wv(r.row) != 0] + [
    scenes.Recipe("rtf::k_std_lean<false, 1, false>", "bvh/perf300", 0, 4 | 8, 0),
    scenes.Recipe("rtf::k_std_lean<false, 2, false>", "bvh/perf300", 0, 4 | 16, 0)]


@pytest.mark.parametrize("r", FP32_CULLED, ids=recipe_id)
def test_fp32_culls_move_only_silhouettes(gpu, r):
    """The row's frame against the same FP32 frame with RT_FLAG_NO_CULL; see
    the module docstring for the measurement these bars rest on.  The cull
    tests (rt_device.hpp ball_touch) are conservative for the exact geometry,
    with margins above their own float rounding, so a culled object is one the
    ray truly misses: where the two frames differ, the unculled FP32 trace
    found a hit that is not there, and the culled frame must be no farther from
    the oracle than the unculled one."""
    bvh_flags = gpu.RT_FLAG_NO_BVH | gpu.RT_FLAG_FORCE_BVH
    sc = _load(gpu, r)
    a, ca, la = _frames(gpu, sc, r.mode, r.flags, r.frame + 1)[r.frame]
    (b, cb, lb), = _frames(gpu, _load(gpu, r), r.mode, (r.flags & ~bvh_flags) | gpu.RT_FLAG_NO_CULL, 1)
    assert la[0] == r.row
    assert _wv(lb[0]) == 0 and lb[0].startswith("rtf::"), lb
    ref, _ = _oracle_frame(gpu, r, sc)
    d = np.abs(a - b)
    moved = d > 1e-3
    far = float(np.mean(moved))
    ea, eb = float(np.abs(a - ref)[moved].sum()), float(np.abs(b - ref)[moved].sum())
    print(f"  {recipe_id(r)} culled vs NO_CULL: far={far:.5f} differing={float(np.mean(a != b)):.5f} max={d.max():.3g} "
          f"rays {ca} vs {cb}; on the moved channels sum|culled - oracle|={ea:.4g} sum|NO_CULL - oracle|={eb:.4g}, "
          f"culled closer on {int((np.abs(a - ref) < np.abs(b - ref))[moved].sum())} of {int(moved.sum())}")
    assert np.isfinite(a).all() and np.isfinite(b).all()
    assert far <= FAR_FRAC
    assert abs(sum(ca) - sum(cb)) <= 0.05 * sum(cb) + 16
    if r.mode == 0 and not _secondary(sc):
        # (with reflection the two frames come from different kernels, trace_wave and the general k_std: their
        # difference is arithmetic, not culls)
        assert ea <= eb


QUERY = [r for r in RECIPES if r.query >= 0]


@pytest.mark.parametrize("r", QUERY, ids=recipe_id)
def test_query_row_launches_and_matches_oracle(gpu, r):
    name = r.scene_name.split("/", 1)[1]
    assert QUERY_SCENES[name] == scenes.recipe_scene(r.scene_name)   # (the recipe's scene is test_gpu_query's)
    c = query_case(gpu, name)
    gpu.launch_log(True)
    try:
        if r.query == 0:
            got = q_isect(gpu, c.scene, c.rays[:N_QUERY])
        else:
            got = q_occl(gpu, c.scene, c.seg_rays[:N_QUERY])
        log = gpu.launch_log_get()
    finally:
        gpu.launch_log(False)
    print(f"  launched {log}")
    assert log == [r.row]
    if r.query == 0:
        check_hits(c, c.rays[:N_QUERY], got, c.ref_hit[:N_QUERY], c.ref_rec[:N_QUERY], recipe_id(r))
        assert c.ref_hit[:N_QUERY].sum() >= N_QUERY // 4
    else:
        check_occluded(c, c.seg_rays[:N_QUERY], got, c.ref_occ[:N_QUERY], recipe_id(r))
        assert 0 < c.ref_occ[:N_QUERY].sum() < N_QUERY


FINISH = [r for r in RECIPES if "k_paper_finish" in r.row]


@pytest.mark.parametrize("r", FINISH, ids=recipe_id)
def test_finish_row_launches_and_matches_oracle(gpu, r):
    sc = _load(gpu, r)
    (one, counts, log), = _frames(gpu, sc, 1, r.flags, 1)
    assert log[1:] == [_finish_row(gpu, sc, r.flags)] and "k_paper_primary" in log[0]
    _check_frame(gpu, r, sc, one, counts)
    if r.world == 1:
        assert log[1] == r.row
        return
    # CODES: the ranks of a distributed frame write one byte per pixel, the root decodes
    gpu.launch_log(True)
    try:
        got = gpu.render_dist_sim(sc, sc.width, sc.height, 1, r.world, flags=r.flags)
        log = gpu.launch_log_get()
    finally:
        gpu.launch_log(False)
    print(f"  {r.world} ranks launched {log}")
    fin = [k for k in log if "k_paper_finish" in k]
    assert len(fin) >= r.world and set(fin) == {r.row}
    assert np.array_equal(got, one)
