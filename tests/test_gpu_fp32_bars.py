"""The FP32 kernels (RT_FLAG_FP32: the rtf namespace, the same templates with
real = float, contraction and approximate division / square root) against the
oracle PIXEL BY PIXEL, by the stability bars of tests/fp32_bars.py: every
channel of every standard-mode pixel within its pixel's bar, every stable
pixel of a paper frame bit-equal.  The bars come from the reference alone
(tests/test_fp32_bars.py holds them on the CPU, and shows three small shading
mistakes that pass the whole-frame bars of tests/test_gpu_fp32.py and fail
these).  Those whole-frame tests stay beside this file as they are.

Exceptions exist only through fp32_bars.EXCEPTIONS.

Measured on an MI355X: the first run found three faults of the float build
(DESIGN.md Numerics: the paper frames held float-rounded values of the output
alphabet; CSG::interval's 1e-6 origin test put a third of the rays refracted
into a CSG solid on the wrong side of its surface; the sphere discriminant
cancelled and moved small, far and grazed spheres by more than the bars
allow).  With them fixed every case passes with an empty exception table, the
largest |d| / bar over all standard frames being 0.25.

Run with -s: every case prints its pixels, its unconstrained (unstable) share,
how many pixels are over the bar (0) and the largest and median |d| / bar
(profiles/fp32_bars/gpu_tests.txt)."""
import pytest

import fp32_bars as B
from test_fp32_bars import EDGES, RTF, scene_of
from test_gpu_kernel_table import _finish_row, _frames, _load
from test_gpu_parity import SMALL
from test_kernel_table import recipe_id

pytestmark = pytest.mark.gpu


def _hold(rt, case_id, text, lights, seed, mode, fb, counts):
    if mode == 1:
        ref, stable = B.paper_stable(rt, text, lights, seed)
        B.held32_paper(case_id, fb, ref, stable)
        return
    r = B.standard_case(rt, text, lights, seed)
    B.held32(case_id, fb, r.ref, r.bar)
    if r.ray_free:   # no decision of this frame's trace is near its edge: the ray counts are the oracle's own
        assert counts == r.counts, (case_id, counts, r.counts)


@pytest.mark.parametrize("no_cull", [False, True], ids=["cull", "no_cull"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_frames(gpu, name, mode, no_cull):
    text, lights, seed = scene_of("small/" + name)
    flags = gpu.RT_FLAG_FP32 | (gpu.RT_FLAG_NO_CULL if no_cull else 0)
    (fb, counts, log), = _frames(gpu, gpu.load_scene_from_json_text(text), mode, flags, 1)
    assert log and all(k.startswith("rtf::") for k in log), log
    _hold(gpu, f"frame {name}/m{mode}/f{flags}", text, lights, seed, mode, fb, counts)


@pytest.mark.parametrize("r", RTF, ids=recipe_id)
def test_every_rtf_row(gpu, r):
    """Every row of the rtf launch tables through its recipe (wave culls, the
    wave BVH, k_std_secw, the counting builds, the timed and untimed paper
    builds, the finish kernels), the row asserted in the launch log; every
    frame the recipe renders is held."""
    text, lights, seed = scene_of("recipe/" + r.scene_name)
    sc = _load(gpu, r)
    frames = _frames(gpu, sc, r.mode, r.flags, r.frame + 1)
    log = frames[r.frame][2]
    if "k_paper_finish" in r.row:
        assert log[1:] == [r.row] and "k_paper_primary" in log[0], log
    else:
        assert log == [r.row] + ([_finish_row(gpu, sc, r.flags)] if r.mode == 1 else []), log
    for k, (fb, counts, _) in enumerate(frames):
        _hold(gpu, f"row {recipe_id(r)}" + (f" (frame {k})" if k != r.frame else ""), text, lights, seed, r.mode, fb, counts)


def test_the_rtf_rows_are_all_here(gpu):
    have = {r.row for r in RTF}
    for t, name in enumerate(gpu.KERNEL_TABLES):
        rows = gpu.kernel_rows(t)
        if name.startswith("rtf "):
            assert rows and set(rows) <= have, name
        assert {row for row in rows if row.startswith("rtf::")} <= have, name


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", EDGES)
def test_partial_waves(gpu, case, mode):
    """cfg4 at 3x17 and 1x1 (tests/test_gpu_edges.py): every wave is a partial one."""
    text, lights, seed = scene_of(case)
    sc = gpu.load_scene_from_json_text(text)
    assert f"{sc.width}x{sc.height}" == case.split("@")[1]
    (fb, counts, log), = _frames(gpu, sc, mode, gpu.RT_FLAG_FP32, 1)
    assert log and all(k.startswith("rtf::") for k in log), log
    _hold(gpu, f"frame {case}/m{mode}", text, lights, seed, mode, fb, counts)
