"""The launch tables against scenes.kernel_recipes(): every row of every table
(rt_test_kernel_row reads them from the arrays the launchers search: the
standard and paper tables of rtd, rtf and rtdb, the query tables, the finish
kernels) has exactly one recipe, and the frame's own kernel choice
(rt_test_kernel_name / rt_test_query_kernel_name) for a recipe's scene, mode
and flags is that row.  A row added without a recipe, or a recipe whose scene
stops picking its row, fails here without a device;
tests/test_gpu_kernel_table.py renders every recipe and pins what was
launched.

rt_test_kernel_name never reports a timed paper kernel (T = true: the first
frame of a scene handle), so those rows are held here on their untimed name
and by the launch log on the GPU."""
import collections

import pytest

import scenes

RECIPES = scenes.kernel_recipes()

def recipe_id(r):
    return f"{r.row}@{r.scene_name}/m{r.mode}/f{r.flags}/frame{r.frame}".replace(" ", "")


@pytest.fixture(scope="module")
def lib(rt):
    rt.amd_lib()
    return rt


def test_every_table_row_has_one_recipe(lib):
    tables = {name: lib.kernel_rows(t) for t, name in enumerate(lib.KERNEL_TABLES)}
    assert all(tables[k] for k in ("rtd std", "rtd paper", "rtdb std", "rtdb paper", "rtd query", "rtdb query", "finish"))
    rows = [r for v in tables.values() for r in v]
    assert len(set(rows)) == len(rows), [r for r, n in collections.Counter(rows).items() if n > 1]
    have = collections.Counter(r.row for r in RECIPES)
    assert not [r for r, n in have.items() if n > 1], "duplicate recipes"
    assert sorted(set(rows) - set(have)) == [], "table rows without a recipe"
    assert sorted(set(have) - set(rows)) == [], "recipes for rows no table has"
    import ctypes as C
    buf = C.create_string_buffer(160)
    assert lib.amd_lib().rt_test_kernel_row(len(tables), 0, buf, 160) == lib.RT_ERR_INVALID_ARG   # (past the last table)
    assert lib.amd_lib().rt_test_kernel_row(0, -1, buf, 160) == lib.RT_ERR_INVALID_ARG


def test_row_names_carry_their_namespace(lib):
    for t, name in enumerate(lib.KERNEL_TABLES):
        for row in lib.kernel_rows(t):
            ns = row.split("::")[0]
            assert ns == name.split()[0] if name != "finish" else ns in ("rtd", "rtf"), (name, row)


@pytest.mark.parametrize("r", [r for r in RECIPES if "k_paper_finish" not in r.row], ids=recipe_id)
def test_recipe_names_its_row(lib, r):
    text, lights = scenes.recipe_scene(r.scene_name)
    sc = lib.load_scene_from_json_text(text)
    if lights:
        sc = lib.with_dir_lights(sc, lights)
    if r.query >= 0:
        rc, name = lib.query_kernel_name(sc, r.query, r.flags)
    else:
        rc, name = lib.kernel_name(sc, r.mode, r.flags)
    assert rc == 0, lib.last_error()
    assert name == scenes.row_timed(r.row, False)
    timed = scenes.row_timed(r.row, True) == r.row and scenes.row_timed(r.row, False) != r.row
    if r.mode == 1 and r.query < 0:
        # the first frame of a handle launches the timed build unless it counts ops
        assert r.frame == (0 if timed or (r.flags & lib.RT_FLAG_COUNT_OPS) else 1)
    else:
        assert r.frame == 0 and not timed


@pytest.mark.parametrize("r", [r for r in RECIPES if "k_paper_finish" in r.row], ids=recipe_id)
def test_finish_recipe_shape(lib, r):
    """k_paper_finish<CODES, PAIR>: PAIR is the width's parity, CODES a rank of
    a distributed FP64 frame."""
    text, _ = scenes.recipe_scene(r.scene_name)
    sc = lib.load_scene_from_json_text(text)
    ns, args = r.row.split("::k_paper_finish<")
    codes, pair = (v.strip() == "true" for v in args.rstrip(">").split(","))
    assert r.mode == 1 and pair == (sc.width % 2 == 0)
    assert codes == (r.world > 1) and not (codes and r.flags & lib.RT_FLAG_FP32)
    assert ns == ("rtf" if r.flags & lib.RT_FLAG_FP32 else "rtd")
    assert sc.height > 30 or r.world == 1   # (RT_PAPER_STRIP_ROWS: both ranks get rows)


def test_row_timed():
    assert scenes.row_timed("rtd::k_paper_primary<true, true, false>", True) == "rtd::k_paper_primary<true, true, false, true>"
    assert scenes.row_timed("rtd::k_paper_primary<true, true, false, true>", False) == "rtd::k_paper_primary<true, true, false>"
    assert scenes.row_timed("rtf::k_paper_primary_lean<false, 2, false, true>", True) == \
        "rtf::k_paper_primary_lean<false, 2, true, true>"
    assert scenes.row_timed("rtd::k_std_lean<false, 1, true>", True) == "rtd::k_std_lean<false, 1, true>"


def test_launch_log_records_only_while_on(lib):
    """The log's host side (no launch happens here): on clears, off stops, get
    returns the count and refuses a buffer that is too small."""
    import ctypes as C
    lib.launch_log(True)
    assert lib.launch_log_get() == []
    lib.launch_log(False)
    assert lib.launch_log_get() == []
    buf = C.create_string_buffer(1)
    assert lib.amd_lib().rt_test_launch_log_get(buf, 1) == 0 and buf.value == b""
    assert lib.amd_lib().rt_test_launch_log_get(None, 0) == lib.RT_ERR_INVALID_ARG
