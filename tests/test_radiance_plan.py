"""Radiance queries on the CPU (no device is touched): the reference the GPU
tests use, rtamd.oracle_trace, held to the oracle's own frames; the kernel a
radiance query launches (frame_plan.cpp pick_radiance_variant + the radiance
table of rt_radiance_kernels.hpp) through rt_test_radiance_kernel_name; and
the census list scenes.radiance_recipes() against the tables.  The kernels'
results are checked against the oracle by tests/test_gpu_radiance.py."""
import ctypes as C
import json

import numpy as np
import pytest

import scenes

RT_ERR_INVALID_ARG, RT_ERR_UNSUPPORTED = -1, -6


def _args(name):
    return [a.strip() for a in name.split("<", 1)[1].rsplit(">", 1)[0].split(",")]


def _kernel(rt, sc, flags=0):
    rc, name = rt.radiance_kernel_name(sc, flags)
    assert rc == 0, rt.last_error()
    assert "::k_radiance<" in name and len(_args(name)) == 4   # E, D, SEC, PL
    return name


def _frame_kernel(rt, sc, mode=0, flags=0):
    buf = C.create_string_buffer(160)
    rc = rt.amd_lib().rt_test_kernel_name(sc.handle, mode, flags, buf, 160)
    return rc, buf.value.decode()


def _load(rt, name):
    text, lights = scenes.recipe_scene(name)
    sc = rt.load_scene_from_json_text(text)
    return rt.with_dir_lights(sc, lights) if lights else sc


# ------------------------------------------------ the reference's reference
@pytest.mark.parametrize("name", ["config3", "torture/reflect_refract"])
def test_oracle_trace_over_the_frames_rays_is_oracle_render(rt, name):
    """The frame's own 8 W H jittered rays through oracle_trace, averaged per
    pixel in sample order, are oracle_render's frame: colours within 1e-9
    (measured 1.8e-12: oracle_trace re-normalises P - o) and the Scene::intersect
    / Scene::occluded counts exactly equal."""
    text = scenes.config_json(3, dpi=24)[0] if name == "config3" else json.dumps(scenes.torture_scenes(dpi=24)[name[8:]])
    sc = rt.load_scene_from_json_text(text)
    W, H = sc.width, sc.height
    ref, ost = rt.oracle_render(sc, W, H, 0, threads=8)
    o, d = rt.oracle_frame_rays(sc)
    rgb, ni, no = rt.oracle_trace(sc, o.reshape(-1, 3), d.reshape(-1, 3))
    rgb = rgb.reshape(H, W, 8, 3)
    acc = np.zeros((H, W, 3))
    for s in range(8):   # (acc += trace(...) for s = 0..7 in order, then x 1/8)
        acc += rgb[:, :, s]
    acc *= 1.0 / 8.0
    err = float(np.abs(acc - ref).max())
    print(f"  {name}: {W}x{H}, {8 * W * H} rays, max|d|={err:.3g}, counts ({int(ni.sum())}, {int(no.sum())})")
    assert err <= 1e-9
    assert (int(ni.sum()), int(no.sum())) == (ost.rays_intersect, ost.rays_occluded)
    assert ni.min() >= 1   # (every ray is one Scene::intersect call at least)
    assert np.array_equal(rt.oracle_trace_dirs(o.reshape(-1, 3), d.reshape(-1, 3)),
                          (o.reshape(-1, 3) + d.reshape(-1, 3)) - o.reshape(-1, 3))


# ------------------------------------------------------------ kernel choice
def test_config3_takes_a_plain_row(rt):
    sc = rt.load_scene_from_json_text(scenes.config_json(3, dpi=24)[0])
    k = _kernel(rt, sc)
    assert k.startswith("rtd::") and _args(k)[3] == "true", k
    # RT_FLAG_NO_CULL changes the scene argument, not the kernel; the BVH flags nothing
    for f in (rt.RT_FLAG_NO_CULL, rt.RT_FLAG_NO_BVH, rt.RT_FLAG_FORCE_BVH):
        assert _kernel(rt, sc, f) == k


def test_config4_takes_a_csg_row(rt):
    sc = rt.load_scene_from_json_text(scenes.config_json(4, dpi=24)[0])
    k = _kernel(rt, sc)
    assert k.startswith("rtd::") and _args(k)[0] == "false" and _args(k)[3] == "false", k
    assert _kernel(rt, sc, rt.RT_FLAG_NO_CULL) == k


def test_secondary_follows_the_frames_rule(rt):
    """SEC as for a frame: some material reflects or refracts, and
    recursion_limit >= 2."""
    s = scenes.shading_scenes(dpi=16)
    mirrors = rt.load_scene_from_json_text(json.dumps(s["media_few_rec2"]))
    rec1 = rt.load_scene_from_json_text(json.dumps(s["media_few_rec1"]))
    assert mirrors.desc.recursion_limit == 2 and rec1.desc.recursion_limit == 1
    assert _args(_kernel(rt, mirrors))[2] == "true"
    assert _args(_kernel(rt, rec1))[2] == "false"
    # config 4 has no reflecting or refracting material
    cfg4 = rt.load_scene_from_json_text(scenes.config_json(4, dpi=24)[0])
    d = cfg4.desc
    assert d.recursion_limit >= 2 and not any(d.materials[i].kr > 0 or d.materials[i].kt > 0 for i in range(d.n_materials))
    assert _args(_kernel(rt, cfg4))[2] == "false"
    # the same scene with a mirror does
    assert _args(_kernel(rt, rt.with_material_fields(cfg4, {0: {"kr": 0.5}})))[2] == "true"


def test_mirrors_rec24_takes_the_big_stacks(rt):
    """Unlike the hit queries, a radiance query needs the frame's recursion
    frames: mirrors_rec24 runs where its frames run."""
    sc = rt.load_scene_from_json_text(json.dumps(scenes.deep_scenes()["mirrors_rec24"]))
    assert _kernel(rt, sc) == "rtdb::k_radiance<true, true, true, false>"
    assert _frame_kernel(rt, sc)[1].startswith("rtdb::")
    assert rt.query_kernel_name(sc, 0)[1].startswith("rtd::")


@pytest.mark.parametrize("name", sorted(scenes.deep_scenes()))
def test_deep_scenes_take_their_frames_namespace(rt, name):
    sc = rt.load_scene_from_json_text(json.dumps(scenes.deep_scenes()[name]))
    assert _kernel(rt, sc).split("::")[0] == _frame_kernel(rt, sc)[1].split("::")[0] == "rtdb"


@pytest.mark.parametrize("which", sorted(scenes.torture_scenes()))
def test_torture_scenes_have_a_radiance_kernel(rt, which):
    sc = rt.load_scene_from_json_text(json.dumps(scenes.torture_scenes(dpi=12)[which]))
    e, d, sec, pl = _args(_kernel(rt, sc))
    assert pl == "false"                           # every one holds a transform or CSG object
    assert not (e == "true" and d == "false")      # eager scenes always use D
    assert not (e == "true" and sec == "false")    # and the general row


def test_refused_flags(rt):
    sc = rt.load_scene_from_json_text(scenes.config_json(3, dpi=24)[0])
    rc, _ = rt.radiance_kernel_name(sc, rt.RT_FLAG_FP32)
    assert rc == RT_ERR_UNSUPPORTED and "FP32" in rt.last_error()
    rc, _ = rt.radiance_kernel_name(sc, rt.RT_FLAG_COUNT_OPS)
    assert rc == RT_ERR_UNSUPPORTED and "COUNT_OPS" in rt.last_error()
    buf = C.create_string_buffer(16)
    assert rt.amd_lib().rt_test_radiance_kernel_name(None, 0, buf, 16) == RT_ERR_INVALID_ARG


def test_scene_beyond_the_big_stacks_is_refused_like_its_frames(rt):
    leaves = [{"sphere": {"position": [0.01 * i, 0, -2], "radius": 0.5, "color": {"diffuse": [1, 1, 1]}}}
              for i in range(80)]
    node = leaves[-1]
    for leaf in reversed(leaves[:-1]):
        node = {"csg": {"operator": "union", "left": leaf, "right": node}}
    sc = rt.load_scene_from_json_text(json.dumps({"screen": {"dpi": 4, "dimensions": [2, 2], "position": [-1, -1, 0],
                                                             "observer": [0, 0, 3]}, "objects": [node]}))
    assert _frame_kernel(rt, sc)[0] == RT_ERR_UNSUPPORTED
    frame_msg = rt.last_error()
    rc, _ = rt.radiance_kernel_name(sc)
    assert rc == RT_ERR_UNSUPPORTED and "CSG operand depth 80" in rt.last_error()
    assert rt.last_error() == frame_msg


def test_recursion_beyond_the_big_stacks_is_refused_like_its_frames(rt):
    sc = rt.load_scene_from_json_text(json.dumps(scenes.deep_recursion_scene(131)))
    assert _frame_kernel(rt, sc)[0] == RT_ERR_UNSUPPORTED
    frame_msg = rt.last_error()
    assert rt.radiance_kernel_name(sc)[0] == RT_ERR_UNSUPPORTED and rt.last_error() == frame_msg
    assert rt.query_kernel_name(sc, 0)[0] == 0   # (a hit query traces one ray)


# ------------------------------------------------------------------- census
def test_every_row_has_exactly_one_recipe(rt):
    recipes = scenes.radiance_recipes()
    assert len(rt.RADIANCE_TABLES) == 2
    rows = []
    for table, ns in enumerate(("rtd", "rtdb")):
        got = rt.radiance_rows(table)
        assert got and all(r.startswith(ns + "::k_radiance<") for r in got), (table, got)
        assert len(set(got)) == len(got)
        rows += got
    assert rt.radiance_rows(0)[0] == "rtd::k_radiance<true, true, true, false>"
    assert rt.radiance_rows(1) == ["rtdb::k_radiance<true, true, true, false>"]
    assert sorted(r.row for r in recipes) == sorted(rows)   # one each, none for a row no table has


@pytest.mark.parametrize("recipe", scenes.radiance_recipes(), ids=lambda r: r.row)
def test_each_recipes_scene_picks_its_row(rt, recipe):
    assert _kernel(rt, _load(rt, recipe.scene_name), recipe.flags) == recipe.row


def test_row_hook_bounds(rt):
    lib = rt.amd_lib()
    buf = C.create_string_buffer(160)
    assert lib.rt_test_radiance_kernel_row(2, 0, buf, 160) == RT_ERR_INVALID_ARG
    assert lib.rt_test_radiance_kernel_row(-1, 0, buf, 160) == RT_ERR_INVALID_ARG
    assert lib.rt_test_radiance_kernel_row(0, -1, buf, 160) == RT_ERR_INVALID_ARG
    assert lib.rt_test_radiance_kernel_row(0, len(rt.radiance_rows(0)), buf, 160) == RT_ERR_INVALID_ARG
    assert lib.rt_test_radiance_kernel_row(0, 0, None, 160) == RT_ERR_INVALID_ARG
    assert lib.rt_test_radiance_kernel_row(0, 0, buf, 160) == 0 and buf.value.decode() == rt.radiance_rows(0)[0]
