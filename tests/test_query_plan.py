"""The kernel a ray query launches (frame_plan.cpp pick_query_variant + the
query table of rt_query_kernels.hpp), through rt_test_query_kernel_name: host
logic only, no device is touched.  A query takes pick_variant's stack tiers
and its eager / deep / plain rules, always with per-lane culls; the results of
those kernels are checked against the oracle by tests/test_gpu_query.py."""
import ctypes as C
import json

import pytest

import scenes

ISECT, OCCL = 0, 1
RT_ERR_INVALID_ARG, RT_ERR_UNSUPPORTED = -1, -6


def _args(name):
    return [a.strip() for a in name.split("<", 1)[1].rsplit(">", 1)[0].split(",")]


def _query_kernel(rt, sc, kind, flags=0):
    rc, name = rt.query_kernel_name(sc, kind, flags)
    assert rc == 0, rt.last_error()
    return name


def _frame_kernel(rt, sc, mode, flags=0):
    buf = C.create_string_buffer(160)
    assert rt.amd_lib().rt_test_kernel_name(sc.handle, mode, flags, buf, 160) == 0
    return buf.value.decode()


def _both(rt, sc, flags=0):
    """The two kinds' kernels: different kernels of the same variant."""
    i, o = _query_kernel(rt, sc, ISECT, flags), _query_kernel(rt, sc, OCCL, flags)
    assert i != o
    assert "::k_query_isect<" in i and "::k_query_occl<" in o
    assert i.split("::")[0] == o.split("::")[0] and _args(i) == _args(o)
    return i, o


def test_config3_takes_the_plain_kernels(rt):
    sc = rt.load_scene_from_json_text(scenes.config_json(3, dpi=24)[0])
    i, o = _both(rt, sc)
    assert i == "rtd::k_query_isect<false, false, true>" and o == "rtd::k_query_occl<false, false, true>"
    # RT_FLAG_NO_CULL changes the scene argument, not the kernel
    assert _both(rt, sc, rt.RT_FLAG_NO_CULL) == (i, o)


def test_config5_takes_the_plain_kernels(rt):
    sc = rt.load_scene_from_json_text(scenes.config_json(5, dpi=24)[0])
    assert _args(_both(rt, sc)[0]) == ["false", "false", "true"]


def test_config4_takes_a_csg_kernel(rt):
    sc = rt.load_scene_from_json_text(scenes.config_json(4, dpi=24)[0])
    i, _ = _both(rt, sc)
    assert i.startswith("rtd::") and _args(i)[2] == "false", i   # not plain
    assert _args(i)[0] == "false", i                             # no eager programs in snorlax


@pytest.mark.parametrize("name", sorted(scenes.deep_scenes()))
def test_deep_scenes_take_their_stack_tier(rt, name):
    """A query needs no reflection / refraction frames: mirrors_rec24, whose
    frames run on the big stacks for their recursion alone, is queried on the
    common kernels; the transform and CSG depths keep their frames' namespace."""
    sc = rt.load_scene_from_json_text(json.dumps(scenes.deep_scenes()[name]))
    i, _ = _both(rt, sc)
    frame_ns = _frame_kernel(rt, sc, 0).split("::")[0]
    assert frame_ns == "rtdb"
    if name == "mirrors_rec24":
        assert i == "rtd::k_query_isect<false, false, true>"
    else:
        assert i == f"{frame_ns}::k_query_isect<true, true, false>"


def test_xform_nest12_takes_its_frames_namespace(rt):
    sc = rt.load_scene_from_json_text(json.dumps(scenes.deep_scenes()["xform_nest12"]))
    for mode in (0, 1):
        assert _query_kernel(rt, sc, ISECT).split("::")[0] == _frame_kernel(rt, sc, mode).split("::")[0]


@pytest.mark.parametrize("case", sorted(scenes.dir_light_cases()))
def test_directional_lights_take_the_deep_variant(rt, case):
    text, lights = scenes.dir_light_cases()[case]
    base = rt.load_scene_from_json_text(text)
    sc = rt.with_dir_lights(base, lights)
    i, _ = _both(rt, sc)
    assert _args(i)[1] == "true" and _args(i)[2] == "false", i
    if case.startswith("cfg2"):   # the same scene without them is plain
        assert _args(_both(rt, base)[0]) == ["false", "false", "true"]


@pytest.mark.parametrize("which", sorted(scenes.torture_scenes()))
def test_torture_scenes_have_a_query_kernel(rt, which):
    sc = rt.load_scene_from_json_text(json.dumps(scenes.torture_scenes(dpi=12)[which]))
    i, _ = _both(rt, sc)
    e, d, pl = _args(i)
    assert pl == "false", i                        # every one holds a transform or CSG object
    assert not (e == "true" and d == "false"), i   # eager scenes always use D


@pytest.mark.parametrize("kind", [ISECT, OCCL])
def test_refused_flags(rt, kind):
    sc = rt.load_scene_from_json_text(scenes.config_json(3, dpi=24)[0])
    rc, _ = rt.query_kernel_name(sc, kind, rt.RT_FLAG_FP32)
    assert rc == RT_ERR_UNSUPPORTED and "FP32" in rt.last_error()
    rc, _ = rt.query_kernel_name(sc, kind, rt.RT_FLAG_COUNT_OPS)
    assert rc == RT_ERR_UNSUPPORTED and "COUNT_OPS" in rt.last_error()


def test_bad_kind_and_null(rt):
    sc = rt.load_scene_from_json_text(scenes.config_json(3, dpi=24)[0])
    assert rt.query_kernel_name(sc, 2)[0] == RT_ERR_INVALID_ARG
    buf = C.create_string_buffer(16)
    assert rt.amd_lib().rt_test_query_kernel_name(None, 0, 0, buf, 16) == RT_ERR_INVALID_ARG


def test_scene_beyond_the_big_stacks_is_refused_like_its_frames(rt):
    leaves = [{"sphere": {"position": [0.01 * i, 0, -2], "radius": 0.5, "color": {"diffuse": [1, 1, 1]}}}
              for i in range(80)]
    node = leaves[-1]
    for leaf in reversed(leaves[:-1]):
        node = {"csg": {"operator": "union", "left": leaf, "right": node}}
    sc = rt.load_scene_from_json_text(json.dumps({"screen": {"dpi": 4, "dimensions": [2, 2], "position": [-1, -1, 0],
                                                             "observer": [0, 0, 3]}, "objects": [node]}))
    buf = C.create_string_buffer(160)
    assert rt.amd_lib().rt_test_kernel_name(sc.handle, 0, 0, buf, 160) == RT_ERR_UNSUPPORTED
    rc, _ = rt.query_kernel_name(sc, ISECT)
    assert rc == RT_ERR_UNSUPPORTED and "CSG operand depth 80" in rt.last_error()


def test_ray_and_hit_records_are_64_bytes(rt):
    assert C.sizeof(rt.Ray) == C.sizeof(rt.Hit) == 64
    assert rt.RAY_DTYPE.itemsize == rt.HIT_DTYPE.itemsize == 64
    assert C.sizeof(rt.Hit) == C.sizeof(rt.OracleHit)
    assert [(n, getattr(rt.Hit, n).offset) for n, _ in rt.Hit._fields_] == \
           [(n, getattr(rt.OracleHit, n).offset) for n, _ in rt.OracleHit._fields_]
    rays = rt.make_rays([[0, 0, 5], [1, 2, 3]], [[0, 0, -1], [0, 0, -2]], tmax=[1.0, 2.0])
    assert rays["tmin"].tolist() == [1e-4, 1e-4] and rays["tmax"].tolist() == [1.0, 2.0]
    with pytest.raises(ValueError):
        rt.make_rays([[0, 0, 5]], [[0, 0, -1], [0, 0, -2]])
