"""GPU: the lean standard kernel with its arguments read again from the
kernarg segment (scene_again / std_again, rt_device.hpp and rt_kernels.hpp).

The shading loops, the primary wave query and the kernel's tail no longer use
the kernel's DevScene / StdParams copies but re-read the fields where they use
them, at an offset of the kernarg segment.  What can go wrong is an address:
a field read at the wrong offset, a table pointer, a count, the framebuffer,
the row list or the counter block.  So the benchmark's scene (snorlax with
config 4's five lights and recursion limit) is rendered on frames whose width
and height are no multiple of a wave's 2x4-pixel tile - partial waves at the
right and bottom edges, a single row of workgroups, one workgroup column - with
culling on, with RT_FLAG_NO_CULL and with RT_FLAG_COUNT_OPS (the counter
flush), as row subsets (rows / jrow / fb), and with 6 and 33 lights (the last
light past the LDS light cache; a second round of 32 lights)."""
import ctypes as C
import functools
import json

import numpy as np
import pytest

import scenes

TOL = 1e-5   # the suite's channel tolerance against the oracle (tests/test_gpu_parity.py)
# width, height, dpi: the screen stays about 4 units wide around config 4's centre
FRAMES = [(13, 7, 3), (37, 29, 9), (130, 3, 32)]
# the op counters the standard kernels share one for one with the reference when
# culling is off (tests/test_gpu_parity.py: Pokeball regions and eager programs
# are resolved lazily, so their two counters differ by design)
FLOP_COUNTERS = ["sphere_isect", "sphere_isect_hit", "sphere_ivl", "sphere_ivl_hit", "half_isect", "half_isect_hit",
                 "half_ivl", "xform", "shade_light", "shade_spec", "secondary", "light_eval", "shade_call"]


def _text(W, H, dpi):
    return json.dumps(scenes.with_size(scenes.cfg4_scene(), W, H, dpi))


@functools.lru_cache(maxsize=None)
def _oracle(W, H, dpi):
    """(frame, rays_intersect, rays_occluded, op counts) of the CPU oracle, once per frame size."""
    import rtamd as rt

    sc = rt.load_scene_from_json_text(_text(W, H, dpi))
    assert (sc.width, sc.height) == (W, H)
    fb, st = rt.oracle_render(sc, W, H, 0, threads=8)
    fb.setflags(write=False)
    return fb, int(st.rays_intersect), int(st.rays_occluded), {n: int(st.ops[i]) for i, n in enumerate(rt.OP_NAMES)}


def _render(rt, sc, flags=0):
    st = rt.Stats()
    fb = rt.Tracer(sc, sc.width, sc.height, 0, flags=flags).render(st)
    return fb, st


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,dpi", FRAMES)
def test_odd_frames_match_oracle(gpu, W, H, dpi):
    rt = gpu
    sc = rt.load_scene_from_json_text(_text(W, H, dpi))
    assert (sc.width, sc.height) == (W, H)
    # the kernels under test: the benchmark's, its per-lane-cull and its op-counting builds
    assert rt.kernel_name(sc, 0) == (0, "rtd::k_std_lean<false, 1, false>")
    assert rt.kernel_name(sc, 0, rt.RT_FLAG_NO_CULL) == (0, "rtd::k_std_lean<false, 0, false>")
    assert rt.kernel_name(sc, 0, rt.RT_FLAG_COUNT_OPS) == (0, "rtd::k_std_lean<true, 1, false>")
    ref, ri, ro, ops = _oracle(W, H, dpi)
    cull, st = _render(rt, sc)
    err = float(np.abs(cull - ref).max())
    print(f"{W}x{H}: max|d| vs oracle {err:.3g}, rays ({st.rays_intersect}, {st.rays_occluded}) oracle ({ri}, {ro})")
    assert err <= TOL
    assert (st.rays_intersect, st.rays_occluded) == (ri, ro)
    plain, st1 = _render(rt, sc, rt.RT_FLAG_NO_CULL)
    assert np.array_equal(cull, plain)
    assert (st1.rays_intersect, st1.rays_occluded) == (ri, ro)
    # the counter flush: culling on (same image, same rays), then off (the oracle's op counts)
    cnt, st2 = _render(rt, sc, rt.RT_FLAG_COUNT_OPS)
    assert np.array_equal(cnt, cull)
    assert (st2.rays_intersect, st2.rays_occluded) == (ri, ro)
    cnt0, st3 = _render(rt, sc, rt.RT_FLAG_COUNT_OPS | rt.RT_FLAG_NO_CULL)
    assert np.array_equal(cnt0, cull)
    assert (st3.rays_intersect, st3.rays_occluded) == (ri, ro)
    got = {n: int(st3.ops[i]) for i, n in enumerate(rt.OP_NAMES)}
    assert {n: got[n] for n in FLOP_COUNTERS} == {n: ops[n] for n in FLOP_COUNTERS}


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, 1], ids=["timed", "count_ops"])
def test_row_subsets_match_full_frame(gpu, flags):
    """Every 3rd group of 8 rows of the 37x29 frame (the strips a rank of three
    renders; the last group has 5 rows), bit for bit the full frame's rows,
    and the three strips' ray counts add up to the frame's."""
    rt = gpu
    W, H, dpi = FRAMES[1]
    sc = rt.load_scene_from_json_text(_text(W, H, dpi))
    full, st = _render(rt, sc, flags)
    lib = rt.amd_lib()
    rays = [0, 0]
    for rank in range(3):
        rows = [r for g in range((H + 7) // 8) if g % 3 == rank for r in range(g * 8, min(H, g * 8 + 8))]
        buf = rt.DeviceBuffer(len(rows) * W * 3 * 8)
        s1 = rt.Stats()
        rc = lib.rt_render_rows_device(sc.handle, W, H, 0, flags, (C.c_int32 * len(rows))(*rows), len(rows),
                                       buf.ptr, None, C.byref(s1))
        assert rc == 0, rt.last_error()
        assert np.array_equal(buf.to_host(np.float64, (len(rows), W, 3)), full[rows]), rank
        rays[0] += s1.rays_intersect
        rays[1] += s1.rays_occluded
    assert tuple(rays) == (st.rays_intersect, st.rays_occluded)


def _lights(n):
    """n point lights on a ring above and in front of the model, some behind it."""
    out = []
    for k in range(n):
        a = 2.0 * np.pi * k / n
        out.append(((6.0 * np.cos(a), 3.0 + 0.25 * (k % 5), 2.0 + 6.0 * np.sin(a)), (3.0 + (k % 3), 3.0, 4.0 - (k % 2))))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", [6, 33])
def test_light_counts_match_oracle(gpu, n):
    """6 lights: one past the five the LDS light cache holds; 33: a second
    round of the two light passes with one light in it."""
    rt = gpu
    W, H, dpi = FRAMES[1]
    sc = rt.with_point_lights(rt.load_scene_from_json_text(_text(W, H, dpi)), _lights(n))
    assert rt.kernel_name(sc, 0) == (0, "rtd::k_std_lean<false, 1, false>")
    ref, ost = rt.oracle_render(sc, W, H, 0, threads=8)
    fb, st = _render(rt, sc)
    err = float(np.abs(fb - ref).max())
    print(f"{n} lights: max|d| vs oracle {err:.3g}, rays ({st.rays_intersect}, {st.rays_occluded})")
    assert err <= TOL
    assert (st.rays_intersect, st.rays_occluded) == (ost.rays_intersect, ost.rays_occluded)
    assert st.rays_occluded > 0
    plain, _ = _render(rt, sc, rt.RT_FLAG_NO_CULL)
    assert np.array_equal(fb, plain)
