#!/usr/bin/env python3
"""The bounce loop against the fused radiance query (GPU box; DESIGN.md
§Bounce loop): rtamd.radiance_bounces_device - per level rt_query_intersect,
rt_rays_wo, rt_query_shade, rt_scatter_rays on device buffers, then
rt_combine_bounce from the last level up - and rt_query_radiance_device on the
same rays, the jittered frame rays of rt_camera_rays_device, for

  cfg5   config 5's scene in standard mode (recursion 6)
  deep   scenes.deep_recursion_scene(6)

per level and in total.  One side runs more launches and moves every level's
rays, hits and colours through HBM; the other diverges per lane inside
k_radiance and keeps its frame stack in scratch.  Which way it falls is a
figure to write down, not a gate.

The loop's time is the device-event time (rt_stats.ms_kernel) of its queries
and scatters PLUS the host wall time of its rt_rays_wo_device and
rt_combine_bounce_device calls, which return no device time: they block until
their kernel is done, so their wall time bounds it from above, and the loop's
total here is an upper bound of its device time.  The fused side is
rt_stats.ms_kernel of rt_query_radiance_device.  The kernels' own times -
k_rays_wo, k_scatter_count / k_scan_tile / k_scatter_emit, k_combine_bounce by
name, and k_camera_rays<false>, the project's yardstick for 64 B record writes,
in the same trace - come from running it under `rocprofv3 --kernel-trace
--stats`; --yardstick adds a centre-ray launch of the same ray count to that
trace.  Bytes of a scatter are NOMINAL: 129 B per parent in each of the two
passes as if every parent were read (a parent whose mask is 0 or whose material
is null is not), + 1 B written, 1 B reread, 8 B of first per parent and 72 B per
child written.  They are not counted on the device.

Usage: python tools/bounce_perf.py [--scene cfg5|deep|both] [--dpi 480] [--reps 3] [--yardstick] [--json PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracing-project_amd", "python"))

import rtamd  # noqa: E402
import scenes  # noqa: E402


def scene_of(tag: str, dpi: int):
    if tag == "cfg5":   # (its own medium.recursion is 6)
        return rtamd.load_scene_from_json_text(scenes.config_json(5, dpi=dpi)[0])
    return rtamd.load_scene_from_json_text(json.dumps(scenes.deep_recursion_scene(6, dpi=dpi)))


def scatter_bytes(n: int, m: int) -> int:
    """Nominal bytes of one rt_scatter_rays_device over n parents with m children (every parent read in full)."""
    return n * (129 + 1) + n * (129 + 1 + 8) + m * 72


def measure(tag: str, dpi, reps: int, yardstick: bool) -> dict:
    sc = scene_of(tag, dpi)
    W, H = sc.width, sc.height
    n = rtamd.RT_SPP * W * H
    d_rays, d_rgb = rtamd.DeviceBuffer(n * 64), rtamd.DeviceBuffer(n * 24)
    st = rtamd.Stats()
    assert rtamd.camera_rays_device(sc, W, H, rtamd.RT_RAYS_JITTERED, None, d_rays, stats=st) == n
    res = {"scene": tag, "W": W, "H": H, "rays": n, "recursion": int(sc.desc.recursion_limit),
           "kernel": rtamd.radiance_kernel_name(sc)[1]}
    fused, fused_wall = [], []
    for k in range(1 + reps):
        t0 = time.perf_counter()
        rtamd.query_radiance_device(sc, d_rays, n, d_rgb, stats=st)
        if k:
            fused.append(st.ms_kernel)
            fused_wall.append((time.perf_counter() - t0) * 1e3)
    res["fused"] = {"ms_kernel": fused, "ms_wall": fused_wall, "rays": [int(st.rays_intersect), int(st.rays_occluded)]}
    want = d_rgb.to_host()[:3 * n]
    runs = []
    for k in range(1 + reps):
        levels = []
        t0 = time.perf_counter()
        d_out, sizes, lst = rtamd.radiance_bounces_device(sc, d_rays, n, per_level=levels)
        wall = (time.perf_counter() - t0) * 1e3
        if k:
            wo = sum(lv["rays_wo"]["ms_total"] for lv in levels if "level" in lv)
            unwind = sum(lv["unwind"]["ms_total"] for lv in levels if "unwind" in lv)
            runs.append({"ms_kernel": lst.ms_kernel, "ms_rays_wo_wall": wo, "ms_combine_wall": unwind,
                         "ms_loop": lst.ms_kernel + wo + unwind, "ms_wall": wall, "levels": levels})
        if k == reps:
            got = d_out.to_host()[:3 * n]
            eq = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
            res["loop_equals_fused"] = bool(eq.all())
            res["loop_rays"] = [int(lst.rays_intersect), int(lst.rays_occluded)]
            res["level_sizes"] = sizes
        d_out.free()
    res["loop"] = runs
    best = min(runs, key=lambda r: r["ms_loop"])
    print(f"{tag} {W}x{H}, {n} rays, levels {res['level_sizes']}")
    print(f"  fused {res['kernel']}: ms_kernel min {min(fused):.3f}  wall min {min(fused_wall):.3f}")
    res["loop_vs_fused"] = best["ms_loop"] / min(fused)
    print(f"  loop: queries' and scatters' ms_kernel {best['ms_kernel']:.3f} + rays_wo calls (wall) "
          f"{best['ms_rays_wo_wall']:.3f} + combine calls (wall) {best['ms_combine_wall']:.3f} = {best['ms_loop']:.3f} ms "
          f"= {res['loop_vs_fused']:.2f}x fused; whole-loop host wall min {min(r['ms_wall'] for r in runs):.3f}; equal bytes "
          f"{res['loop_equals_fused']}, equal counts {res['loop_rays'] == res['fused']['rays']}")
    for lv in best["levels"]:
        if "level" not in lv:
            print(f"    unwind (all levels' rt_combine_bounce_device, host wall): {lv['unwind']['ms_total']:.3f} ms")
            continue
        sb = scatter_bytes(lv["n"], lv["children"])
        sk = lv["scatter"]["ms_kernel"]
        print(f"    level {lv['level']}: {lv['n']:>9} rays  intersect {lv['intersect']['ms_kernel']:.3f}  shade "
              f"{lv['shade']['ms_kernel']:.3f}  scatter {sk:.3f} ms ({lv['children']} children, "
              f"{sb / max(sk, 1e-9) / 1e6:.0f} GB/s of {sb / 1e6:.1f} nominal MB)  rays_wo wall {lv['rays_wo']['ms_total']:.3f}")
    if yardstick:   # k_camera_rays<false> over the same number of 64 B records, for the trace
        n_rows = max(1, n // W)
        d_c = rtamd.DeviceBuffer(n_rows * W * 64)
        cam = rtamd.Camera.from_buffer_copy(sc.desc.camera)
        for _ in range(1 + reps):
            rtamd.camera_rays_device(cam, W, n_rows, rtamd.RT_RAYS_CENTRE, None, d_c, stats=st)
        res["yardstick"] = {"rays": n_rows * W, "ms_kernel": st.ms_kernel,
                            "gb_per_s": n_rows * W * 64 / max(st.ms_kernel, 1e-9) / 1e6}
        print(f"  yardstick k_camera_rays<false>: {n_rows * W} records of 64 B in {st.ms_kernel:.3f} ms = "
              f"{res['yardstick']['gb_per_s']:.0f} GB/s")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="both", choices=["cfg5", "deep", "both"])
    ap.add_argument("--dpi", type=int, default=480, help="the screen's dpi (480: 1920x1080 / 1920x1440, 8 rays a pixel)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--yardstick", action="store_true")
    ap.add_argument("--json", default=None, help="also write the result line to this file")
    a = ap.parse_args()
    out = [measure(t, a.dpi, a.reps, a.yardstick) for t in (("cfg5", "deep") if a.scene == "both" else (a.scene,))]
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
