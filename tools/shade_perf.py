#!/usr/bin/env python3
"""Shading-query throughput on config 4's pixel-centre rays at 3840x2160
(8.3 M rays; GPU box; DESIGN.md §Shade queries): the deferred pipeline on
device buffers

  intersect  rt_query_intersect_device of the rays
  shade      rt_query_shade_device on its (hits, mask) output in place, wo = -d

and, as the yardstick, rt_query_radiance_device of the same rays on a
recursion-limit-1 copy of the scene: existing code that does the closest hit
plus the same shading in one kernel.  Shading alone does strictly less work
than the yardstick.  The figures are device-event times (rt_stats.ms_kernel).

Usage: python tools/shade_perf.py [--dpi 960] [--reps 5] [--json PATH]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracing-project_amd", "python"))

import rtamd  # noqa: E402
import scenes  # noqa: E402


def summary(ms):
    return {"min": min(ms), "median": float(np.median(ms)), "max": max(ms), "all": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dpi", type=int, default=960, help="config 4's dpi (960: 3840x2160)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None, help="also write the result line to this file")
    a = ap.parse_args()
    lib = rtamd.amd_lib()
    sc = rtamd.load_scene_from_json_text(scenes.config_json(4, dpi=a.dpi)[0])
    rec1 = rtamd.with_recursion_limit(sc, 1)
    W, H = sc.width, sc.height
    n = W * H
    res = {"scene": "config 4", "W": W, "H": H, "rays": n, "kernels": {
        "intersect": rtamd.query_kernel_name(sc, 0)[1], "shade": rtamd.shade_kernel_name(sc)[1],
        "radiance": rtamd.radiance_kernel_name(rec1)[1]}}
    d_rays, d_hits, d_mask = rtamd.DeviceBuffer(n * 64), rtamd.DeviceBuffer(n * 64), rtamd.DeviceBuffer(n)
    d_wo, d_rgb, d_rad = rtamd.DeviceBuffer(n * 24), rtamd.DeviceBuffer(n * 24), rtamd.DeviceBuffer(n * 24)
    # the pixel-centre camera rays (Camera::generate_ray, camera.h) in frame order and
    # their wo = (-d).normalized(), both generated on the device
    assert rtamd.camera_rays_device(sc, W, H, rtamd.RT_RAYS_CENTRE, None, d_rays) == n
    rtamd.rays_wo_device(d_rays, n, d_wo)
    st = rtamd.Stats()
    ti, ts, tr = [], [], []
    for k in range(1 + a.reps):   # (one warm-up round)
        rc = lib.rt_query_intersect_device(sc.handle, d_rays.ptr, n, 0, d_hits.ptr, d_mask.ptr, None, C.byref(st))
        assert rc == 0, rtamd.last_error()
        if k:
            ti.append(st.ms_kernel)
        rtamd.query_shade_device(sc, d_hits, d_wo, d_mask, n, d_rgb, stats=st)
        if k:
            ts.append(st.ms_kernel)
    res["hits"] = int(d_mask.to_host(np.uint8).sum())
    res["shade_occluded"] = int(st.rays_occluded)
    for k in range(1 + a.reps):
        rtamd.query_radiance_device(rec1, d_rays, n, d_rad, stats=st)
        if k:
            tr.append(st.ms_kernel)
    res["radiance_rays"] = [int(st.rays_intersect), int(st.rays_occluded)]
    res["max_abs_diff_shade_to_radiance"] = float(np.abs(d_rgb.to_host() - d_rad.to_host()).max())
    for tag, t in (("intersect", ti), ("shade", ts), ("radiance_rec1", tr)):
        res[tag + "_ms_kernel"] = summary(t)
        print(f"{tag:14s}: ms_kernel min {min(t):.3f} median {np.median(t):.3f} max {max(t):.3f}  "
              f"{n / min(t) / 1e3:.0f} M entries/s", flush=True)
    res["shade_vs_radiance_median"] = float(np.median(ts)) / float(np.median(tr))
    res["pipeline_vs_radiance_median"] = (float(np.median(ti)) + float(np.median(ts))) / float(np.median(tr))
    print(f"{res['hits']} of {n} rays hit; shade {res['shade_occluded']} occluded calls, radiance "
          f"{res['radiance_rays'][1]}; max|shade - radiance| = {res['max_abs_diff_shade_to_radiance']:.3g}; shade is "
          f"{res['shade_vs_radiance_median']:.2f}x the radiance query, intersect + shade "
          f"{res['pipeline_vs_radiance_median']:.2f}x")
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
