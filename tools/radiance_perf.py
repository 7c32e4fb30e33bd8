#!/usr/bin/env python3
"""Radiance-query throughput on config 4 at 1920x1080 (GPU box; DESIGN.md
§Radiance queries): rt_query_radiance_device over the standard frame's own
8 W H jittered rays (16.6 M rays, about 1 GB on the device)

  frame     in frame order: output row, pixel, sample (a wave = 8 pixels x 8 samples of a row)
  shuffled  the same rays in a random order (every wave incoherent)

and, as the yardstick, the standard-mode frame of the same scene and size,
which traces exactly those rays with its wave-level culls and generates them
on chip.  The script's figures are device-event times (rt_stats.ms_kernel);
the kernels' own times come from running it under `rocprofv3 --kernel-trace
--stats`, where k_radiance and the frame's kernel appear by name.

Usage: python tools/radiance_perf.py [--dpi 480] [--reps 5] [--frames-only] [--json PATH]
RTAMD_LIB=<another build's librtamd.so> with --frames-only measures that
build's frame (e.g. the parent commit's, for the yardstick)."""
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

def frame_rays(sc, d_rays) -> int:
    """The frame's jittered rays (tracer.cpp:284-293, camera.h:68-78) in frame
    order (output row, x, sample), generated on the device from the frame's own
    resident draws (rt_camera_rays_device; held bit-equal to the oracle by
    tests/test_gpu_camera_rays.py)."""
    st = rtamd.Stats()
    n = rtamd.camera_rays_device(sc, sc.width, sc.height, rtamd.RT_RAYS_JITTERED, None, d_rays, stats=st)
    print(f"{n} frame rays generated on the device: ms_rng {st.ms_rng:.3f} ms_kernel {st.ms_kernel:.3f}", flush=True)
    return n


def frame_times(sc, reps):
    """(ms_kernel of `reps` standard frames after three warm-up frames (the
    first two are the wave-BVH trial, when the scene has one), last stats)."""
    lib = rtamd.amd_lib()
    W, H = sc.width, sc.height
    rows = (C.c_int32 * H)(*range(H))
    buf = rtamd.DeviceBuffer(H * W * 3 * 8)
    st = rtamd.Stats()
    out = []
    for k in range(3 + reps):
        rc = lib.rt_render_rows_device(sc.handle, W, H, rtamd.RT_MODE_STANDARD, 0, rows, H, buf.ptr, None, C.byref(st))
        assert rc == 0, rtamd.last_error()
        if k >= 3:
            out.append(st.ms_kernel)
    fb = buf.to_host(np.float64, (H, W, 3))
    buf.free()
    return out, st, fb


def summary(ms):
    return {"min": min(ms), "median": float(np.median(ms)), "max": max(ms), "all": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dpi", type=int, default=480, help="config 4's dpi (480: 1920x1080)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames-only", action="store_true", help="only the standard-mode frame (the yardstick)")
    ap.add_argument("--json", default=None, help="also write the result line to this file")
    a = ap.parse_args()
    text, _ = scenes.config_json(4, dpi=a.dpi)
    sc = rtamd.load_scene_from_json_text(text)
    W, H = sc.width, sc.height
    n = 8 * W * H
    res = {"scene": "config 4", "W": W, "H": H, "rays": n,
           "lib": "RTAMD_LIB" if os.environ.get("RTAMD_LIB") else "lib/librtamd.so",
           "frame_kernel": rtamd.kernel_name(sc, 0)[1]}
    ft, fst, fb = frame_times(sc, a.reps)
    res["frame_ms_kernel"] = summary(ft)
    res["frame_rays"] = [int(fst.rays_intersect), int(fst.rays_occluded)]
    print(f"standard frame {W}x{H} ({res['frame_kernel']}): ms_kernel min {min(ft):.3f} median {np.median(ft):.3f} "
          f"max {max(ft):.3f}", flush=True)
    if not a.frames_only:
        d_rays, d_rgb = rtamd.DeviceBuffer(n * 64), rtamd.DeviceBuffer(n * 24)
        assert frame_rays(sc, d_rays) == n
        res["kernel"] = rtamd.radiance_kernel_name(sc)[1]
        perm = np.random.default_rng(12345).permutation(n)
        for tag in ("frame", "shuffled"):
            if tag == "shuffled":   # (one round trip to permute the device's rays)
                d_rays.from_host(d_rays.to_host(np.uint8).view(rtamd.RAY_DTYPE)[perm])
            st = rtamd.Stats()
            qt = []
            for k in range(1 + a.reps):
                rtamd.query_radiance_device(sc, d_rays, n, d_rgb, stats=st)
                if k >= 1:
                    qt.append(st.ms_kernel)
            res[tag] = {"ms_kernel": summary(qt), "mrays_per_s": n / min(qt) / 1e3,
                        "rays": [int(st.rays_intersect), int(st.rays_occluded)],
                        "vs_frame_median": float(np.median(qt)) / float(np.median(ft))}
            print(f"query_radiance {tag:9s}: ms_kernel min {min(qt):.3f} median {np.median(qt):.3f} max {max(qt):.3f}  "
                  f"{n / min(qt) / 1e3:.0f} Mrays/s  {res[tag]['vs_frame_median']:.2f}x the frame", flush=True)
            # the frame's own rays: its ray counts (reported, not asserted), and
            # (frame order) its pixels
            res[tag]["rays_equal_frame"] = res[tag]["rays"] == res["frame_rays"]
            if tag == "frame":
                rgb = d_rgb.to_host(np.float64, (H, W, 8, 3))
                acc = np.zeros((H, W, 3))
                for s in range(8):
                    acc += rgb[:, :, s]
                res["max_abs_diff_to_frame"] = float(np.abs(acc * 0.125 - fb).max())
                print(f"  per-pixel means against the frame: max|d| = {res['max_abs_diff_to_frame']:.3g}", flush=True)
                del rgb, acc
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
