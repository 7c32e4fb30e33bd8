#!/usr/bin/env python3
"""Ray-query throughput on config 5 at 7680x4320 (GPU box; DESIGN.md §Ray
queries): rt_query_intersect_device over the frame's pixel-centre camera rays
(generated on the device by rt_camera_rays_device)

  coherent   in row-major pixel order (a wave = 64 consecutive pixels of a row)
  shuffled   the same rays in a random order (every wave incoherent)

and, as the yardstick, the paper-mode frame of the same scene and size, whose
k_paper_primary* kernel traces exactly those rays and also shades them.  The
script's own figures are device-event times (rt_stats.ms_kernel: for the frame
that is primary + finish pass); the primary kernel alone comes from running
the script under `rocprofv3 --kernel-trace --stats`, where the query kernels
(k_query_isect / k_query_occl) and k_paper_primary* appear by name.

Usage: python tools/query_perf.py [--dpi 1920] [--reps 5] [--frames-only] [--occluded] [--json PATH]
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


def camera_rays(sc, d_rays) -> int:
    """Camera::generate_ray (camera.h:44-58) of every pixel, row-major from the
    top row, generated on the device (rt_camera_rays_device; held bit-equal to
    the oracle by tests/test_gpu_camera_rays.py): the rays k_paper_primary
    generates itself."""
    st = rtamd.Stats()
    n = rtamd.camera_rays_device(sc, sc.width, sc.height, rtamd.RT_RAYS_CENTRE, None, d_rays, stats=st)
    print(f"{n} camera rays generated on the device: ms_kernel {st.ms_kernel:.3f}", flush=True)
    return n


def frame_times(sc, reps):
    """ms_kernel of `reps` paper-mode frames after two warm-up frames (the first
    is the timed launch whose wave times order the later ones)."""
    lib = rtamd.amd_lib()
    W, H = sc.width, sc.height
    rows = (C.c_int32 * H)(*range(H))
    buf = rtamd.DeviceBuffer(H * W * 3 * 8)
    st = rtamd.Stats()
    out = []
    for k in range(2 + reps):
        rc = lib.rt_render_rows_device(sc.handle, W, H, rtamd.RT_MODE_PAPER, 0, rows, H, buf.ptr, None, C.byref(st))
        assert rc == 0, rtamd.last_error()
        if k >= 2:
            out.append(st.ms_kernel)
    buf.free()
    return out


def query_times(sc, d_rays, n, d_hits, d_mask, reps, occluded):
    lib = rtamd.amd_lib()
    st = rtamd.Stats()
    out = []
    for k in range(1 + reps):
        if occluded:
            rc = lib.rt_query_occluded_device(sc.handle, d_rays.ptr, n, 0, d_mask.ptr, None, C.byref(st))
        else:
            rc = lib.rt_query_intersect_device(sc.handle, d_rays.ptr, n, 0, d_hits.ptr, d_mask.ptr, None, C.byref(st))
        assert rc == 0, rtamd.last_error()
        if k >= 1:
            out.append(st.ms_kernel)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dpi", type=int, default=1920, help="config 5's dpi (1920: 7680x4320)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames-only", action="store_true", help="only the paper-mode frame (the yardstick)")
    ap.add_argument("--occluded", action="store_true", help="also time rt_query_occluded_device on the same rays")
    ap.add_argument("--json", default=None, help="also write the result line to this file")
    a = ap.parse_args()
    text, _ = scenes.config_json(5, dpi=a.dpi)
    sc = rtamd.load_scene_from_json_text(text)
    W, H = sc.width, sc.height
    n = W * H
    res = {"scene": "config 5", "W": W, "H": H, "rays": n,
           "lib": "RTAMD_LIB" if os.environ.get("RTAMD_LIB") else "lib/librtamd.so"}

    def rate(ms):
        return n / ms / 1e3   # Mrays/s

    ft = frame_times(sc, a.reps)
    res["frame_ms_kernel"] = {"min": min(ft), "median": float(np.median(ft)), "all": ft}
    print(f"paper frame {W}x{H} (k_paper_primary* + k_paper_finish): ms_kernel min {min(ft):.3f} median "
          f"{np.median(ft):.3f}", flush=True)
    if not a.frames_only:
        d_rays, d_hits, d_mask = rtamd.DeviceBuffer(n * 64), rtamd.DeviceBuffer(n * 64), rtamd.DeviceBuffer(n)
        assert camera_rays(sc, d_rays) == n
        # coherent: the device's rays as they are; shuffled: one round trip to permute them
        perm = np.random.default_rng(12345).permutation(n)
        cases = [("coherent", None), ("shuffled", perm)]
        for tag, r in cases:
            if r is not None:
                d_rays.from_host(d_rays.to_host(np.uint8).view(rtamd.RAY_DTYPE)[r])
            qt = query_times(sc, d_rays, n, d_hits, d_mask, a.reps, False)
            hit = int(d_mask.to_host(np.uint8).sum())
            res[tag] = {"ms_kernel": {"min": min(qt), "median": float(np.median(qt)), "all": qt},
                        "mrays_per_s": rate(min(qt)), "hits": hit}
            print(f"query_intersect {tag:9s}: ms_kernel min {min(qt):.3f} median {np.median(qt):.3f}  "
                  f"{rate(min(qt)):.0f} Mrays/s  hits {hit}", flush=True)
            if a.occluded:
                ot = query_times(sc, d_rays, n, d_hits, d_mask, a.reps, True)
                res[tag]["occluded_ms_kernel"] = {"min": min(ot), "median": float(np.median(ot)), "all": ot}
                print(f"query_occluded  {tag:9s}: ms_kernel min {min(ot):.3f}  {rate(min(ot)):.0f} Mrays/s", flush=True)
        assert res["coherent"]["hits"] == res["shuffled"]["hits"]
        res["kernel"] = rtamd.query_kernel_name(sc, 0)[1]
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
