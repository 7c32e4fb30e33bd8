#!/usr/bin/env python3
"""Ray-query throughput on config 5 at 7680x4320 (GPU box; DESIGN.md §Ray
queries): rt_query_intersect_device over the frame's pixel-centre camera rays

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
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracing-project_amd", "python"))

import rtamd  # noqa: E402
import scenes  # noqa: E402


def camera_rays(sc) -> np.ndarray:
    """Camera::generate_ray (camera.h:44-58) of every pixel, row-major from the
    top row: the rays k_paper_primary generates on the device."""
    cam = sc.desc.camera
    W, H = sc.width, sc.height
    eye, P = np.array(cam.eye[:]), np.array(cam.P[:])
    sx = (np.arange(W, dtype=np.float64) + 0.5) / W
    sy = ((H - 1 - np.arange(H, dtype=np.float64)) + 0.5) / H
    rays = np.empty(W * H, dtype=rtamd.RAY_DTYPE)
    d = rays["d"].reshape(H, W, 3)
    d[:, :, 0] = (P[0] + cam.Lx * sx - eye[0])[None, :]
    d[:, :, 1] = (P[1] + cam.Ly * sy - eye[1])[:, None]
    d[:, :, 2] = P[2] - eye[2]
    d /= np.sqrt((d * d).sum(axis=2, keepdims=True))
    rays["o"] = eye
    rays["tmin"] = 1e-4
    rays["tmax"] = np.inf
    return rays


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
        t0 = time.time()
        rays = camera_rays(sc)
        # the host formula against the oracle's Camera::generate_ray at a few pixels
        if os.path.exists(os.path.join(rtamd.ORACLE_DIR, "liboracle.so")):
            o3, d3 = (C.c_double * 3)(), (C.c_double * 3)()
            for (i, j) in ((0, 0), (W - 1, H - 1), (W // 3, H // 2), (17, H - 5)):
                rtamd.oracle_lib().oracle_camera_ray(sc.desc_ptr, i, j, 0.0, 0.0, 0, o3, d3)
                assert np.allclose(rays["d"][j * W + i], list(d3), rtol=0, atol=1e-14), (i, j)
        d_rays, d_hits, d_mask = rtamd.DeviceBuffer(n * 64), rtamd.DeviceBuffer(n * 64), rtamd.DeviceBuffer(n)
        print(f"{n} camera rays built in {time.time() - t0:.1f} s", flush=True)
        cases = [("coherent", rays)]
        perm = np.random.default_rng(12345).permutation(n)
        cases.append(("shuffled", None))
        for tag, r in cases:
            if r is None:
                r = rays[perm]
            d_rays.from_host(r)
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
            del r
        assert res["coherent"]["hits"] == res["shuffled"]["hits"]
        res["kernel"] = rtamd.query_kernel_name(sc, 0)[1]
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
