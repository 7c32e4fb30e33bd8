#!/usr/bin/env python3
"""Camera-ray and composed-frame measurements on config 4 at 3840x2160 (GPU
box; DESIGN.md §Camera rays and sample resolve).

  kernels   k_camera_rays<false> over the whole frame (8.3 M rays, 531 MB
            written) and k_camera_rays<true> over 270 of its rows (the same
            ray count, plus 133 MB of draws read), with the jitter cache off so
            that every jittered call also runs the jitter-fill kernel
            (k_mt_fill_w, 133 MB written: the write-bound yardstick).  The
            script prints device-event times; run it under `rocprofv3
            --kernel-trace --stats` for the kernels' own times by name.
  pipeline  the frame composed on the device in row chunks of 270 (rays ->
            radiance -> resolve, every buffer on the device), beside rt_render's
            frame and beside the same composition fed from host rays (64 B per
            ray up, 24 B per ray back, averaged on the host), in one process.

Usage: python tools/camera_perf.py [--dpi 960] [--reps 5] [--chunk-rows 270] [--what kernels,pipeline] [--json PATH]
RTAMD_LIB=<another build's librtamd.so> measures that build's kernels."""
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


def summary(ms):
    return {"min": min(ms), "median": float(np.median(ms)), "max": max(ms), "all": ms}


def kernels(sc, W, H, chunk_rows, reps, res):
    n = W * H
    rows = list(range(chunk_rows))
    assert chunk_rows * 8 == H, "the jittered rows must give the whole frame's ray count"
    d_rays = rtamd.DeviceBuffer(n * 64)
    st = rtamd.Stats()
    tc, tj, tr = [], [], []
    for k in range(1 + reps):
        assert rtamd.camera_rays_device(sc, W, H, rtamd.RT_RAYS_CENTRE, None, d_rays, stats=st) == n
        if k:
            tc.append(st.ms_kernel)
    try:
        rtamd.jitter_cache_budget(0)   # every call generates its draws: the fill kernel runs each time
        for k in range(1 + reps):
            assert rtamd.camera_rays_device(sc, W, H, rtamd.RT_RAYS_JITTERED, rows, d_rays, stats=st) == n
            if k:
                tj.append(st.ms_kernel)
                tr.append(st.ms_rng)
    finally:
        rtamd.jitter_cache_budget(-1)
    d_rays.free()
    draws = chunk_rows * W * 16 * 8
    res["kernels"] = {
        "rays": n,
        "centre": {"ms_kernel": summary(tc), "bytes_written": n * 64, "gb_per_s": n * 64 / min(tc) / 1e6},
        "jittered": {"ms_kernel": summary(tj), "bytes_written": n * 64, "bytes_read": draws,
                     "gb_per_s": (n * 64 + draws) / min(tj) / 1e6},
        "jitter_fill": {"ms_rng": summary(tr), "bytes_written": draws, "gb_per_s": draws / min(tr) / 1e6},
    }
    for tag, v in res["kernels"].items():
        if tag != "rays":
            t = v.get("ms_kernel") or v["ms_rng"]
            print(f"{tag:12s}: min {t['min']:.4f} median {t['median']:.4f} ms  {v['gb_per_s']:.0f} GB/s", flush=True)


def pipeline(sc, W, H, chunk_rows, reps, res):
    lib = rtamd.amd_lib()
    all_rows = (C.c_int32 * H)(*range(H))
    d_fb = rtamd.DeviceBuffer(H * W * 24)
    st = rtamd.Stats()
    # rt_render's frame (three warm-up frames: the wave-BVH trial, when the scene has one)
    tf, tfw = [], []
    for k in range(3 + reps):
        t0 = time.perf_counter()
        rc = lib.rt_render_rows_device(sc.handle, W, H, 0, 0, all_rows, H, d_fb.ptr, None, C.byref(st))
        assert rc == 0, rtamd.last_error()
        if k >= 3:
            tf.append(st.ms_kernel)
            tfw.append((time.perf_counter() - t0) * 1e3)
    frame = d_fb.to_host(shape=(H, W, 3))
    frame_rays = (int(st.rays_intersect), int(st.rays_occluded))
    # the frame composed on the device, rows in chunks (the ray buffer is chunk_rows * W * 8 * 64 B)
    nc = chunk_rows * W * 8
    d_rays, d_rgb = rtamd.DeviceBuffer(nc * 64), rtamd.DeviceBuffer(nc * 24)
    chunks = [list(range(r0, min(H, r0 + chunk_rows))) for r0 in range(0, H, chunk_rows)]
    split, wall = [], []
    for k in range(1 + reps):
        ms = {"rays": 0.0, "rng": 0.0, "radiance": 0.0, "resolve_wall": 0.0}
        counts = [0, 0]
        t0 = time.perf_counter()
        for rows in chunks:
            n = rtamd.camera_rays_device(sc, W, H, rtamd.RT_RAYS_JITTERED, rows, d_rays, stats=st)
            ms["rays"] += st.ms_kernel
            ms["rng"] += st.ms_rng
            rtamd.query_radiance_device(sc, d_rays, n, d_rgb, stats=st)
            ms["radiance"] += st.ms_kernel
            counts[0] += int(st.rays_intersect)
            counts[1] += int(st.rays_occluded)
            t1 = time.perf_counter()
            rc = lib.rt_resolve_samples_device(d_rgb.ptr, len(rows) * W, 8, C.c_void_p(d_fb.ptr.value + rows[0] * W * 24),
                                               None)
            assert rc == 0, rtamd.last_error()
            ms["resolve_wall"] += (time.perf_counter() - t1) * 1e3
        if k:
            wall.append((time.perf_counter() - t0) * 1e3)
            split.append(ms)
    composed = d_fb.to_host(shape=(H, W, 3))
    res["pipeline"] = {
        "chunk_rows": chunk_rows, "chunks": len(chunks),
        "frame": {"ms_kernel": summary(tf), "wall_ms": summary(tfw), "rays": frame_rays},
        "device_composed": {"wall_ms": summary(wall), "rays": counts,
                            "split_ms_median": {key: float(np.median([s[key] for s in split])) for key in split[0]},
                            "max_abs_diff_to_frame": float(np.abs(composed - frame).max())},
    }
    p = res["pipeline"]
    print(f"rt_render frame      : ms_kernel median {p['frame']['ms_kernel']['median']:.3f}, wall {p['frame']['wall_ms']['median']:.3f}")
    print(f"composed on device   : wall median {p['device_composed']['wall_ms']['median']:.3f} ms, split "
          f"{p['device_composed']['split_ms_median']}, max|d| to the frame {p['device_composed']['max_abs_diff_to_frame']:.3g}, "
          f"rays equal the frame's: {tuple(counts) == frame_rays}", flush=True)
    # the same composition fed from host rays: upload 64 B per ray, read 24 B back, average on the host
    host_wall = []
    out = np.zeros((H, W, 3))
    for k in range(2):
        t_all = 0.0
        for rows in chunks:
            rays = rtamd.camera_rays(sc, W, H, rtamd.RT_RAYS_JITTERED, rows=rows).reshape(-1)   # (not timed: today built on the host)
            rgb = np.zeros((len(rays), 3))
            t0 = time.perf_counter()
            rc = lib.rt_query_radiance(sc.handle, rays.ctypes.data_as(C.c_void_p), len(rays), 0,
                                       rgb.ctypes.data_as(C.c_void_p), None)
            assert rc == 0, rtamd.last_error()
            out[rows[0]:rows[0] + len(rows)] = rtamd.resolve_samples(rgb.reshape(len(rows), W, 8, 3), 8)
            t_all += (time.perf_counter() - t0) * 1e3
            del rays, rgb
        host_wall.append(t_all)
    p["host_fed"] = {"wall_ms": summary(host_wall), "max_abs_diff_to_frame": float(np.abs(out - frame).max()),
                     "equals_device_composed": bool(out.tobytes() == composed.tobytes())}
    print(f"fed from host rays   : wall min {min(host_wall):.1f} ms (query + host resolve; building the rays not counted), "
          f"equal to the device-composed frame: {p['host_fed']['equals_device_composed']}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dpi", type=int, default=960, help="config 4's dpi (960: 3840x2160)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk-rows", type=int, default=270)
    ap.add_argument("--what", default="kernels,pipeline")
    ap.add_argument("--json", default=None, help="also write the result line to this file")
    a = ap.parse_args()
    sc = rtamd.load_scene_from_json_text(scenes.config_json(4, dpi=a.dpi)[0])
    W, H = sc.width, sc.height
    res = {"scene": "config 4", "W": W, "H": H,
           "lib": os.environ.get("RTAMD_LIB") or "lib/librtamd.so"}
    what = a.what.split(",")
    if "kernels" in what:
        kernels(sc, W, H, a.chunk_rows, a.reps, res)
    if "pipeline" in what:
        pipeline(sc, W, H, a.chunk_rows, a.reps, res)
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
