#!/usr/bin/env python3
"""The paper frame composed from the queries, on config 5's scene at 7680x4320
(33.2 M pixels; GPU box; DESIGN.md §Paper frames from the queries), every
buffer on the device:

  rays       rt_camera_rays_device (pixel centres)
  intersect  rt_query_intersect_device
  wo         rt_rays_wo_device
  shade      rt_query_shade_device, misses white
  resolve    rt_paper_resolve_device (fb and, with --edge, the edge map)

in --bands row bands with halos (1: the whole frame, about 7 GB of buffers),
against rt_render paper of the same frame, and against a device-to-device copy
that moves as many bytes as k_paper_resolve must (89 B in, 24 or 32 B out per
pixel).  The stage figures are device-event times: rt_stats.ms_kernel, and for
wo and the copy, which report none, HIP events on the default stream around
the call.  The composed frame is compared with rt_render's bytes.

Usage: python tools/paper_perf.py [--dpi 1920] [--bands 1] [--reps 5] [--edge] [--json PATH]"""
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


class Events:
    """Two HIP events on the default stream, from the runtime librtamd.so runs on."""

    def __init__(self):
        self.hip = C.CDLL(rtamd.check_one_hip_runtime())
        self.e = [C.c_void_p(), C.c_void_p()]
        for e in self.e:
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def time(self, fn):
        assert self.hip.hipEventRecord(self.e[0], None) == 0
        fn()
        assert self.hip.hipEventRecord(self.e[1], None) == 0
        assert self.hip.hipEventSynchronize(self.e[1]) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.e[0], self.e[1]) == 0
        return float(ms.value)

    def copy(self, dst, src, nbytes):
        self.hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        return self.time(lambda: self.hip.hipMemcpyAsync(dst.ptr, src.ptr, nbytes, 3, None))   # 3: device to device


def summary(ms):
    return {"min": min(ms), "median": float(np.median(ms)), "max": max(ms), "all": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dpi", type=int, default=1920, help="config 5's dpi (1920: 7680x4320)")
    ap.add_argument("--bands", type=int, default=1, help="row bands the frame is composed in")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--edge", action="store_true", help="also write the edge map (32 B out per pixel)")
    ap.add_argument("--json", default=None, help="also write the result line to this file")
    a = ap.parse_args()
    rtamd.amd_lib()
    sc = rtamd.load_scene_from_json_text(scenes.config_json(5, dpi=a.dpi)[0])
    W, H = sc.width, sc.height
    ev = Events()
    cuts = [H * k // a.bands for k in range(a.bands + 1)]
    bands = [(cuts[k], cuts[k + 1] - cuts[k]) for k in range(a.bands) if cuts[k + 1] > cuts[k]]
    n_max = max(rtamd.paper_band(H, r0, nr)[1] - rtamd.paper_band(H, r0, nr)[0] for r0, nr in bands) * W
    d_rays, d_hits, d_mask = rtamd.DeviceBuffer(n_max * 64), rtamd.DeviceBuffer(n_max * 64), rtamd.DeviceBuffer(n_max)
    d_wo, d_rgb = rtamd.DeviceBuffer(n_max * 24), rtamd.DeviceBuffer(n_max * 24)
    d_fb = rtamd.DeviceBuffer(W * H * 24)
    d_edge = rtamd.DeviceBuffer(W * H * 8) if a.edge else None
    stages = ("rays", "intersect", "wo", "shade", "resolve")
    t = {s: [] for s in stages}
    st = rtamd.Stats()
    for k in range(1 + a.reps):   # (one warm-up round)
        acc = dict.fromkeys(stages, 0.0)
        for row0, n_rows in bands:
            in0, in1 = rtamd.paper_band(H, row0, n_rows)
            n = (in1 - in0) * W
            rows = None if (in0, in1) == (0, H) else list(range(in0, in1))
            assert rtamd.camera_rays_device(sc, W, H, rtamd.RT_RAYS_CENTRE, rows, d_rays, stats=st) == n
            acc["rays"] += st.ms_kernel
            rtamd.query_intersect_device(sc, d_rays, n, d_hits, d_mask, stats=st)
            acc["intersect"] += st.ms_kernel
            acc["wo"] += ev.time(lambda: rtamd.rays_wo_device(d_rays, n, d_wo))
            rtamd.query_shade_device(sc, d_hits, d_wo, d_mask, n, d_rgb, miss_rgb=(1.0, 1.0, 1.0), stats=st)
            acc["shade"] += st.ms_kernel
            out = lambda b, per: None if b is None else type("At", (), {   # noqa: E731  (the band's rows of the frame)
                "ptr": C.c_void_p(b.ptr.value + row0 * W * per), "nbytes": b.nbytes - row0 * W * per})()
            rtamd.paper_resolve_device(d_hits, d_mask, d_rgb, W, H, row0, n_rows, out(d_fb, 24), out(d_edge, 8), stats=st)
            acc["resolve"] += st.ms_kernel
        if k:
            for s in stages:
                t[s].append(acc[s])
    fb = d_fb.to_host(shape=(H, W, 3))
    fst, tf = rtamd.Stats(), []
    for k in range(1 + a.reps):
        frame = rtamd.Tracer(sc, W, H, rtamd.RT_MODE_PAPER).render(fst)
        if k:
            tf.append(fst.ms_kernel)
    # the copy that moves k_paper_resolve's bytes: 89 in + 24 (32) out per pixel, half read and half written
    px_bytes = 89 + (32 if a.edge else 24)
    copy_bytes = W * H * px_bytes // 2
    d_a, d_b = rtamd.DeviceBuffer(copy_bytes), rtamd.DeviceBuffer(copy_bytes)
    tc = [ev.copy(d_b, d_a, copy_bytes) for _ in range(1 + a.reps)][1:]
    res = {"scene": "config 5", "W": W, "H": H, "pixels": W * H, "bands": len(bands), "edge": bool(a.edge),
           "equal_to_rt_render": bool(fb.tobytes() == frame.tobytes()),
           "pixels_differing": int((fb != frame).any(axis=2).sum()),
           "stages_ms": {s: summary(t[s]) for s in stages},
           "composed_ms_median": float(sum(np.median(t[s]) for s in stages)),
           "rt_render_paper_ms_kernel": summary(tf),
           "resolve_bytes_per_pixel": px_bytes, "copy_bytes": copy_bytes, "copy_ms": summary(tc)}
    res["resolve_GBps"] = W * H * px_bytes / (res["stages_ms"]["resolve"]["median"] * 1e6)
    res["copy_GBps"] = 2 * copy_bytes / (res["copy_ms"]["median"] * 1e6)
    res["resolve_vs_copy"] = res["stages_ms"]["resolve"]["median"] / res["copy_ms"]["median"]
    for s in stages:
        print(f"{s:10s}: min {min(t[s]):.3f} median {np.median(t[s]):.3f} max {max(t[s]):.3f} ms", flush=True)
    print(f"composed {res['composed_ms_median']:.3f} ms; rt_render paper kernel {np.median(tf):.3f} ms; "
          f"equal to rt_render: {res['equal_to_rt_render']}; resolve {res['resolve_GBps']:.0f} GB/s of "
          f"{px_bytes} B/px, copy of the same bytes {res['copy_GBps']:.0f} GB/s ({res['resolve_vs_copy']:.2f}x the copy's time)")
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
