#!/usr/bin/env python3
"""Ray queries on the per-ray BVH (RT_FLAG_RAY_BVH) beside the flat kernels
(GPU box; DESIGN.md §Ray BVH).

The scene is scenes.bvh_perf_scene(n) for n = 4096, 1024, 300, resident; the
batches are its 1920x1080 centre rays from rt_camera_rays_device:

  camera    as generated (a wave's 64 rays are neighbours of a pixel row)
  shuffled  the same rays under a fixed random permutation: every wave incoherent
  segments  surface-to-surface segments between the camera rays' hit points
            (from p_a + 1e-3 n_a toward p_b, tmax their distance, shuffled),
            through rt_query_occluded

Each batch runs flat and flagged in the same process, alternating, on device
buffers; the time is rt_stats.ms_kernel, one warm-up, then the minimum of
--reps.  The two calls' bytes are compared on the way.

Usage: python tools/ray_bvh_perf.py [--sizes 4096,1024,300] [--reps 5] [--json PATH]"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracing-project_amd", "python"))

import rtamd  # noqa: E402
import scenes  # noqa: E402

SEED = 20250301


def timed(sc, kind, d_rays, n, d_hits, d_mask, reps):
    """(min ms flat, min ms flagged, all, bytes equal) of the query of `kind` over d_rays[0, n)."""
    ms = {0: [], rtamd.RT_FLAG_RAY_BVH: []}
    out = {}
    st = rtamd.Stats()
    for k in range(1 + reps):
        for fl in ms:
            if kind == 0:
                rtamd.query_intersect_device(sc, d_rays, n, d_hits, d_mask, fl, stats=st)
            else:
                rtamd.query_occluded_device(sc, d_rays, n, d_mask, fl, stats=st)
            if k:
                ms[fl].append(st.ms_kernel)
            else:
                out[fl] = (d_hits.to_host(np.uint8).tobytes() if kind == 0 else b"") + d_mask.to_host(np.uint8).tobytes()
    flat, bvh = ms[0], ms[rtamd.RT_FLAG_RAY_BVH]
    return {"flat_ms": min(flat), "ray_bvh_ms": min(bvh), "flat_over_ray_bvh": min(flat) / min(bvh),
            "flat_all": flat, "ray_bvh_all": bvh, "bytes_equal": out[0] == out[rtamd.RT_FLAG_RAY_BVH]}


def run(n_spheres, reps):
    sc = rtamd.load_scene_from_json_text(json.dumps(scenes.bvh_perf_scene(n_spheres)))
    W, H = sc.width, sc.height
    n = W * H
    rng = np.random.default_rng(SEED)
    d_rays, d_hits, d_mask = rtamd.DeviceBuffer(n * 64), rtamd.DeviceBuffer(n * 64), rtamd.DeviceBuffer(n)
    assert rtamd.camera_rays_device(sc, W, H, rtamd.RT_RAYS_CENTRE, None, d_rays) == n
    names = [rtamd.ray_bvh_kernel_name(sc, k, rtamd.RT_FLAG_RAY_BVH)[1] for k in (0, 1)]
    res = {"spheres": n_spheres, "W": W, "H": H, "rays": n, "kernels": names,
           "nodes": int(len(rtamd.ray_bvh_nodes(sc)[0]))}
    res["camera"] = timed(sc, 0, d_rays, n, d_hits, d_mask, reps)
    rays = d_rays.to_host(np.uint8).view(rtamd.RAY_DTYPE)
    hits = d_hits.to_host(np.uint8).view(rtamd.HIT_DTYPE)
    hit = d_mask.to_host(np.uint8).astype(bool)
    d_rays.from_host(rays[rng.permutation(n)])
    res["shuffled"] = timed(sc, 0, d_rays, n, d_hits, d_mask, reps)
    p, nn = hits["p"][hit], hits["n"][hit]
    a, b = rng.integers(0, len(p), n), rng.integers(0, len(p), n)
    so = p[a] + 1e-3 * nn[a]
    sd = p[b] - so
    d_rays.from_host(rtamd.make_rays(so, sd, 1e-4, np.sqrt((sd * sd).sum(axis=1))))
    res["segments"] = timed(sc, 1, d_rays, n, d_hits, d_mask, reps)
    res["segments"]["occluded_fraction"] = float(d_mask.to_host(np.uint8).mean())
    for b_ in (d_rays, d_hits, d_mask):
        b_.free()
    for tag in ("camera", "shuffled", "segments"):
        r = res[tag]
        print(f"{n_spheres:5d} spheres {tag:9s}: flat {r['flat_ms']:9.3f} ms  ray BVH {r['ray_bvh_ms']:9.3f} ms  "
              f"flat / ray BVH {r['flat_over_ray_bvh']:6.2f}  bytes equal {r['bytes_equal']}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,1024,300")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None, help="also write the result line to this file")
    a = ap.parse_args()
    res = {"lib": os.environ.get("RTAMD_LIB") or "lib/librtamd.so", "reps": a.reps,
           "runs": [run(int(s), a.reps) for s in a.sizes.split(",")]}
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
