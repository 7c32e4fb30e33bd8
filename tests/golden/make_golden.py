#!/usr/bin/env python3
"""Generate tests/golden/*.npz from the REFERENCE's own hot-path code.

Runs in the build container only: oracle/_ref/libref.so is the reference's
raytracer/src/{tracer,shading,scene,geometry,csg,transform}.cpp compiled in
place by oracle/Makefile with our harness (oracle/ref_harness.cpp); scenes are
turned into IR by our loader (librt_host.so).  Outputs are data only:

  frames.npz   framebuffers (float64) + Scene::intersect / Scene::occluded
               counts for every parity scene, standard and paper mode
  kats.npz     primitive-level known answers: random rays -> intersect and
               interval results for every node kind of the torture scenes
  jitter.npz   draws of std::mt19937(12345) + uniform_real_distribution(-0.5,0.5)
               at pixel/sample offsets up to the last pixels of 8K
  cameras.npz  Camera::generate_ray / generate_ray_subpixel outputs
  dirlights.npz  frames + counts of scenes with directional lights attached
               (scenes.dir_light_cases), standard and paper mode
  deep.npz     frames + counts of the scenes beyond the device's common
               stacks (scenes.deep_scenes: recursion 24, 12 nested
               transforms, a 12-leaf right-nested csg), both modes
  crowd.npz    frames + counts of the seeded 150-object random scenes
               (scenes.crowd_scene, seeds 1-3), both modes
  bvh.npz      frames + counts of the wave-BVH scenes (scenes.bvh_scenes:
               a 576-sphere lattice, exact closest-hit ties), both modes

  shading.npz  frames + counts of the shading scene family
               (scenes.shading_scenes: 33-65 lights, near and skipped lights,
               specular exponents, extreme coefficients, a non-vacuum medium,
               null materials), both modes, with each scene's JSON and the
               nodes / materials patched through the IR
  graph.npz    frames + counts of the scene-graph scenes (scenes.graph_cases,
               scenes.graph_scene at GRAPH_SEEDS), both modes, at GRAPH_DPI,
               and intersect / interval answers of every top-level object of
               the named cases for 64 rays per case
  leaves.npz, leaf_seeds.npz, leaf_rays.npz
               frames + counts of the leaf-parameter scenes (scenes.leaf_cases,
               scenes.leaf_scene at LEAF_SEEDS), both modes, at LEAF_DPI, and
               Scene::intersect / Scene::occluded of the non-finite and
               overflowing ray groups (scenes.odd_ray_groups)
  forest.npz   frames + counts of the forest scenes (scenes.forest_cases: more
               than 256 objects of mixed forms), both modes, and
               Scene::intersect / Scene::occluded of each case's query rays

Usage: python tests/golden/make_golden.py [frames kats jitter cameras dirlights deep crowd bvh shading graph leaves forest]
"""
from __future__ import annotations

import contextlib
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "raytracing-project_amd", "python"))

import rtamd  # noqa: E402
import scenes  # noqa: E402

_dp = C.POINTER(C.c_double)


@contextlib.contextmanager
def quiet_stdout():
    """The reference prints a progress bar to stdout (tracer.cpp:213-240)."""
    fd = os.dup(1)
    devnull = os.open(os.devnull, os.O_WRONLY)
    os.dup2(devnull, 1)
    try:
        yield
    finally:
        os.dup2(fd, 1)
        os.close(devnull)
        os.close(fd)


def parity_scenes(dpi_examples=16, dpi_torture=16) -> dict[str, str]:
    out = {}
    for name in ("penguin", "pokeballs", "snorlax"):
        out[name] = json.dumps(scenes.with_dpi(scenes.load_example(name), dpi_examples))
    for n in (2, 3, 4, 5):
        out[f"cfg{n}"] = scenes.config_json(n, dpi=dpi_examples)[0]
    for k, v in scenes.torture_scenes(dpi=dpi_torture).items():
        out[k] = json.dumps(v)
    return out


def make_frames():
    data = {}
    for name, text in parity_scenes().items():
        sc = rtamd.load_scene_from_json_text(text)
        for mode in (0, 1):
            with quiet_stdout():
                fb, ni, no = rtamd.ref_render(sc, sc.width, sc.height, mode)
            data[f"{name}/{mode}/fb"] = fb
            data[f"{name}/{mode}/counts"] = np.array([ni, no], dtype=np.int64)
            data[f"{name}/scene"] = np.frombuffer(text.encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "frames.npz"), **data)
    print("frames:", len(data))


def deep_golden_scenes() -> dict[str, dict]:
    """scenes.deep_scenes plus the recursion depths at the common kernels'
    stack edge (kMaxDepth = 16 frames: medium.recursion 17 the last on the
    common kernels, 18 the first on the big-stack ones)."""
    out = scenes.deep_scenes(dpi=12)
    for rec in (17, 18):
        out[f"mirrors_rec{rec}"] = scenes.deep_recursion_scene(rec, dpi=8)
    return out


def make_deep():
    data = {}
    for name, d in deep_golden_scenes().items():
        text = json.dumps(d)
        sc = rtamd.load_scene_from_json_text(text)
        for mode in (0, 1):
            with quiet_stdout():
                fb, ni, no = rtamd.ref_render(sc, sc.width, sc.height, mode)
            data[f"{name}/{mode}/fb"] = fb
            data[f"{name}/{mode}/counts"] = np.array([ni, no], dtype=np.int64)
        data[f"{name}/scene"] = np.frombuffer(text.encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "deep.npz"), **data)
    print("deep:", len(data))


def _random_rays(rng, n, center, spread):
    o = center + rng.normal(size=(n, 3)) * spread + np.array([0.0, 0.0, 4.0])
    tgt = center + rng.normal(size=(n, 3)) * spread * 0.6
    d = tgt - o
    # a few rays start inside the objects and a few are axis-parallel
    o[: n // 10] = center + rng.normal(size=(n // 10, 3)) * 0.2
    d[n // 10: n // 10 + 8] = np.array([1.0, 0.0, 0.0])
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def make_kats():
    rng = np.random.default_rng(1234)
    lib = rtamd.ref_lib()
    data = {}
    for sname, sc_json in scenes.torture_scenes(dpi=8).items():
        sc = rtamd.load_scene_from_json_text(json.dumps(sc_json))
        d = sc.desc
        for node in range(d.n_nodes):
            n = 128
            o, dirs = _random_rays(rng, n, np.zeros(3) + np.array([0.0, 0.0, -1.2]), 1.5)
            ok = (C.c_int * n)()
            hits = (rtamd.OracleHit * n)()
            for tag, (tmin, tmax) in (("isect", (1e-4, np.inf)), ("isect_win", (0.5, 4.0))):
                lib.ref_node_intersect_batch(sc.desc_ptr, node, n, o.ctypes.data_as(_dp), dirs.ctypes.data_as(_dp),
                                             tmin, tmax, ok, hits)
                data[f"{sname}/{node}/{tag}/ok"] = np.array(ok[:], dtype=np.int32)
                data[f"{sname}/{node}/{tag}/hit"] = _hits_array(hits)
                data[f"{sname}/{node}/{tag}/range"] = np.array([tmin, tmax])
            t0 = np.zeros(n)
            t1 = np.zeros(n)
            h0 = (rtamd.OracleHit * n)()
            h1 = (rtamd.OracleHit * n)()
            lib.ref_node_interval_batch(sc.desc_ptr, node, n, o.ctypes.data_as(_dp), dirs.ctypes.data_as(_dp), ok,
                                        t0.ctypes.data_as(_dp), t1.ctypes.data_as(_dp), h0, h1)
            data[f"{sname}/{node}/ivl/ok"] = np.array(ok[:], dtype=np.int32)
            data[f"{sname}/{node}/ivl/t"] = np.stack([t0, t1], axis=1)
            data[f"{sname}/{node}/ivl/h0"] = _hits_array(h0)
            data[f"{sname}/{node}/ivl/h1"] = _hits_array(h1)
            data[f"{sname}/{node}/o"] = o
            data[f"{sname}/{node}/d"] = dirs
        data[f"{sname}/scene"] = np.frombuffer(json.dumps(sc_json).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "kats.npz"), **data)
    print("kats:", len(data))


def _hits_array(hits):
    # t, p(3), n(3), mat, front_face  (mat/ff stored as float)
    return np.array([[h.t, *h.p, *h.n, float(h.mat), float(h.front_face)] for h in hits])


def make_jitter():
    lib = rtamd.ref_lib()
    points = []
    for W, H in ((640, 480), (3840, 2160), (7680, 4320)):
        npx = W * H
        for p in (0, 1, W - 1, W, npx // 2, npx - W, npx - 1):
            points.append(p)
    pts = sorted(set(points))
    draws = np.zeros((len(pts), 16))
    for i, p in enumerate(pts):
        buf = np.zeros(16)
        lib.ref_jitter(16 * p, 16, buf.ctypes.data_as(_dp))   # 8 samples x (dx, dy)
        draws[i] = buf
    words = np.zeros(4096, dtype=np.uint32)
    lib.ref_mt_words(0, 4096, words.ctypes.data_as(C.POINTER(C.c_uint32)))
    np.savez_compressed(os.path.join(HERE, "jitter.npz"), pixels=np.array(pts, dtype=np.int64), draws=draws,
                        words0=words)
    print("jitter points:", len(pts))


def make_cameras():
    lib = rtamd.ref_lib()
    rng = np.random.default_rng(7)
    data = {}
    for name in ("penguin", "pokeballs", "snorlax"):
        sc = rtamd.load_scene_from_json_text(json.dumps(scenes.load_example(name)))
        W, H = sc.width, sc.height
        rows = []
        for _ in range(200):
            i = int(rng.integers(-2, W + 2))
            j = int(rng.integers(-2, H + 2))
            dx, dy = rng.uniform(-0.5, 0.5, 2)
            for sub in (0, 1):
                o = np.zeros(3)
                d = np.zeros(3)
                lib.ref_camera_ray(sc.desc_ptr, i, j, dx, dy, sub, o.ctypes.data_as(_dp), d.ctypes.data_as(_dp))
                rows.append([i, j, dx, dy, sub, *o, *d])
        data[name] = np.array(rows)
    np.savez_compressed(os.path.join(HERE, "cameras.npz"), **data)
    print("cameras:", len(data))


def make_dirlights():
    """Directional-light frames (scenes.dir_light_cases), both modes."""
    data = {}
    for name, (text, lights) in scenes.dir_light_cases().items():
        sc = rtamd.with_dir_lights(rtamd.load_scene_from_json_text(text), lights)
        for mode in (0, 1):
            with quiet_stdout():
                fb, ni, no = rtamd.ref_render(sc, sc.width, sc.height, mode)
            data[f"{name}/{mode}/fb"] = fb
            data[f"{name}/{mode}/counts"] = np.array([ni, no], dtype=np.int64)
        data[f"{name}/lights"] = np.array(lights, dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "dirlights.npz"), **data)
    print("dirlights:", len(data))


CROWD_SEEDS = (1, 2, 3)


def make_crowd():
    """Seeded 150-object random scenes (scenes.crowd_scene), both modes."""
    data = {}
    for seed in CROWD_SEEDS:
        sc = rtamd.load_scene_from_json_text(json.dumps(scenes.crowd_scene(seed)))
        for mode in (0, 1):
            with quiet_stdout():
                fb, ni, no = rtamd.ref_render(sc, sc.width, sc.height, mode)
            data[f"{seed}/{mode}/fb"] = fb
            data[f"{seed}/{mode}/counts"] = np.array([ni, no], dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, "crowd.npz"), **data)
    print("crowd:", len(data))


def make_bvh():
    """Scenes of more than kWaveBvhMin = 256 objects (the wave BVH threshold) for the wave BVH
    (scenes.bvh_scenes), both modes."""
    data = {}
    for name, scene in scenes.bvh_scenes(dpi=16).items():
        sc = rtamd.load_scene_from_json_text(json.dumps(scene))
        for mode in (0, 1):
            with quiet_stdout():
                fb, ni, no = rtamd.ref_render(sc, sc.width, sc.height, mode)
            data[f"{name}/{mode}/fb"] = fb
            data[f"{name}/{mode}/counts"] = np.array([ni, no], dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, "bvh.npz"), **data)
    print("bvh:", len(data))


SHADING_DPI = 12


def make_shading():
    """The shading scene family (scenes.shading_scenes), both modes."""
    data = {}
    for name, d in scenes.shading_scenes(dpi=SHADING_DPI, detail=0.5).items():
        text = json.dumps(d)
        plain = rtamd.load_scene_from_json_text(text)
        null_nodes, kd0 = scenes.shading_patch_indices(rtamd, plain, name)
        sc = scenes.shading_apply(rtamd, plain, null_nodes, kd0)
        for mode in (0, 1):
            with quiet_stdout():
                fb, ni, no = rtamd.ref_render(sc, sc.width, sc.height, mode)
            data[f"{name}/{mode}/fb"] = fb
            data[f"{name}/{mode}/counts"] = np.array([ni, no], dtype=np.int64)
        data[f"{name}/scene"] = np.frombuffer(text.encode(), dtype=np.uint8)
        data[f"{name}/null_nodes"] = np.array(null_nodes, dtype=np.int32)
        data[f"{name}/kd0_mats"] = np.array(kd0, dtype=np.int32)
    np.savez_compressed(os.path.join(HERE, "shading.npz"), **data)
    print("shading:", len(data))


GRAPH_SEEDS = (2, 3, 8, 9, 10, 12)
GRAPH_DPI = 12   # 48 x 36 frames: the file stays under 1 MB


def graph_golden_scenes(dpi=GRAPH_DPI) -> dict[str, dict]:
    out = dict(scenes.graph_cases(dpi=dpi))
    for seed in GRAPH_SEEDS:
        out[f"seed{seed}"] = scenes.graph_scene(seed, dpi=dpi)
    return out


def make_graph():
    """The scene-graph scenes (scenes.graph_cases, scenes.graph_scene), both
    modes, and the named cases' top-level objects ray by ray (rows of misses
    are stored as zeros)."""
    lib = rtamd.ref_lib()
    rng = np.random.default_rng(4321)
    data = {"dpi": np.array(GRAPH_DPI, dtype=np.int64), "seeds": np.array(GRAPH_SEEDS, dtype=np.int64)}
    named = set(scenes.graph_cases())
    for name, d in graph_golden_scenes().items():
        sc = scenes.graph_load(rtamd, name, d)
        for mode in (0, 1):
            with quiet_stdout():
                fb, ni, no = rtamd.ref_render(sc, sc.width, sc.height, mode)
            data[f"{name}/{mode}/fb"] = fb
            data[f"{name}/{mode}/counts"] = np.array([ni, no], dtype=np.int64)
        if name not in named:
            continue
        n = 64
        o, dirs = _random_rays(rng, n, np.array([0.0, 0.0, -1.2]), 1.5)
        data[f"{name}/o"], data[f"{name}/d"] = o, dirs
        for k in range(sc.desc.n_objects):
            node = int(sc.desc.objects[k])
            ok = (C.c_int * n)()
            hits = (rtamd.OracleHit * n)()
            lib.ref_node_intersect_batch(sc.desc_ptr, node, n, o.ctypes.data_as(_dp), dirs.ctypes.data_as(_dp),
                                         1e-4, np.inf, ok, hits)
            okv = np.array(ok[:], dtype=np.int8)
            data[f"{name}/{k}/isect/ok"] = okv
            data[f"{name}/{k}/isect/hit"] = np.where(okv[:, None] != 0, _hits_array(hits), 0.0)
            t0, t1 = np.zeros(n), np.zeros(n)
            h0, h1 = (rtamd.OracleHit * n)(), (rtamd.OracleHit * n)()
            lib.ref_node_interval_batch(sc.desc_ptr, node, n, o.ctypes.data_as(_dp), dirs.ctypes.data_as(_dp), ok,
                                        t0.ctypes.data_as(_dp), t1.ctypes.data_as(_dp), h0, h1)
            okv = np.array(ok[:], dtype=np.int8)
            data[f"{name}/{k}/ivl/ok"] = okv
            data[f"{name}/{k}/ivl/rec"] = np.where(okv[:, None] != 0, np.concatenate(
                [np.stack([t0, t1], axis=1), _hits_array(h0), _hits_array(h1)], axis=1), 0.0)
    np.savez_compressed(os.path.join(HERE, "graph.npz"), **data)
    print("graph:", len(data))


LEAF_SEEDS = (1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13)
LEAF_DPI = 12   # 48 x 36 frames


def _ref_frames(data, name, d):
    sc = rtamd.load_scene_from_json_text(json.dumps(d))
    for mode in (0, 1):
        with quiet_stdout():
            fb, ni, no = rtamd.ref_render(sc, sc.width, sc.height, mode)
        data[f"{name}/{mode}/fb"] = fb
        data[f"{name}/{mode}/counts"] = np.array([ni, no], dtype=np.int64)


def make_leaves():
    """The leaf-parameter scenes (scenes.leaf_cases -> leaves.npz,
    scenes.leaf_scene at LEAF_SEEDS -> leaf_seeds.npz), both modes, and the
    reference's Scene::intersect / Scene::occluded of the non-finite and
    overflowing ray groups (scenes.odd_ray_groups on scenes.ODD_RAY_SCENES ->
    leaf_rays.npz: per "<scene>|<group>" the rays (o, d, tmin, tmax), the hit
    flags, the hit records (a miss is zeros) and the occluded flags)."""
    lib = rtamd.ref_lib()
    data = {"dpi": np.array(LEAF_DPI, dtype=np.int64)}
    for name, d in scenes.leaf_cases(dpi=LEAF_DPI).items():
        _ref_frames(data, name, d)
    np.savez_compressed(os.path.join(HERE, "leaves.npz"), **data)
    print("leaves:", len(data))
    data = {"dpi": np.array(LEAF_DPI, dtype=np.int64), "seeds": np.array(LEAF_SEEDS, dtype=np.int64)}
    for seed in LEAF_SEEDS:
        _ref_frames(data, f"seed{seed}", scenes.leaf_scene(seed, dpi=LEAF_DPI))
    np.savez_compressed(os.path.join(HERE, "leaf_seeds.npz"), **data)
    print("leaf_seeds:", len(data))
    data = {}
    for name in scenes.ODD_RAY_SCENES:
        sc = rtamd.load_scene_from_json_text(scenes.odd_ray_scene(name))
        o, d = np.zeros((scenes.ODD_RAY_N, 3)), np.zeros((scenes.ODD_RAY_N, 3))
        for k, (i, j) in enumerate(scenes.odd_ray_pixels(sc.width, sc.height)):
            lib.ref_camera_ray(sc.desc_ptr, i, j, 0.0, 0.0, 0, o[k].ctypes.data_as(_dp), d[k].ctypes.data_as(_dp))
        groups = dict(scenes.odd_ray_groups(o, d))
        if name.startswith("leaf/"):
            zero = [b["sphere"]["position"] for b in scenes.leaf_cases()[name[5:]]["objects"]
                    if "sphere" in b and b["sphere"]["radius"] == 0.0][0]
            groups["zero radius centre"] = scenes.zero_radius_centre_rays(zero)
        for tag, g in groups.items():
            rays = rtamd.make_rays(*g)
            ok, rec = rtamd.ref_scene_intersect(sc, rays)
            key = f"{name}|{tag}"
            data[key + "/rays"] = np.concatenate([rays["o"], rays["d"], rays["tmin"][:, None], rays["tmax"][:, None]], axis=1)
            data[key + "/ok"] = ok.astype(np.int8)
            data[key + "/hit"] = np.concatenate([rec["t"][:, None], rec["p"], rec["n"], rec["mat"][:, None].astype(float),
                                                 rec["front_face"][:, None].astype(float)], axis=1)
            data[key + "/occ"] = rtamd.ref_scene_occluded(sc, rays).astype(np.int8)
            # Tracer::trace of the same rays (its range is its own: tmin / tmax play no part)
            rgb, ni, no = rtamd.ref_trace(sc, rays["o"], rays["d"])
            data[key + "/rgb"] = rgb
            data[key + "/counts"] = np.stack([ni, no], axis=1)
        # shade_lambert_phong of the base rays' hits with odd fields (scenes.odd_hit_groups)
        base = rtamd.make_rays(o, d)
        ok, rec = rtamd.ref_scene_intersect(sc, base)
        for tag, (H, wo) in scenes.odd_hit_groups(rec[ok], -d[ok]).items():
            rgb, no = rtamd.ref_shade(sc, H, wo)
            data[f"{name}|shade {tag}/rgb"] = rgb
            data[f"{name}|shade {tag}/no"] = no
    np.savez_compressed(os.path.join(HERE, "leaf_rays.npz"), **data)
    print("leaf_rays:", len(data))


def make_forest():
    """The forest scenes (scenes.forest_cases at tests/test_forest_scenes.DPI),
    both modes, and the reference's Scene::intersect / Scene::occluded of each
    case's 768 query rays (the recipe of tests/test_forest_scenes.forest_case):
    packed hit and occluded flags, t (0 for a miss), material (-1) and the
    SHA-256 of the flags and full records (test_forest_scenes.records_digest;
    the records themselves, 55 KB a case, do not fit the file's 1 MB)."""
    sys.path.insert(0, os.path.dirname(HERE))
    import test_forest_scenes as F
    data = {"dpi": np.array(F.DPI, dtype=np.int64)}
    for name in F.KEYS:
        sc = F.load(rtamd, name)
        for mode in (0, 1):
            with quiet_stdout():
                fb, ni, no = rtamd.ref_render(sc, sc.width, sc.height, mode)
            data[f"{name}/{mode}/fb"] = fb
            data[f"{name}/{mode}/counts"] = np.array([ni, no], dtype=np.int64)
        c = F.forest_case(rtamd, name)
        ok, rec = rtamd.ref_scene_intersect(sc, c.rays)
        data[f"{name}/q/hit"] = np.packbits(ok)
        data[f"{name}/q/occ"] = np.packbits(rtamd.ref_scene_occluded(sc, c.seg_rays))
        data[f"{name}/q/t"] = np.where(ok, rec["t"], 0.0)
        data[f"{name}/q/mat"] = np.where(ok, rec["mat"], -1).astype(np.int32)
        data[f"{name}/q/sha"] = F.records_digest(ok, rec)
    np.savez_compressed(os.path.join(HERE, "forest.npz"), **data)
    print("forest:", len(data), os.path.getsize(os.path.join(HERE, "forest.npz")), "bytes")


if __name__ == "__main__":
    if len(sys.argv) > 1:
        for what in sys.argv[1:]:
            globals()["make_" + what]()
        sys.exit(0)
    make_frames()
    make_kats()
    make_jitter()
    make_cameras()
    make_dirlights()
    make_deep()
    make_crowd()
    make_bvh()
    make_shading()
    make_graph()
    make_leaves()
    make_forest()
