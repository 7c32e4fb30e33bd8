"""rtamd — ctypes bindings over the C-ABI in include/rt.h.

This is test/bench plumbing, not the product: the product is the C-ABI
(lib/librtamd.so, lib/librt_host.so) and the `ray` CLI.  The Python names
mirror the reference's interface for the hot path:

* ``load_scene_from_json_text`` / ``load_scene_from_json`` ->
  ``jsonio::load_scene_from_json_text`` / ``load_scene_from_json``
  (raytracer/src/json_loader.cpp:458-503)
* ``Tracer(scene, width, height, mode).render()`` -> ``Tracer::render``
  (raytracer/src/tracer.h:18-35, tracer.cpp:247-305)
* ``query_intersect(scene, origins, dirs, ...)`` / ``query_occluded`` ->
  ``Scene::intersect`` / ``Scene::occluded`` for a batch of rays
  (raytracer/src/scene.cpp:10-24, 33-42)

The GPU path fails loudly (RuntimeError) when librtamd.so is missing or no HIP
device is present; there is no CPU fallback.  The CPU oracle (oracle/) and the
reference harness (oracle/_ref) are exposed separately for tests only.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_DIR = os.path.dirname(_HERE)
REPO_DIR = os.path.dirname(PKG_DIR)
LIB_DIR = os.path.join(PKG_DIR, "lib")
BIN_DIR = os.path.join(PKG_DIR, "bin")
ORACLE_DIR = os.path.join(REPO_DIR, "oracle")

RT_OK = 0
RT_MODE_STANDARD = 0
RT_MODE_PAPER = 1
RT_OK = 0
RT_ERR_INVALID_ARG = -1
RT_ERR_HIP = -5
RT_ERR_UNSUPPORTED = -6
RT_ERR_NO_DEVICE = -7
RT_FLAG_NONE = 0
RT_FLAG_COUNT_OPS = 1
RT_FLAG_NO_CULL = 2
RT_FLAG_FP32 = 4   # non-parity FP32 fast path
RT_FLAG_NO_BVH = 8   # wave culls without the wave BVH (A/B; identical results)
RT_FLAG_FORCE_BVH = 16   # the wave BVH on every frame (no on/off trial frames)
RT_FLAG_RAY_BVH = 32   # ray queries: every ray walks the ray BVH on its own (identical results)
RT_RAYS_CENTRE = 0     # rt_camera_rays: Camera::generate_ray at the pixel centres
RT_RAYS_JITTERED = 1   # ... generate_ray_subpixel at the frame's own RT_SPP jitter draws per pixel
RT_SPP = 8             # samples per pixel of a standard frame (tracer.cpp:283)
RT_SPAWN_REFLECT = 1   # rt_scatter_rays: the bits of spawn[i]
RT_SPAWN_REFRACT = 2

NODE_SPHERE, NODE_HALFSPACE, NODE_POKEBALL, NODE_TRANSLATION, NODE_SCALING, NODE_ROTATION, NODE_CSG = range(7)
CSG_UNION, CSG_INTERSECTION, CSG_DIFFERENCE = range(3)

OP_NAMES = [
    "sphere_isect", "sphere_isect_hit", "sphere_ivl", "sphere_ivl_hit", "half_isect", "half_isect_hit",
    "half_ivl", "poke_region", "csg_combine", "xform", "shade_light", "shade_spec", "secondary", "culled",
    "light_eval", "shade_call",
]


class Material(C.Structure):
    _fields_ = [("albedo", C.c_double * 3), ("ambient", C.c_double * 3), ("kd", C.c_double), ("ks", C.c_double),
                ("kr", C.c_double), ("kt", C.c_double), ("shininess", C.c_double),
                ("refractive_index", C.c_double)]


class Node(C.Structure):
    _fields_ = [("kind", C.c_int32), ("a", C.c_int32), ("b", C.c_int32), ("op", C.c_int32), ("mat", C.c_int32),
                ("mats", C.c_int32 * 5), ("v", C.c_double * 24), ("aux", C.c_double * 4)]


class Light(C.Structure):
    _fields_ = [("pos", C.c_double * 3), ("intensity", C.c_double * 3)]


class DirLight(C.Structure):
    _fields_ = [("dir", C.c_double * 3), ("radiance", C.c_double * 3)]


class Camera(C.Structure):
    _fields_ = [("eye", C.c_double * 3), ("P", C.c_double * 3), ("Lx", C.c_double), ("Ly", C.c_double),
                ("dpi", C.c_int32), ("pad_", C.c_int32)]


class SceneDesc(C.Structure):
    _fields_ = [("camera", Camera), ("background", C.c_double * 3), ("ambient", C.c_double * 3),
                ("medium_index", C.c_double), ("recursion_limit", C.c_int32), ("n_lights", C.c_int32),
                ("lights", C.POINTER(Light)), ("n_materials", C.c_int32), ("n_nodes", C.c_int32),
                ("materials", C.POINTER(Material)), ("nodes", C.POINTER(Node)), ("n_objects", C.c_int32),
                ("pad_", C.c_int32), ("objects", C.POINTER(C.c_int32)), ("n_dir_lights", C.c_int32),
                ("pad2_", C.c_int32), ("dir_lights", C.POINTER(DirLight))]


class Stats(C.Structure):
    _fields_ = [("rays_intersect", C.c_uint64), ("rays_occluded", C.c_uint64), ("rays_traced", C.c_uint64),
                ("pixels", C.c_uint64), ("ms_rng", C.c_double), ("ms_kernel", C.c_double),
                ("ms_total", C.c_double), ("ops", C.c_uint64 * 16),
                ("ms_gather", C.c_double), ("ms_tobyte", C.c_double), ("ms_d2h", C.c_double),
                ("n_gpus", C.c_int32), ("pad_", C.c_int32)]

    def as_dict(self) -> dict:
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "ops"}
        d["ops"] = {OP_NAMES[i]: int(self.ops[i]) for i in range(16)}
        return d


class OracleStats(C.Structure):
    _fields_ = [("rays_intersect", C.c_uint64), ("rays_occluded", C.c_uint64), ("ops", C.c_uint64 * 16)]


class OracleHit(C.Structure):
    _fields_ = [("t", C.c_double), ("p", C.c_double * 3), ("n", C.c_double * 3), ("mat", C.c_int32),
                ("front_face", C.c_int32)]

    def as_tuple(self):
        return (self.t, tuple(self.p), tuple(self.n), self.mat, self.front_face)


class Ray(C.Structure):
    """rt_ray: Ray(o, d) (d is normalised on the device, core.h:278) and its range."""
    _fields_ = [("o", C.c_double * 3), ("d", C.c_double * 3), ("tmin", C.c_double), ("tmax", C.c_double)]


class Hit(C.Structure):
    """rt_hit (the layout of oracle_hit); a miss: mat -1, every other field 0."""
    _fields_ = [("t", C.c_double), ("p", C.c_double * 3), ("n", C.c_double * 3), ("mat", C.c_int32),
                ("front_face", C.c_int32)]


# the same records as numpy dtypes (64 B each)
RAY_DTYPE = np.dtype([("o", "<f8", (3,)), ("d", "<f8", (3,)), ("tmin", "<f8"), ("tmax", "<f8")])
HIT_DTYPE = np.dtype([("t", "<f8"), ("p", "<f8", (3,)), ("n", "<f8", (3,)), ("mat", "<i4"), ("front_face", "<i4")])
assert RAY_DTYPE.itemsize == C.sizeof(Ray) == 64 and HIT_DTYPE.itemsize == C.sizeof(Hit) == 64

_dp = C.POINTER(C.c_double)


def _load(path: str, mode=C.RTLD_GLOBAL):
    if not os.path.exists(path):
        raise RuntimeError(f"required library not built: {path} (run __graft_entry__.build())")
    return C.CDLL(path, mode=mode)


_host = None
_amd = None
_oracle = None
_ref = None


def host_lib():
    global _host
    if _host is None:
        lib = _load(os.path.join(LIB_DIR, "librt_host.so"))
        lib.rt_last_error.restype = C.c_char_p
        lib.rt_scene_load_json_text.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p)]
        lib.rt_scene_load_json_file.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        lib.rt_scene_from_desc.argtypes = [C.POINTER(SceneDesc), C.POINTER(C.c_void_p)]
        lib.rt_scene_get_desc.argtypes = [C.c_void_p]
        lib.rt_scene_get_desc.restype = C.POINTER(SceneDesc)
        lib.rt_scene_destroy.argtypes = [C.c_void_p]
        lib.rt_camera_width.argtypes = [C.POINTER(Camera)]
        lib.rt_camera_height.argtypes = [C.POINTER(Camera)]
        lib.rt_framebuffer_to_rgb8.argtypes = [_dp, C.c_size_t, C.POINTER(C.c_uint8)]
        lib.rt_write_png.argtypes = [C.c_char_p, C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_int]
        if hasattr(lib, "rt_resolve_samples"):   # (absent only in builds of older sources)
            lib.rt_resolve_samples.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        if hasattr(lib, "rt_paper_resolve"):   # (likewise)
            lib.rt_rays_wo.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
            lib.rt_paper_resolve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_void_p, C.c_void_p]
        if hasattr(lib, "rt_scatter_rays"):   # (likewise)
            lib.rt_scatter_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                            C.POINTER(C.c_size_t), C.POINTER(Stats)]
            lib.rt_combine_bounce.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                              C.c_size_t]
        _host = lib
    return _host


def amd_lib():
    """The HIP renderer.  Raises if the extension is missing (no fallback)."""
    global _amd
    if _amd is None:
        host_lib()
        # RTAMD_LIB: diagnostic override (tools/ build experiments); never a fallback
        lib = _load(os.environ.get("RTAMD_LIB") or os.path.join(LIB_DIR, "librtamd.so"))
        lib.rt_render.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _dp, C.POINTER(Stats)]
        lib.rt_render_rows_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.c_void_p,
                                              C.POINTER(Stats)]
        lib.rt_scatter_rows_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        if hasattr(lib, "rt_frame_begin"):   # (absent only in RTAMD_LIB builds of older sources)
            lib.rt_frame_begin.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32),
                                           C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
            lib.rt_frame_trace.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
            lib.rt_frame_end.argtypes = [C.c_void_p, C.POINTER(Stats)]
        lib.rt_framebuffer_to_rgb8_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        if hasattr(lib, "rt_query_intersect"):   # (absent only in RTAMD_LIB builds of older sources)
            lib.rt_query_intersect.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p,
                                               C.POINTER(Stats)]
            lib.rt_query_occluded.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p,
                                              C.POINTER(Stats)]
            lib.rt_query_intersect_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.POINTER(Stats)]
            lib.rt_query_occluded_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p,
                                                     C.c_void_p, C.POINTER(Stats)]
        if hasattr(lib, "rt_query_node_intersect"):   # (absent only in RTAMD_LIB builds of older sources)
            lib.rt_query_node_intersect.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p,
                                                    C.c_void_p, C.POINTER(Stats)]
            lib.rt_query_node_interval.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.POINTER(Stats)]
            lib.rt_query_node_intersect_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int,
                                                           C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
            lib.rt_query_node_interval_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int,
                                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                          C.POINTER(Stats)]
            lib.rt_test_node_kernel_name.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]
            lib.rt_test_node_program.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int,
                                                 C.POINTER(C.c_int32)]
        if hasattr(lib, "rt_query_radiance"):   # (absent only in RTAMD_LIB builds of older sources)
            lib.rt_query_radiance.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p,
                                              C.POINTER(Stats)]
            lib.rt_query_radiance_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p,
                                                     C.c_void_p, C.POINTER(Stats)]
        if hasattr(lib, "rt_query_shade"):   # (likewise)
            lib.rt_query_shade.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                           C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(Stats)]
            lib.rt_query_shade_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                  C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                  C.POINTER(Stats)]
        if hasattr(lib, "rt_camera_rays"):   # (likewise)
            lib.rt_camera_rays.argtypes = [C.POINTER(Camera), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int,
                                           C.c_void_p, C.POINTER(Stats)]
            lib.rt_camera_rays_device.argtypes = [C.POINTER(Camera), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32),
                                                  C.c_int, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
            lib.rt_resolve_samples_device.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
            lib.rt_test_camera_chunk_rays.argtypes = [C.c_size_t]
        if hasattr(lib, "rt_paper_resolve_device"):   # (likewise)
            lib.rt_rays_wo_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
            lib.rt_paper_resolve_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                    C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        if hasattr(lib, "rt_scatter_rays_device"):   # (likewise)
            lib.rt_scatter_rays_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                   C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(Stats)]
            lib.rt_combine_bounce_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                     C.c_void_p, C.c_size_t, C.c_void_p]
            lib.rt_query_radiance_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p,
                                                    C.POINTER(Stats)]
            lib.rt_query_radiance_depth_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int,
                                                           C.c_void_p, C.c_void_p, C.POINTER(Stats)]
            lib.rt_test_scatter_launch_items.argtypes = [C.c_size_t]
        lib.rt_device_count.restype = C.c_int
        lib.rt_render_multi.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp,
                                        C.POINTER(Stats)]
        lib.rt_render_rgb8.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.POINTER(C.c_uint8), C.POINTER(Stats)]
        lib.rt_dist_get_id.argtypes = [C.POINTER(C.c_uint8)]
        lib.rt_dist_create.argtypes = [C.POINTER(C.c_uint8), C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        lib.rt_dist_destroy.argtypes = [C.c_void_p]
        lib.rt_dist_destroy.restype = None
        lib.rt_render_dist.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                       C.c_void_p, C.POINTER(Stats)]
        lib.rt_render_dist_rgb8.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            C.c_void_p, C.POINTER(Stats)]
        lib.rt_dist_rows.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]
        lib.rt_dist_rows_mode.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]
        lib.rt_test_render_dist_sim.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                _dp, C.POINTER(C.c_uint8)]
        lib.rt_test_dist_threads.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, _dp,
                                             C.POINTER(C.c_uint8)]
        lib.rt_dist_reduce_max.argtypes = [C.c_void_p, _dp, C.c_int]
        lib.rt_dist_barrier.argtypes = [C.c_void_p]
        lib.rt_dist_frame_split.argtypes = [C.c_void_p, _dp, C.c_int]
        lib.rt_set_device.argtypes = [C.c_int]
        lib.rt_device_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
        lib.rt_device_free.argtypes = [C.c_void_p]
        lib.rt_memcpy_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.rt_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.rt_stream_create.argtypes = [C.POINTER(C.c_void_p)]
        lib.rt_stream_destroy.argtypes = [C.c_void_p]
        lib.rt_test_dist_create_rccl1.argtypes = [C.POINTER(C.c_void_p)]
        check_one_hip_runtime()
        _amd = lib
    return _amd


def mapped_libraries(stem: str) -> list[str]:
    """Real paths of the shared objects whose file name starts with `stem`
    mapped into this process (/proc/self/maps)."""
    out = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                parts = line.split(None, 5)
                if len(parts) == 6:
                    path = parts[5].strip()
                    if os.path.basename(path).startswith(stem):
                        out.add(os.path.realpath(path))
    except OSError:
        return []
    return sorted(out)


ROCM_DIR = os.path.realpath(os.environ.get("ROCM_PATH", "/opt/rocm"))


def check_one_hip_runtime() -> str:
    """librtamd.so must run on ONE HIP runtime, the one `ray` and the
    INTEGRATION binding use: /opt/rocm's.  A process that imported torch
    first has torch's bundled runtime (same soname) already mapped, and
    librtamd.so binds to it; loading torch afterwards maps a second runtime
    (two runtimes torn down at exit aborted the process).  Raises in both
    cases; a single runtime outside ROCM_PATH only warns.  Returns the
    runtime's path."""
    hips = mapped_libraries("libamdhip64.so")
    if len(hips) > 1:
        raise RuntimeError("two HIP runtimes mapped in this process: " + ", ".join(hips) +
                           " (do not import torch in a process that uses librtamd.so)")
    if hips and os.sep + "torch" + os.sep in hips[0]:
        raise RuntimeError(f"librtamd.so is bound to torch's bundled HIP runtime {hips[0]} "
                           "(import torch after, or not at all in, a process that uses librtamd.so)")
    if hips and not hips[0].startswith(ROCM_DIR + os.sep):
        # one runtime, not a torch wheel's: another ROCm install (/opt/rocm-X.Y without the
        # /opt/rocm link, a distro package) is legitimate
        import warnings

        warnings.warn(f"librtamd.so runs on the HIP runtime {hips[0]}, outside ROCM_PATH={ROCM_DIR}")
    return hips[0] if hips else ""


def oracle_lib():
    """CPU oracle (TEST INFRASTRUCTURE ONLY)."""
    global _oracle
    if _oracle is None:
        lib = _load(os.path.join(ORACLE_DIR, "liboracle.so"), mode=C.RTLD_LOCAL)
        lib.oracle_render_rows.argtypes = [C.POINTER(SceneDesc), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp,
                                           C.POINTER(OracleStats), C.c_int]
        lib.oracle_node_intersect.argtypes = [C.POINTER(SceneDesc), C.c_int, _dp, _dp, C.c_double, C.c_double,
                                              C.POINTER(OracleHit)]
        lib.oracle_node_interval.argtypes = [C.POINTER(SceneDesc), C.c_int, _dp, _dp, _dp, _dp,
                                             C.POINTER(OracleHit), C.POINTER(OracleHit)]
        lib.oracle_scene_intersect.argtypes = [C.POINTER(SceneDesc), _dp, _dp, C.c_double, C.c_double,
                                               C.POINTER(OracleHit)]
        lib.oracle_scene_occluded.argtypes = [C.POINTER(SceneDesc), _dp, _dp, C.c_double, C.c_double]
        lib.oracle_camera_ray.argtypes = [C.POINTER(SceneDesc), C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                          _dp, _dp]
        lib.oracle_jitter.argtypes = [C.c_uint64, C.c_uint64, _dp]
        lib.oracle_mt_words.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32)]
        if hasattr(lib, "oracle_set_pow"):   # (absent only in a liboracle.so built from older sources: every
            # earlier entry point stays usable with it; oracle_pow / oracle_shade_hits then raise)
            lib.oracle_set_pow.argtypes = [C.c_int]
            lib.oracle_set_pow.restype = None
            lib.oracle_spec_pow.argtypes = [C.c_int, _dp, _dp, C.c_int, _dp]
            lib.oracle_spec_pow.restype = None
            lib.oracle_shade_hits.argtypes = [C.POINTER(SceneDesc), C.c_int, C.c_void_p, _dp, C.c_void_p, C.c_int, _dp,
                                              C.c_void_p]
        _oracle = lib
    return _oracle


def _oracle_pow_lib():
    """oracle_lib() with oracle_set_pow, oracle_spec_pow and oracle_shade_hits, or an error that says what to do."""
    lib = oracle_lib()
    if not hasattr(lib, "oracle_set_pow"):
        raise RuntimeError("liboracle.so was built from sources without oracle_set_pow (run __graft_entry__.build())")
    return lib


ORACLE_POW_LIBM = 0     # the reference: libm pow everywhere (every fixture under tests/golden)
ORACLE_POW_DEVICE = 1   # the correctly rounded x^k wherever the device takes pow_spec (rt_device.hpp)


@contextlib.contextmanager
def oracle_pow(mode: int):
    """The oracle's specular power (oracle_set_pow, process-wide) for the body
    of a `with`; mode 0, the reference, is back afterwards whatever happens.
    Answers computed under mode 1 are the device's yardstick only: keep them
    out of every cache that mode-0 tests read.  TEST ONLY."""
    lib = _oracle_pow_lib()
    if lib.oracle_get_pow() != ORACLE_POW_LIBM:
        raise RuntimeError("oracle_pow: the oracle is not in mode 0 (a nested or leaked mode)")
    lib.oracle_set_pow(int(mode))
    try:
        yield
    finally:
        lib.oracle_set_pow(ORACLE_POW_LIBM)


def oracle_spec_pow(x, y, any_x: bool = False) -> np.ndarray:
    """oracle_spec_pow: the oracle's pow(rdotv, shininess) of (x[i], y[i]) in
    the current mode (any_x: the shading queries' condition).  TEST ONLY."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    assert x.shape == y.shape and x.ndim == 1
    out = np.zeros_like(x)
    _oracle_pow_lib().oracle_spec_pow(len(x), x.ctypes.data_as(_dp), y.ctypes.data_as(_dp), 1 if any_x else 0,
                                 out.ctypes.data_as(_dp))
    return out


def ref_lib():
    """The reference's own sources compiled by oracle/Makefile (container only)."""
    global _ref
    if _ref is None:
        lib = _load(os.path.join(ORACLE_DIR, "_ref", "libref.so"), mode=C.RTLD_LOCAL)
        lib.ref_render.argtypes = [C.POINTER(SceneDesc), C.c_int, C.c_int, C.c_int, _dp, C.POINTER(C.c_uint64),
                                   C.POINTER(C.c_uint64)]
        lib.ref_node_intersect_batch.argtypes = [C.POINTER(SceneDesc), C.c_int, C.c_int, _dp, _dp, C.c_double,
                                                 C.c_double, C.POINTER(C.c_int), C.POINTER(OracleHit)]
        lib.ref_node_interval_batch.argtypes = [C.POINTER(SceneDesc), C.c_int, C.c_int, _dp, _dp,
                                                C.POINTER(C.c_int), _dp, _dp, C.POINTER(OracleHit),
                                                C.POINTER(OracleHit)]
        lib.ref_camera_ray.argtypes = [C.POINTER(SceneDesc), C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                       _dp, _dp]
        lib.ref_jitter.argtypes = [C.c_uint64, C.c_uint64, _dp]
        lib.ref_mt_words.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32)]
        if hasattr(lib, "ref_roundtrip"):
            lib.ref_roundtrip.argtypes = [C.POINTER(SceneDesc), C.POINTER(C.c_void_p)]
        _ref = lib
    return _ref


class RTError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(msg)
        self.code = code


def last_error() -> str:
    return host_lib().rt_last_error().decode("utf-8", "replace")


class Scene:
    """Owned rt_scene handle (scene IR)."""

    def __init__(self, handle: int):
        self._h = C.c_void_p(handle)

    @property
    def handle(self):
        return self._h

    @property
    def desc(self) -> SceneDesc:
        return host_lib().rt_scene_get_desc(self._h).contents

    @property
    def desc_ptr(self):
        return host_lib().rt_scene_get_desc(self._h)

    @property
    def width(self) -> int:
        return host_lib().rt_camera_width(C.byref(self.desc.camera))

    @property
    def height(self) -> int:
        return host_lib().rt_camera_height(C.byref(self.desc.camera))

    def close(self):
        if self._h and self._h.value:
            host_lib().rt_scene_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def load_scene_from_json_text(text: str) -> Scene:
    """jsonio::load_scene_from_json_text (json_loader.cpp:458); raises RTError."""
    raw = text.encode("utf-8")
    out = C.c_void_p()
    rc = host_lib().rt_scene_load_json_text(raw, len(raw), C.byref(out))
    if rc != RT_OK:
        raise RTError(rc, last_error())
    return Scene(out.value)


def load_scene_from_json(path: str) -> Scene:
    """jsonio::load_scene_from_json (json_loader.cpp:499)."""
    out = C.c_void_p()
    rc = host_lib().rt_scene_load_json_file(path.encode(), C.byref(out))
    if rc != RT_OK:
        raise RTError(rc, last_error())
    return Scene(out.value)


def scene_from_desc(desc: SceneDesc) -> Scene:
    out = C.c_void_p()
    rc = host_lib().rt_scene_from_desc(C.byref(desc), C.byref(out))
    if rc != RT_OK:
        raise RTError(rc, last_error())
    return Scene(out.value)


def with_dir_lights(scene: Scene, lights) -> Scene:
    """Copy of `scene` with directional lights [(dir, radiance), ...]: the
    reference's Scene::dir_lights (scene.h:10-15, 36), which its JSON loader
    never fills; reachable here through rt_scene_from_desc as there through
    the Scene API."""
    d = SceneDesc.from_buffer_copy(scene.desc)   # arrays are deep-copied by rt_scene_from_desc
    arr = (DirLight * max(1, len(lights)))()
    for i, (dv, rad) in enumerate(lights):
        arr[i].dir[:] = [float(v) for v in dv]
        arr[i].radiance[:] = [float(v) for v in rad]
    d.n_dir_lights = len(lights)
    d.dir_lights = C.cast(arr, C.POINTER(DirLight))
    return scene_from_desc(d)


def with_point_lights(scene: Scene, lights) -> Scene:
    """Copy of `scene` whose point lights are [(pos, intensity), ...] (the
    reference's Scene::point_lights); everything else, the directional lights
    included, is the scene's."""
    d = SceneDesc.from_buffer_copy(scene.desc)
    arr, d.n_lights = _light_array(lights)
    d.lights = C.cast(arr, C.POINTER(Light))
    return scene_from_desc(d)


def with_recursion_limit(scene: Scene, k: int) -> Scene:
    """Copy of `scene` with Scene::recursion_limit = k (at 1, Tracer::trace
    returns the hit's shade_lambert_phong: tracer.cpp:36-38)."""
    d = SceneDesc.from_buffer_copy(scene.desc)
    d.recursion_limit = int(k)
    return scene_from_desc(d)


def with_null_materials(scene: Scene, node_indices) -> Scene:
    """Copy of `scene` whose sphere / half-space nodes `node_indices` have no
    material (rt_node.mat = -1): the reference's default mat{nullptr}
    (geometry.h), which its JSON schema cannot spell; reachable here through
    rt_scene_from_desc as there through the constructors."""
    d = SceneDesc.from_buffer_copy(scene.desc)
    nodes = (Node * d.n_nodes)()
    C.memmove(nodes, d.nodes, C.sizeof(Node) * d.n_nodes)
    for i in node_indices:
        i = int(i)
        if not 0 <= i < d.n_nodes or nodes[i].kind not in (NODE_SPHERE, NODE_HALFSPACE):
            raise ValueError(f"node {i} is not a sphere or half-space of this scene")
        nodes[i].mat = -1
    d.nodes = C.cast(nodes, C.POINTER(Node))
    return scene_from_desc(d)


def with_material_fields(scene: Scene, changes: dict) -> Scene:
    """Copy of `scene` with Material fields set, {material index: {field:
    value}}: values the JSON schema cannot give (kd is 1 for every colour
    block, json_loader.cpp:83-123)."""
    d = SceneDesc.from_buffer_copy(scene.desc)
    mats = (Material * d.n_materials)()
    C.memmove(mats, d.materials, C.sizeof(Material) * d.n_materials)
    for i, fields in changes.items():
        if not 0 <= int(i) < d.n_materials:
            raise ValueError(f"no material {i} in this scene")
        for k, v in fields.items():
            setattr(mats[int(i)], k, float(v))
    d.materials = C.cast(mats, C.POINTER(Material))
    return scene_from_desc(d)


def sphere_nodes_at(scene: Scene, centres) -> list[int]:
    """Node index of the sphere node at each of `centres` (exact coordinates)."""
    d = scene.desc
    out = []
    for c in centres:
        found = [i for i in range(d.n_nodes)
                 if d.nodes[i].kind == NODE_SPHERE and tuple(d.nodes[i].v[0:3]) == tuple(float(x) for x in c)]
        if len(found) != 1:
            raise ValueError(f"{len(found)} sphere nodes at {list(c)}")
        out.append(found[0])
    return out


def _kernel_name(hook: str, scene: Scene, *args: int) -> tuple[int, str]:
    """(status, "ns::kernel") from the rt_test_*_kernel_name hook `hook` of (scene, *args)."""
    fn = getattr(amd_lib(), hook)
    fn.argtypes = [C.c_void_p] + [C.c_int] * len(args) + [C.c_char_p, C.c_int]
    buf = C.create_string_buffer(160)
    rc = fn(scene.handle, *args, buf, 160)
    return rc, buf.value.decode()


def _kernel_rows(hook: str, table: int) -> list[str]:
    """The rows ("ns::kernel") of table `table` from the rt_test_*_kernel_row hook
    `hook`, read from the table the launcher searches."""
    fn = getattr(amd_lib(), hook)
    fn.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_int]
    buf = C.create_string_buffer(160)
    out = []
    while fn(table, len(out), buf, 160) == RT_OK:
        out.append(buf.value.decode())
    return out


def kernel_name(scene: Scene, mode: int, flags: int = RT_FLAG_NONE) -> tuple[int, str]:
    """rt_test_kernel_name: (status, "ns::kernel") of the trace kernel a frame
    of this scene, mode and flags launches.  Host only."""
    return _kernel_name("rt_test_kernel_name", scene, mode, flags)


OBJ_KINDS = ("sphere", "half", "poke", "chain", "eager", "never", "group")
OP_CODES = ("xpush", "leaf_ivl", "csg", "xpop_ivl", "leaf_isect", "csg_isect", "xpop_hit", "never", "ivl_group")
CSG_OPS = ("union", "intersection", "difference")


def compile_forms(scene: Scene) -> dict:
    """rt_test_compile_forms: the histogram of a scene's compiled forms
    (include/rt_test.h), as {"obj/<kind>", "chain_core/leaf|csg",
    "chain_m/0|1|2|3+", "chain_m3+/leaf|csg", "fold/<op>", "op/<code>",
    "never_top/0|1|2", "ivl_group/<op>", "max_ray_depth", "max_ivl_depth",
    "bounded", "prefilter"}.
    Host only."""
    lib = amd_lib()
    lib.rt_test_compile_forms.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int]
    n = 37   # RT_TEST_FORMS_LEN
    out = (C.c_int32 * n)()
    rc = lib.rt_test_compile_forms(scene.handle, out, n)
    if rc != RT_OK:
        raise RTError(rc, last_error())
    keys = ([f"obj/{k}" for k in OBJ_KINDS] + ["chain_core/leaf", "chain_core/csg"] +
            [f"chain_m/{m}" for m in ("0", "1", "2", "3+")] + ["chain_m3+/leaf", "chain_m3+/csg"] +
            [f"fold/{o}" for o in CSG_OPS] + [f"op/{k}" for k in OP_CODES] +
            [f"never_top/{t}" for t in (0, 1, 2)] + [f"ivl_group/{o}" for o in CSG_OPS] +
            ["max_ray_depth", "max_ivl_depth", "bounded", "prefilter"])
    assert len(keys) == n
    return dict(zip(keys, (int(v) for v in out)))


KERNEL_TABLES = ("rtd std", "rtd paper", "rtf std", "rtf paper", "rtdb std", "rtdb paper", "rtd query", "rtdb query",
                 "finish")


def kernel_rows(table: int) -> list[str]:
    """rt_test_kernel_row: the rows ("ns::kernel") of launch table `table`
    (an index into KERNEL_TABLES), read from the table the launcher searches.
    Host only."""
    return _kernel_rows("rt_test_kernel_row", table)


def launch_log(on: bool) -> None:
    """rt_test_launch_log: clear the launch log and start recording (True), or stop (False)."""
    _ok(amd_lib().rt_test_launch_log(1 if on else 0), "rt_test_launch_log")


def launch_log_get() -> list[str]:
    """rt_test_launch_log_get: the kernels ("ns::kernel") launched since
    launch_log(True), in launch order."""
    lib = amd_lib()
    lib.rt_test_launch_log_get.argtypes = [C.c_char_p, C.c_int]
    cap = 1 << 16
    while True:
        buf = C.create_string_buffer(cap)
        n = lib.rt_test_launch_log_get(buf, cap)
        if n >= 0:
            lines = buf.value.decode().splitlines()
            assert len(lines) == n, (len(lines), n)
            return lines
        if cap >= 1 << 26:
            raise RTError(n, last_error())
        cap *= 16


def pow_spec(x, y) -> np.ndarray:
    """rt_test_pow_spec: the device's pow_spec(x[i], y[i]) (rt_device.hpp)."""
    lib = amd_lib()
    lib.rt_test_pow_spec.argtypes = [_dp, _dp, C.c_int, _dp]
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    assert x.shape == y.shape and x.ndim == 1
    out = np.zeros_like(x)
    _ok(lib.rt_test_pow_spec(x.ctypes.data_as(_dp), y.ctypes.data_as(_dp), len(x), out.ctypes.data_as(_dp)),
        "rt_test_pow_spec")
    return out


def spec_skip(n, wi, wo, shin) -> tuple[np.ndarray, np.ndarray]:
    """rt_test_spec_skip: (skip (m,) bool, plain (m,)) of the device's spec_skips
    (rt_device.hpp) on (n[i], wi[i], wo[i], shin[i]): whether the trace kernels
    leave the lane's specular term out, and the power they compute where they
    do not."""
    lib = amd_lib()
    _ip = C.POINTER(C.c_int)
    lib.rt_test_spec_skip.argtypes = [_dp, _dp, _dp, _dp, C.c_int, _ip, _dp]
    n, wi, wo = (np.ascontiguousarray(a, dtype=np.float64) for a in (n, wi, wo))
    shin = np.ascontiguousarray(shin, dtype=np.float64)
    assert n.ndim == 2 and n.shape[1] == 3 and wi.shape == n.shape and wo.shape == n.shape and shin.shape == (len(n),)
    skip, plain = np.zeros(len(n), dtype=np.int32), np.zeros(len(n))
    _ok(lib.rt_test_spec_skip(n.ctypes.data_as(_dp), wi.ctypes.data_as(_dp), wo.ctypes.data_as(_dp),
                              shin.ctypes.data_as(_dp), len(n), skip.ctypes.data_as(_ip), plain.ctypes.data_as(_dp)),
        "rt_test_spec_skip")
    return skip.astype(bool), plain


_u64p = C.POINTER(C.c_uint64)


def jitter_cache_stats(slot: int | None = None) -> dict:
    """rt_test_jitter_cache_stats: {hits, misses, entries, bytes} of the jitter
    cache of the calling thread's workspace on the current device, or of
    workspace slot `slot` (r + 1: simulated rank r of dist_threads)."""
    lib = amd_lib()
    lib.rt_test_jitter_cache_stats.argtypes = [_u64p] * 4
    lib.rt_test_jitter_cache_stats_slot.argtypes = [C.c_int] + [_u64p] * 4
    v = [C.c_uint64() for _ in range(4)]
    refs = [C.byref(x) for x in v]
    if slot is None:
        _ok(lib.rt_test_jitter_cache_stats(*refs), "rt_test_jitter_cache_stats")
    else:
        _ok(lib.rt_test_jitter_cache_stats_slot(slot, *refs), "rt_test_jitter_cache_stats_slot")
    return dict(zip(("hits", "misses", "entries", "bytes"), (int(x.value) for x in v)))


def jitter_cache_budget(nbytes: int) -> None:
    """rt_test_jitter_cache_budget: the cache budget of every workspace in
    bytes (0: off, < 0: back to RT_JITTER_CACHE_MB); frees every cached entry
    and zeroes the counts."""
    lib = amd_lib()
    lib.rt_test_jitter_cache_budget.argtypes = [C.c_int64]
    _ok(lib.rt_test_jitter_cache_budget(nbytes), "rt_test_jitter_cache_budget")


def jitter_cache_sim(ops, budget: int) -> tuple[int, list[dict]]:
    """rt_test_jitter_cache_sim: the cache's logic over host memory.  ops:
    [(op, W, row0, n_rows, arg), ...] (jitter_cache.hpp jitter_cache_sim);
    returns (status, the state after each op).  Host only."""
    lib = amd_lib()
    lib.rt_test_jitter_cache_sim.argtypes = [C.POINTER(C.c_int64), C.c_int, C.c_int64, C.POINTER(C.c_int64)]
    n = len(ops)
    flat = (C.c_int64 * (5 * n))(*[int(v) for o in ops for v in o])
    out = (C.c_int64 * (8 * n))()
    rc = lib.rt_test_jitter_cache_sim(flat, n, budget, out)
    names = ("buffer", "fill", "upload_rows", "entries", "bytes", "live", "hits", "misses")
    return rc, [dict(zip(names, out[8 * k:8 * k + 8])) for k in range(n)]


def device_count() -> int:
    return int(amd_lib().rt_device_count())


def _ok(rc: int, what: str):
    if rc != RT_OK:
        raise RTError(rc, f"{what}: {last_error()}")


def set_device(dev: int):
    _ok(amd_lib().rt_set_device(dev), "rt_set_device")


def device_synchronize():
    _ok(amd_lib().rt_device_synchronize(), "rt_device_synchronize")


class DeviceBuffer:
    """A device allocation made by librtamd.so itself (rt_device_alloc): the
    tests and bench need no second HIP runtime (torch) for their buffers."""

    def __init__(self, nbytes: int):
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        _ok(amd_lib().rt_device_alloc(self.nbytes, C.byref(p)), "rt_device_alloc")
        self.ptr = p

    def to_host(self, dtype=np.float64, shape=None) -> np.ndarray:
        out = np.empty(self.nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        _ok(amd_lib().rt_memcpy_d2h(out.ctypes.data_as(C.c_void_p), self.ptr, out.nbytes), "rt_memcpy_d2h")
        return out.reshape(shape) if shape is not None else out

    def from_host(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        _ok(amd_lib().rt_memcpy_h2d(self.ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes), "rt_memcpy_h2d")

    def free(self):
        if self.ptr is not None and self.ptr.value:
            amd_lib().rt_device_free(self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Stream:
    """A non-blocking HIP stream made by librtamd.so (rt_stream_create)."""

    def __init__(self):
        p = C.c_void_p()
        _ok(amd_lib().rt_stream_create(C.byref(p)), "rt_stream_create")
        self.handle = p

    def destroy(self):
        if self.handle is not None and self.handle.value:
            amd_lib().rt_stream_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def shutdown():
    """rt_shutdown: release every device resource the library caches."""
    _ok(amd_lib().rt_shutdown(), "rt_shutdown")


@dataclass
class Tracer:
    """Mirror of the reference's Tracer (tracer.h:18-35) over the GPU C-ABI."""
    scene: Scene
    width: int
    height: int
    mode: int = RT_MODE_STANDARD
    flags: int = RT_FLAG_NONE

    def render(self, stats: Stats | None = None) -> np.ndarray:
        lib = amd_lib()
        fb = np.zeros((self.height, self.width, 3), dtype=np.float64)
        st = stats if stats is not None else Stats()
        rc = lib.rt_render(self.scene.handle, self.width, self.height, self.mode, self.flags,
                           fb.ctypes.data_as(_dp), C.byref(st))
        if rc != RT_OK:
            raise RTError(rc, last_error())
        return fb


def make_rays(origins, dirs, tmin=1e-4, tmax=np.inf) -> np.ndarray:
    """An rt_ray array (RAY_DTYPE) from (n, 3) origins and directions; scalar
    tmin / tmax broadcast.  Directions need not be normalised."""
    o = np.asarray(origins, dtype=np.float64)
    d = np.asarray(dirs, dtype=np.float64)
    if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
        raise ValueError(f"origins and dirs must both be (n, 3) arrays, got {o.shape} and {d.shape}")
    rays = np.empty(o.shape[0], dtype=RAY_DTYPE)
    rays["o"], rays["d"] = o, d
    rays["tmin"] = np.broadcast_to(np.asarray(tmin, dtype=np.float64), (o.shape[0],))
    rays["tmax"] = np.broadcast_to(np.asarray(tmax, dtype=np.float64), (o.shape[0],))
    return rays


@dataclass
class QueryHits:
    """query_intersect's result: `records` is the rt_hit array (HIT_DTYPE; a
    miss has mat -1 and zeros), `hit` the hit flags as bools."""
    records: np.ndarray
    hit: np.ndarray

    t = property(lambda self: self.records["t"])
    p = property(lambda self: self.records["p"])
    n = property(lambda self: self.records["n"])
    mat = property(lambda self: self.records["mat"])
    front_face = property(lambda self: self.records["front_face"])

    def __len__(self):
        return len(self.records)


def query_intersect(scene: Scene, origins, dirs, tmin=1e-4, tmax=np.inf, flags: int = RT_FLAG_NONE,
                    stats: Stats | None = None) -> QueryHits:
    """rt_query_intersect: Scene::intersect (closest hit) of every ray."""
    rays = make_rays(origins, dirs, tmin, tmax)
    n = len(rays)
    hits = np.zeros(n, dtype=HIT_DTYPE)
    mask = np.zeros(n, dtype=np.uint8)
    st = stats if stats is not None else Stats()
    rc = amd_lib().rt_query_intersect(scene.handle, rays.ctypes.data_as(C.c_void_p), n, flags,
                                      hits.ctypes.data_as(C.c_void_p), mask.ctypes.data_as(C.c_void_p), C.byref(st))
    if rc != RT_OK:
        raise RTError(rc, last_error())
    return QueryHits(hits, mask.astype(bool))


def query_occluded(scene: Scene, origins, dirs, tmin=1e-4, tmax=np.inf, flags: int = RT_FLAG_NONE,
                   stats: Stats | None = None) -> np.ndarray:
    """rt_query_occluded: Scene::occluded (any hit in [tmin, tmax]) of every ray, as bools."""
    rays = make_rays(origins, dirs, tmin, tmax)
    n = len(rays)
    occ = np.zeros(n, dtype=np.uint8)
    st = stats if stats is not None else Stats()
    rc = amd_lib().rt_query_occluded(scene.handle, rays.ctypes.data_as(C.c_void_p), n, flags,
                                     occ.ctypes.data_as(C.c_void_p), C.byref(st))
    if rc != RT_OK:
        raise RTError(rc, last_error())
    return occ.astype(bool)


def query_intersect_device(scene: Scene, rays_dev: DeviceBuffer, n: int, hits_dev: DeviceBuffer,
                           mask_dev: DeviceBuffer | None, flags: int = RT_FLAG_NONE, stream: Stream | None = None,
                           stats: Stats | None = None) -> None:
    """rt_query_intersect_device: the first n rt_ray records of rays_dev into
    the first n rt_hit records of hits_dev (and n flag bytes of mask_dev, when
    given), on `stream` (None: the default stream)."""
    if n < 0 or rays_dev.nbytes < n * RAY_DTYPE.itemsize or hits_dev.nbytes < n * HIT_DTYPE.itemsize \
            or (mask_dev is not None and mask_dev.nbytes < n):
        raise ValueError("query_intersect_device: a buffer is too small for n rays")
    st = stats if stats is not None else Stats()
    rc = amd_lib().rt_query_intersect_device(scene.handle, rays_dev.ptr, n, flags, hits_dev.ptr,
                                             mask_dev.ptr if mask_dev is not None else None,
                                             stream.handle if stream else None, C.byref(st))
    if rc != RT_OK:
        raise RTError(rc, last_error())


def query_occluded_device(scene: Scene, rays_dev: DeviceBuffer, n: int, occluded_dev: DeviceBuffer,
                          flags: int = RT_FLAG_NONE, stream: Stream | None = None, stats: Stats | None = None) -> None:
    """rt_query_occluded_device: the first n rt_ray records of rays_dev into n
    flag bytes of occluded_dev, on `stream` (None: the default stream)."""
    if n < 0 or rays_dev.nbytes < n * RAY_DTYPE.itemsize or occluded_dev.nbytes < n:
        raise ValueError("query_occluded_device: a buffer is too small for n rays")
    st = stats if stats is not None else Stats()
    rc = amd_lib().rt_query_occluded_device(scene.handle, rays_dev.ptr, n, flags, occluded_dev.ptr,
                                            stream.handle if stream else None, C.byref(st))
    if rc != RT_OK:
        raise RTError(rc, last_error())


def query_kernel_name(scene: Scene, kind: int, flags: int = RT_FLAG_NONE) -> tuple[int, str]:
    """rt_test_query_kernel_name: (status, "ns::kernel") of the kernel a query
    of kind 0 (intersect) / 1 (occluded) launches.  Host only."""
    return _kernel_name("rt_test_query_kernel_name", scene, kind, flags)


# ------------------------------------------------------------------ ray BVH
RAY_BVH_NODE_DTYPE = np.dtype([("c", "<f4", (4,)), ("skip", "<i4"), ("first", "<i4"), ("count", "<i4"),
                               ("pad", "<i4")])   # RayBvhNode (ray_bvh_rules.hpp)
assert RAY_BVH_NODE_DTYPE.itemsize == 32


def ray_bvh_kernel_name(scene: Scene, kind: int, flags: int = RT_FLAG_RAY_BVH) -> tuple[int, str]:
    """rt_test_ray_bvh_kernel_name: (status, "ns::kernel") of the kernel a ray
    query of kind 0 (intersect) / 1 (occluded) launches with these flags: the
    ray-BVH row where RT_FLAG_RAY_BVH takes effect, else the flat row.  Host only."""
    return _kernel_name("rt_test_ray_bvh_kernel_name", scene, kind, flags)


def ray_bvh_rows() -> list[str]:
    """rt_test_ray_bvh_row: the rows ("rtd::kernel") of the ray-BVH launch table.  Host only."""
    fn = amd_lib().rt_test_ray_bvh_row
    fn.argtypes = [C.c_int, C.c_char_p, C.c_int]
    buf = C.create_string_buffer(160)
    out = []
    while fn(len(out), buf, 160) == RT_OK:
        out.append(buf.value.decode())
    return out


def ray_bvh_nodes(scene: Scene) -> tuple[np.ndarray, int, int]:
    """rt_test_ray_bvh: (nodes (RAY_BVH_NODE_DTYPE), lead, n_wave) of the scene's
    ray BVH: the tree lies over objects [lead, n_wave) of the wave list.  No
    tree: an empty node array.  Host only."""
    lib = amd_lib()
    lib.rt_test_ray_bvh.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_int]
    counts = (C.c_int32 * 3)()
    _ok(lib.rt_test_ray_bvh(scene.handle, counts, None, 0), "rt_test_ray_bvh")
    nodes = np.zeros(int(counts[0]), dtype=RAY_BVH_NODE_DTYPE)
    if len(nodes):
        _ok(lib.rt_test_ray_bvh(scene.handle, counts, nodes.ctypes.data_as(C.c_void_p), len(nodes)), "rt_test_ray_bvh")
    return nodes, int(counts[1]), int(counts[2])


def ray_bvh_walk(scene: Scene, origins, dirs, tmin=1e-4, tmax=np.inf) -> tuple[np.ndarray, np.ndarray]:
    """rt_test_ray_bvh_walk: (reached (n, n_objects) bool, node tests (n,)) of
    the kernels' walk restated on the host, for each ray's fixed segment
    [tmin, tmax]: the top-level objects whose evaluation the walk reaches.
    Raises RTError (RT_ERR_UNSUPPORTED) for a scene without a tree.  Host only."""
    lib = amd_lib()
    lib.rt_test_ray_bvh_walk.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    rays = make_rays(origins, dirs, tmin, tmax)
    n, n_obj = len(rays), int(scene.desc.n_objects)
    cand = np.zeros((n, n_obj), dtype=np.uint8)
    tests = np.zeros(n, dtype=np.int32)
    rc = lib.rt_test_ray_bvh_walk(scene.handle, rays.ctypes.data_as(C.c_void_p), n, cand.ctypes.data_as(C.c_void_p),
                                  tests.ctypes.data_as(C.c_void_p))
    if rc != RT_OK:
        raise RTError(rc, last_error())
    return cand.astype(bool), tests


# ------------------------------------------------------------- node queries
NODE_ISECT, NODE_IVL = 0, 1  # node query kinds (scene_compile.hpp kNodeIsect / kNodeIvl)


def query_node_intersect(scene: Scene, node: int, origins, dirs, tmin=1e-4, tmax=np.inf, flags: int = RT_FLAG_NONE,
                         stats: Stats | None = None) -> QueryHits:
    """rt_query_node_intersect: Primitive::intersect of node `node` (an index
    into the scene's nodes) for every ray."""
    rays = make_rays(origins, dirs, tmin, tmax)
    n = len(rays)
    hits = np.zeros(n, dtype=HIT_DTYPE)
    mask = np.zeros(n, dtype=np.uint8)
    st = stats if stats is not None else Stats()
    rc = amd_lib().rt_query_node_intersect(scene.handle, node, rays.ctypes.data_as(C.c_void_p), n, flags,
                                           hits.ctypes.data_as(C.c_void_p), mask.ctypes.data_as(C.c_void_p),
                                           C.byref(st))
    if rc != RT_OK:
        raise RTError(rc, last_error())
    return QueryHits(hits, mask.astype(bool))


def query_node_interval(scene: Scene, node: int, origins, dirs, flags: int = RT_FLAG_NONE,
                        stats: Stats | None = None):
    """rt_query_node_interval: Primitive::interval of node `node` for every
    ray, as (enter, exit, ok): two rt_hit arrays (HIT_DTYPE; t is tEnter /
    tExit; zeros with mat -1 where ok is False) and the return values as bools."""
    rays = make_rays(origins, dirs)
    n = len(rays)
    enter, ex = np.zeros(n, dtype=HIT_DTYPE), np.zeros(n, dtype=HIT_DTYPE)
    mask = np.zeros(n, dtype=np.uint8)
    st = stats if stats is not None else Stats()
    rc = amd_lib().rt_query_node_interval(scene.handle, node, rays.ctypes.data_as(C.c_void_p), n, flags,
                                          enter.ctypes.data_as(C.c_void_p), ex.ctypes.data_as(C.c_void_p),
                                          mask.ctypes.data_as(C.c_void_p), C.byref(st))
    if rc != RT_OK:
        raise RTError(rc, last_error())
    return enter, ex, mask.astype(bool)


def query_node_intersect_device(scene: Scene, node: int, rays_dev: DeviceBuffer, n: int, hits_dev: DeviceBuffer,
                                mask_dev: DeviceBuffer | None, flags: int = RT_FLAG_NONE,
                                stream: Stream | None = None, stats: Stats | None = None) -> None:
    """rt_query_node_intersect_device: the first n rt_ray records of rays_dev
    into the first n rt_hit records of hits_dev (and n flag bytes of mask_dev,
    when given), on `stream` (None: the default stream)."""
    if n < 0 or rays_dev.nbytes < n * RAY_DTYPE.itemsize or hits_dev.nbytes < n * HIT_DTYPE.itemsize \
            or (mask_dev is not None and mask_dev.nbytes < n):
        raise ValueError("query_node_intersect_device: a buffer is too small for n rays")
    st = stats if stats is not None else Stats()
    rc = amd_lib().rt_query_node_intersect_device(scene.handle, node, rays_dev.ptr, n, flags, hits_dev.ptr,
                                                  mask_dev.ptr if mask_dev is not None else None,
                                                  stream.handle if stream else None, C.byref(st))
    if rc != RT_OK:
        raise RTError(rc, last_error())


def query_node_interval_device(scene: Scene, node: int, rays_dev: DeviceBuffer, n: int,
                               enter_dev: DeviceBuffer | None, exit_dev: DeviceBuffer | None,
                               mask_dev: DeviceBuffer | None, flags: int = RT_FLAG_NONE,
                               stream: Stream | None = None, stats: Stats | None = None) -> None:
    """rt_query_node_interval_device: the first n rt_ray records of rays_dev
    into the first n rt_hit records of enter_dev / exit_dev and n flag bytes of
    mask_dev (each optional, not all three absent), on `stream`."""
    if n < 0 or rays_dev.nbytes < n * RAY_DTYPE.itemsize \
            or any(b is not None and b.nbytes < n * HIT_DTYPE.itemsize for b in (enter_dev, exit_dev)) \
            or (mask_dev is not None and mask_dev.nbytes < n):
        raise ValueError("query_node_interval_device: a buffer is too small for n rays")
    st = stats if stats is not None else Stats()
    ptr = lambda b: b.ptr if b is not None else None   # noqa: E731
    rc = amd_lib().rt_query_node_interval_device(scene.handle, node, rays_dev.ptr, n, flags, ptr(enter_dev),
                                                 ptr(exit_dev), ptr(mask_dev), stream.handle if stream else None,
                                                 C.byref(st))
    if rc != RT_OK:
        raise RTError(rc, last_error())


def node_kernel_name(scene: Scene, node: int, kind: int, flags: int = RT_FLAG_NONE) -> tuple[int, str]:
    """rt_test_node_kernel_name: (status, "ns::kernel") of the kernel a node
    query of kind NODE_ISECT / NODE_IVL of this node launches.  Host only."""
    buf = C.create_string_buffer(160)
    rc = amd_lib().rt_test_node_kernel_name(scene.handle, node, kind, flags, buf, 160)
    return rc, buf.value.decode()


NODE_TABLES = ("rtd node", "rtdb node")


def node_rows(table: int) -> list[str]:
    """rt_test_node_kernel_row: the rows ("ns::kernel") of node launch table
    `table` (an index into NODE_TABLES).  Host only."""
    return _kernel_rows("rt_test_node_kernel_row", table)


def node_program(scene: Scene, node: int, kind: int):
    """rt_test_node_program: (ops, (max_ray_depth, max_ivl_depth)) of the
    node's own program; ops as (opcode name of OP_CODES, node, top, csg_op)
    tuples.  Host only."""
    lib = amd_lib()
    depths = (C.c_int32 * 2)()
    n = lib.rt_test_node_program(scene.handle, node, kind, None, 0, depths)
    if n < 0:
        raise RTError(n, last_error())
    buf = (C.c_int32 * (4 * max(1, n)))()
    assert lib.rt_test_node_program(scene.handle, node, kind, buf, n, depths) == n
    ops = [(OP_CODES[buf[4 * i]], int(buf[4 * i + 1]), int(buf[4 * i + 2]), int(buf[4 * i + 3])) for i in range(n)]
    return ops, (int(depths[0]), int(depths[1]))


def query_radiance(scene: Scene, origins, dirs, flags: int = RT_FLAG_NONE, stats: Stats | None = None) -> np.ndarray:
    """rt_query_radiance: Tracer::trace (the radiance along the ray) of every
    ray, as an (n, 3) float64 array.  tmin / tmax play no part."""
    rays = make_rays(origins, dirs)
    n = len(rays)
    rgb = np.zeros((n, 3), dtype=np.float64)
    st = stats if stats is not None else Stats()
    rc = amd_lib().rt_query_radiance(scene.handle, rays.ctypes.data_as(C.c_void_p), n, flags,
                                     rgb.ctypes.data_as(C.c_void_p), C.byref(st))
    if rc != RT_OK:
        raise RTError(rc, last_error())
    return rgb


def query_radiance_device(scene: Scene, rays_dev: DeviceBuffer, n: int, rgb_dev: DeviceBuffer,
                          flags: int = RT_FLAG_NONE, stream: Stream | None = None,
                          stats: Stats | None = None) -> None:
    """rt_query_radiance_device: the first n rt_ray records of rays_dev into
    the first 3n doubles of rgb_dev, on `stream` (None: the default stream)."""
    if n < 0 or rays_dev.nbytes < n * RAY_DTYPE.itemsize or rgb_dev.nbytes < n * 24:
        raise ValueError("query_radiance_device: a buffer is too small for n rays")
    st = stats if stats is not None else Stats()
    rc = amd_lib().rt_query_radiance_device(scene.handle, rays_dev.ptr, n, flags, rgb_dev.ptr,
                                            stream.handle if stream else None, C.byref(st))
    if rc != RT_OK:
        raise RTError(rc, last_error())


def radiance_kernel_name(scene: Scene, flags: int = RT_FLAG_NONE) -> tuple[int, str]:
    """rt_test_radiance_kernel_name: (status, "ns::kernel") of the kernel a
    radiance query of this scene and flags launches.  Host only."""
    return _kernel_name("rt_test_radiance_kernel_name", scene, flags)


RADIANCE_TABLES = ("rtd radiance", "rtdb radiance")


def radiance_rows(table: int) -> list[str]:
    """rt_test_radiance_kernel_row: the rows ("ns::kernel") of radiance launch
    table `table` (an index into RADIANCE_TABLES).  Host only."""
    return _kernel_rows("rt_test_radiance_kernel_row", table)


def _light_array(lights):
    """(rt_light array or None, n_lights) of a light override: None = the
    scene's own (n_lights -1), else [(pos, intensity), ...]."""
    if lights is None:
        return None, -1
    arr = (Light * max(1, len(lights)))()
    for i, (pos, inten) in enumerate(lights):
        arr[i].pos[:] = [float(v) for v in pos]
        arr[i].intensity[:] = [float(v) for v in inten]
    return arr, len(lights)


def query_shade(scene: Scene, hits, wo, mask=None, lights=None, miss_rgb=None, flags: int = RT_FLAG_NONE,
                stats: Stats | None = None) -> np.ndarray:
    """rt_query_shade: shade_lambert_phong(scene, hits[i], wo[i]) of every
    entry, as an (n, 3) float64 array.  hits: a HIT_DTYPE array (t, p, n, mat
    are read); wo: (n, 3); mask (optional, n bytes): entries with 0 get
    miss_rgb (None: the scene's background); lights: None = the scene's own
    point lights, else [(pos, intensity), ...] instead of them."""
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    n = len(hits)
    wo = np.ascontiguousarray(wo, dtype=np.float64)
    if wo.shape != (n, 3):
        raise ValueError(f"wo must be an (n, 3) array for n = {n} hits, got {wo.shape}")
    m = None
    if mask is not None:
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        if m.shape != (n,):
            raise ValueError(f"mask must hold n = {n} flags, got {m.shape}")
    arr, nl = _light_array(lights)
    miss = None if miss_rgb is None else (C.c_double * 3)(*[float(v) for v in miss_rgb])
    rgb = np.zeros((n, 3), dtype=np.float64)
    st = stats if stats is not None else Stats()
    rc = amd_lib().rt_query_shade(scene.handle, hits.ctypes.data_as(C.c_void_p), wo.ctypes.data_as(C.c_void_p),
                                  m.ctypes.data_as(C.c_void_p) if m is not None else None, n,
                                  C.cast(arr, C.c_void_p) if arr is not None else None, nl,
                                  C.cast(miss, C.c_void_p) if miss is not None else None, flags,
                                  rgb.ctypes.data_as(C.c_void_p), C.byref(st))
    if rc != RT_OK:
        raise RTError(rc, last_error())
    return rgb


def query_shade_device(scene: Scene, hits_dev: DeviceBuffer, wo_dev: DeviceBuffer, mask_dev: DeviceBuffer | None,
                       n: int, rgb_dev: DeviceBuffer, lights=None, miss_rgb=None, flags: int = RT_FLAG_NONE,
                       stream: Stream | None = None, stats: Stats | None = None) -> None:
    """rt_query_shade_device: the first n rt_hit records of hits_dev with the
    first 3n doubles of wo_dev (and the first n bytes of mask_dev, when given)
    into the first 3n doubles of rgb_dev, on `stream` (None: the default
    stream).  lights / miss_rgb are host values, as for query_shade."""
    if n < 0 or hits_dev.nbytes < n * HIT_DTYPE.itemsize or wo_dev.nbytes < n * 24 or rgb_dev.nbytes < n * 24 \
            or (mask_dev is not None and mask_dev.nbytes < n):
        raise ValueError("query_shade_device: a buffer is too small for n entries")
    arr, nl = _light_array(lights)
    miss = None if miss_rgb is None else (C.c_double * 3)(*[float(v) for v in miss_rgb])
    st = stats if stats is not None else Stats()
    rc = amd_lib().rt_query_shade_device(scene.handle, hits_dev.ptr, wo_dev.ptr,
                                         mask_dev.ptr if mask_dev is not None else None, n,
                                         C.cast(arr, C.c_void_p) if arr is not None else None, nl,
                                         C.cast(miss, C.c_void_p) if miss is not None else None, flags, rgb_dev.ptr,
                                         stream.handle if stream else None, C.byref(st))
    if rc != RT_OK:
        raise RTError(rc, last_error())


def shade_kernel_name(scene: Scene, flags: int = RT_FLAG_NONE) -> tuple[int, str]:
    """rt_test_shade_kernel_name: (status, "ns::kernel") of the kernel a
    shading query of this scene and flags launches.  Host only."""
    return _kernel_name("rt_test_shade_kernel_name", scene, flags)


SHADE_TABLES = ("rtd shade", "rtdb shade")


def shade_rows(table: int) -> list[str]:
    """rt_test_shade_kernel_row: the rows ("ns::kernel") of shade launch
    table `table` (an index into SHADE_TABLES).  Host only."""
    return _kernel_rows("rt_test_shade_kernel_row", table)


def _camera_of(cam_or_scene) -> Camera:
    """An rt_camera: a Camera as it is, or a copy of a Scene's."""
    if isinstance(cam_or_scene, Camera):
        return cam_or_scene
    if isinstance(cam_or_scene, Scene):
        return Camera.from_buffer_copy(cam_or_scene.desc.camera)
    raise TypeError(f"expected a Camera or a Scene, got {type(cam_or_scene).__name__}")


def _rows_arg(rows, H: int):
    """(int32 array or None, n_rows) of a rows list; None: all H rows in order."""
    if rows is None:
        return None, H
    arr = np.ascontiguousarray(rows, dtype=np.int32)
    if arr.ndim != 1:
        raise ValueError("rows must be a flat list of output rows")
    return arr, len(arr)


def camera_rays(cam_or_scene, W: int, H: int, kind: int, rows=None, stats: Stats | None = None) -> np.ndarray:
    """rt_camera_rays: the rays of output rows `rows` (None: all, in order) of
    a W x H frame seen through the camera, as a RAY_DTYPE array of shape
    (n_rows, W) for RT_RAYS_CENTRE (Camera::generate_ray) or (n_rows, W,
    RT_SPP) for RT_RAYS_JITTERED (generate_ray_subpixel at the frame's own
    draws, samples in the order the frame sums them)."""
    cam = _camera_of(cam_or_scene)
    arr, n_rows = _rows_arg(rows, H)
    shape = (n_rows, max(W, 0), RT_SPP) if kind == RT_RAYS_JITTERED else (n_rows, max(W, 0))
    rays = np.zeros(shape, dtype=RAY_DTYPE)
    st = stats if stats is not None else Stats()
    rc = amd_lib().rt_camera_rays(C.byref(cam), W, H, kind,
                                  arr.ctypes.data_as(C.POINTER(C.c_int32)) if arr is not None else None, n_rows,
                                  rays.ctypes.data_as(C.c_void_p), C.byref(st))
    if rc != RT_OK:
        raise RTError(rc, last_error())
    return rays


def camera_rays_device(cam_or_scene, W: int, H: int, kind: int, rows, rays_dev: DeviceBuffer,
                       stream: Stream | None = None, stats: Stats | None = None) -> int:
    """rt_camera_rays_device: the same rays into rays_dev, on `stream` (None:
    the default stream).  Returns the number of rays written."""
    cam = _camera_of(cam_or_scene)
    arr, n_rows = _rows_arg(rows, H)
    n = n_rows * max(W, 0) * (RT_SPP if kind == RT_RAYS_JITTERED else 1)
    if rays_dev.nbytes < n * RAY_DTYPE.itemsize:
        raise ValueError("camera_rays_device: the ray buffer is too small")
    st = stats if stats is not None else Stats()
    rc = amd_lib().rt_camera_rays_device(C.byref(cam), W, H, kind,
                                         arr.ctypes.data_as(C.POINTER(C.c_int32)) if arr is not None else None, n_rows,
                                         rays_dev.ptr, stream.handle if stream else None, C.byref(st))
    if rc != RT_OK:
        raise RTError(rc, last_error())
    return n


def resolve_samples(rgb, spp: int) -> np.ndarray:
    """rt_resolve_samples (host): rgb (..., spp, 3) summed over the samples in
    order and scaled by 1.0 / spp, as the frame does (tracer.cpp:291-296)."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float64)
    if rgb.ndim < 2 or rgb.shape[-1] != 3 or rgb.shape[-2] != spp:
        raise ValueError(f"rgb must have shape (..., {spp}, 3), got {rgb.shape}")
    fb = np.zeros(rgb.shape[:-2] + (3,), dtype=np.float64)
    rc = host_lib().rt_resolve_samples(rgb.ctypes.data_as(C.c_void_p), fb.size // 3, spp, fb.ctypes.data_as(C.c_void_p))
    if rc != RT_OK:
        raise RTError(rc, last_error())
    return fb


def resolve_samples_device(rgb_dev: DeviceBuffer, n_pixels: int, spp: int, fb_dev: DeviceBuffer,
                           stream: Stream | None = None) -> None:
    """rt_resolve_samples_device: the first n_pixels * spp colours of rgb_dev
    into the first n_pixels colours of fb_dev, on `stream`."""
    if n_pixels < 0 or rgb_dev.nbytes < n_pixels * max(spp, 0) * 24 or fb_dev.nbytes < n_pixels * 24:
        raise ValueError("resolve_samples_device: a buffer is too small")
    rc = amd_lib().rt_resolve_samples_device(rgb_dev.ptr, n_pixels, spp, fb_dev.ptr, stream.handle if stream else None)
    if rc != RT_OK:
        raise RTError(rc, last_error())


def rays_wo(rays) -> np.ndarray:
    """rt_rays_wo (host): wo = (-Ray(o, d).d).normalized() of every rt_ray of a
    RAY_DTYPE array, as an array of its shape + (3,): what Tracer::trace and
    trace_paper hand to shade_lambert_phong, so query_shade's wo for the hits
    of these rays."""
    rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
    wo = np.zeros(rays.shape + (3,), dtype=np.float64)
    rc = host_lib().rt_rays_wo(rays.ctypes.data_as(C.c_void_p), rays.size, wo.ctypes.data_as(C.c_void_p))
    if rc != RT_OK:
        raise RTError(rc, last_error())
    return wo


def rays_wo_device(rays_dev: DeviceBuffer, n: int, wo_dev: DeviceBuffer, stream: Stream | None = None) -> None:
    """rt_rays_wo_device: the first n rt_ray records of rays_dev into the first
    3n doubles of wo_dev, on `stream` (None: the default stream)."""
    if n < 0 or rays_dev.nbytes < n * RAY_DTYPE.itemsize or wo_dev.nbytes < n * 24:
        raise ValueError("rays_wo_device: a buffer is too small for n rays")
    rc = amd_lib().rt_rays_wo_device(rays_dev.ptr, n, wo_dev.ptr, stream.handle if stream else None)
    if rc != RT_OK:
        raise RTError(rc, last_error())


def paper_band(H: int, row0: int, n_rows: int) -> tuple[int, int]:
    """The frame rows [in0, in1) that paper_resolve's inputs hold for output
    rows [row0, row0 + n_rows): the band and the halo rows inside the frame."""
    return max(0, row0 - 1), min(H, row0 + n_rows + 1)


def paper_resolve(hits, mask, rgb, W: int, H: int, row0: int = 0, n_rows: int | None = None, want_edge: bool = False):
    """rt_paper_resolve (host): output rows [row0, row0 + n_rows) (None: to the
    last row) of the W x H paper frame whose G-buffer rows paper_band(H, row0,
    n_rows) are hits (HIT_DTYPE), mask (bytes, or None: all hits) and rgb (the
    shading on white, 3 doubles a pixel).  Returns fb (n_rows, W, 3), or (fb,
    edge (n_rows, W)) with want_edge."""
    if n_rows is None:
        n_rows = H - row0
    in0, in1 = paper_band(H, row0, n_rows)
    n_in = max(in1 - in0, 0) * max(W, 0)
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    rgb = np.ascontiguousarray(rgb, dtype=np.float64)
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    if hits.size != n_in or rgb.size != 3 * n_in or (m is not None and m.size != n_in):
        raise ValueError(f"paper_resolve: inputs must hold rows [{in0}, {in1}) of width {W}")
    fb = np.zeros((max(n_rows, 0), max(W, 0), 3), dtype=np.float64)
    edge = np.zeros((max(n_rows, 0), max(W, 0)), dtype=np.float64) if want_edge else None
    rc = host_lib().rt_paper_resolve(hits.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p) if m is not None else None,
                                     rgb.ctypes.data_as(C.c_void_p), W, H, row0, n_rows, fb.ctypes.data_as(C.c_void_p),
                                     edge.ctypes.data_as(C.c_void_p) if want_edge else None)
    if rc != RT_OK:
        raise RTError(rc, last_error())
    return (fb, edge) if want_edge else fb


def paper_resolve_device(hits_dev: DeviceBuffer, mask_dev: DeviceBuffer | None, rgb_dev: DeviceBuffer | None, W: int,
                         H: int, row0: int, n_rows: int, fb_dev: DeviceBuffer | None,
                         edge_dev: DeviceBuffer | None = None, stream: Stream | None = None,
                         stats: Stats | None = None) -> None:
    """rt_paper_resolve_device: the same from device buffers holding rows
    paper_band(H, row0, n_rows), into the first n_rows*W colours of fb_dev and
    / or the first n_rows*W doubles of edge_dev, on `stream`."""
    in0, in1 = paper_band(H, row0, n_rows)
    n_in, n_out = max(in1 - in0, 0) * max(W, 0), max(n_rows, 0) * max(W, 0)
    if hits_dev.nbytes < n_in * HIT_DTYPE.itemsize or (mask_dev is not None and mask_dev.nbytes < n_in) \
            or (rgb_dev is not None and rgb_dev.nbytes < n_in * 24) or (fb_dev is not None and fb_dev.nbytes < n_out * 24) \
            or (edge_dev is not None and edge_dev.nbytes < n_out * 8):
        raise ValueError("paper_resolve_device: a buffer is too small")
    st = stats if stats is not None else Stats()
    opt = lambda b: b.ptr if b is not None else None   # noqa: E731
    rc = amd_lib().rt_paper_resolve_device(hits_dev.ptr, opt(mask_dev), opt(rgb_dev), W, H, row0, n_rows, opt(fb_dev),
                                           opt(edge_dev), stream.handle if stream else None, C.byref(st))
    if rc != RT_OK:
        raise RTError(rc, last_error())


def scatter_rays(scene: Scene, rays, hits, mask=None, depth: int = 0, child_cap: int | None = None,
                 stats: Stats | None = None):
    """rt_scatter_rays (host): the children that Tracer::trace_recursive spawns
    at recursion depth `depth` for the parents (rays[i], hits[i]) (RAY_DTYPE /
    HIT_DTYPE arrays; mask: n bytes or None = every entry is a hit).  Returns
    (spawn (n,) uint8, first (n,) uint64, child_rays (m,) RAY_DTYPE, child_w
    (m,)), compacted in parent order, reflection before refraction.  child_cap
    (None: 2n, which cannot fail): with fewer than m entries the call raises
    RTError with the needed m in `.needed`."""
    rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    n = len(rays)
    if hits.shape != (n,):
        raise ValueError(f"hits must hold n = {n} records, got {hits.shape}")
    m_in = None
    if mask is not None:
        m_in = np.ascontiguousarray(mask, dtype=np.uint8)
        if m_in.shape != (n,):
            raise ValueError(f"mask must hold n = {n} flags, got {m_in.shape}")
    cap = 2 * n if child_cap is None else int(child_cap)
    spawn, first = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint64)
    child_rays, child_w = np.zeros(cap, dtype=RAY_DTYPE), np.zeros(cap, dtype=np.float64)
    m = C.c_size_t(0)
    st = stats if stats is not None else Stats()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = host_lib().rt_scatter_rays(scene.handle, ptr(rays), ptr(hits), ptr(m_in) if m_in is not None else None, n,
                                    depth, ptr(spawn), ptr(first), ptr(child_rays), ptr(child_w), cap, C.byref(m),
                                    C.byref(st))
    if rc != RT_OK:
        err = RTError(rc, last_error())
        err.needed = int(m.value)
        raise err
    return spawn, first, child_rays[:m.value], child_w[:m.value]


def scatter_rays_device(scene: Scene, rays_dev: DeviceBuffer, hits_dev: DeviceBuffer, mask_dev: DeviceBuffer | None,
                        n: int, depth: int, spawn_dev: DeviceBuffer, first_dev: DeviceBuffer,
                        child_rays_dev: DeviceBuffer | None, child_w_dev: DeviceBuffer | None, child_cap: int,
                        stream: Stream | None = None, stats: Stats | None = None) -> int:
    """rt_scatter_rays_device: the same from the first n records of rays_dev /
    hits_dev (and n bytes of mask_dev, when given) into spawn_dev (n bytes),
    first_dev (n uint64) and at most child_cap records of child_rays_dev /
    doubles of child_w_dev, on `stream`.  Returns m, the number of children;
    m > child_cap raises RTError with m in `.needed`."""
    if n < 0 or rays_dev.nbytes < n * RAY_DTYPE.itemsize or hits_dev.nbytes < n * HIT_DTYPE.itemsize \
            or (mask_dev is not None and mask_dev.nbytes < n) or spawn_dev.nbytes < n or first_dev.nbytes < 8 * n \
            or child_cap < 0 or (child_cap and (child_rays_dev is None or child_w_dev is None)) \
            or (child_rays_dev is not None and child_rays_dev.nbytes < child_cap * RAY_DTYPE.itemsize) \
            or (child_w_dev is not None and child_w_dev.nbytes < child_cap * 8):
        raise ValueError("scatter_rays_device: a buffer is too small")
    m = C.c_size_t(0)
    st = stats if stats is not None else Stats()
    opt = lambda b: b.ptr if b is not None else None   # noqa: E731
    rc = amd_lib().rt_scatter_rays_device(scene.handle, rays_dev.ptr, hits_dev.ptr, opt(mask_dev), n, depth,
                                          spawn_dev.ptr, first_dev.ptr, opt(child_rays_dev), opt(child_w_dev), child_cap,
                                          C.byref(m), stream.handle if stream else None, C.byref(st))
    if rc != RT_OK:
        err = RTError(rc, last_error())
        err.needed = int(m.value)
        raise err
    return int(m.value)


def combine_bounce(rgb, spawn, first, child_rgb, child_w) -> np.ndarray:
    """rt_combine_bounce (host): the parents' direct colours rgb (n, 3) folded
    with their children's colours child_rgb (m, 3) scaled by child_w (m,), as
    tracer.cpp:47, :66 do; returns the totals (n, 3) (rgb is not changed)."""
    out = np.array(rgb, dtype=np.float64, order="C", copy=True)
    n = out.size // 3
    spawn = np.ascontiguousarray(spawn, dtype=np.uint8)
    first = np.ascontiguousarray(first, dtype=np.uint64)
    crgb = np.ascontiguousarray(child_rgb, dtype=np.float64)
    cw = np.ascontiguousarray(child_w, dtype=np.float64)
    if out.size != 3 * n or spawn.size != n or first.size != n or crgb.size != 3 * cw.size:
        raise ValueError("combine_bounce: rgb (n, 3), spawn (n,), first (n,), child_rgb (m, 3), child_w (m,)")
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None   # noqa: E731
    rc = host_lib().rt_combine_bounce(ptr(out), ptr(spawn), ptr(first), n, ptr(crgb), ptr(cw), cw.size)
    if rc != RT_OK:
        raise RTError(rc, last_error())
    return out


def combine_bounce_device(rgb_dev: DeviceBuffer, spawn_dev: DeviceBuffer, first_dev: DeviceBuffer, n: int,
                          child_rgb_dev: DeviceBuffer | None, child_w_dev: DeviceBuffer | None, n_children: int,
                          stream: Stream | None = None) -> None:
    """rt_combine_bounce_device: the same in place on the first 3n doubles of
    rgb_dev, on `stream`."""
    if n < 0 or rgb_dev.nbytes < 24 * n or spawn_dev.nbytes < n or first_dev.nbytes < 8 * n or n_children < 0 \
            or (n_children and (child_rgb_dev is None or child_w_dev is None)) \
            or (child_rgb_dev is not None and child_rgb_dev.nbytes < 24 * n_children) \
            or (child_w_dev is not None and child_w_dev.nbytes < 8 * n_children):
        raise ValueError("combine_bounce_device: a buffer is too small")
    opt = lambda b: b.ptr if b is not None else None   # noqa: E731
    rc = amd_lib().rt_combine_bounce_device(rgb_dev.ptr, spawn_dev.ptr, first_dev.ptr, n, opt(child_rgb_dev),
                                            opt(child_w_dev), n_children, stream.handle if stream else None)
    if rc != RT_OK:
        raise RTError(rc, last_error())


def query_radiance_depth(scene: Scene, origins, dirs, depth: int, flags: int = RT_FLAG_NONE,
                         stats: Stats | None = None) -> np.ndarray:
    """rt_query_radiance_depth: Tracer::trace_recursive(Ray(o, d), depth) of
    every ray, as an (n, 3) float64 array."""
    rays = make_rays(origins, dirs)
    n = len(rays)
    rgb = np.zeros((n, 3), dtype=np.float64)
    st = stats if stats is not None else Stats()
    rc = amd_lib().rt_query_radiance_depth(scene.handle, rays.ctypes.data_as(C.c_void_p), n, flags, depth,
                                           rgb.ctypes.data_as(C.c_void_p), C.byref(st))
    if rc != RT_OK:
        raise RTError(rc, last_error())
    return rgb


def query_radiance_depth_device(scene: Scene, rays_dev: DeviceBuffer, n: int, depth: int, rgb_dev: DeviceBuffer,
                                flags: int = RT_FLAG_NONE, stream: Stream | None = None,
                                stats: Stats | None = None) -> None:
    """rt_query_radiance_depth_device: the first n rt_ray records of rays_dev
    into the first 3n doubles of rgb_dev, started at recursion depth `depth`."""
    if n < 0 or rays_dev.nbytes < n * RAY_DTYPE.itemsize or rgb_dev.nbytes < n * 24:
        raise ValueError("query_radiance_depth_device: a buffer is too small for n rays")
    st = stats if stats is not None else Stats()
    rc = amd_lib().rt_query_radiance_depth_device(scene.handle, rays_dev.ptr, n, flags, depth, rgb_dev.ptr,
                                                  stream.handle if stream else None, C.byref(st))
    if rc != RT_OK:
        raise RTError(rc, last_error())


def scatter_launch_items(n: int) -> None:
    """rt_test_scatter_launch_items: parents per launch group of
    scatter_rays_device (0: the default, 2^30)."""
    _ok(amd_lib().rt_test_scatter_launch_items(n), "rt_test_scatter_launch_items")


def radiance_bounces_device(scene: Scene, rays_dev: DeviceBuffer, n: int, flags: int = RT_FLAG_NONE,
                            stream: Stream | None = None, per_level: list | None = None):
    """Tracer::trace of the first n rays of rays_dev as the bounce loop, every
    buffer on the device: per level k query_intersect_device -> rays_wo_device
    -> query_shade_device (the hit mask, miss_rgb None: the background), then
    scatter_rays_device(depth = k) until it spawns nothing, then
    combine_bounce_device from the last level up.  Returns (rgb_dev, the level
    sizes, the summed Stats); the colours equal query_radiance_device's bit for
    bit and the ray counts are its counts.  recursion_limit <= 0: all black
    without a launch.  per_level (optional list): one dict per level with its
    size and each call's ms_kernel / ms_total is appended, and one for the
    unwind."""
    total = Stats()
    total.n_gpus = 1
    rgb0 = DeviceBuffer(max(24 * n, 16))   # (zero-filled)
    if n <= 0 or scene.desc.recursion_limit <= 0:
        return rgb0, [], total

    def add(st: Stats, rec: dict | None, name: str):
        total.rays_intersect += st.rays_intersect
        total.rays_occluded += st.rays_occluded
        total.rays_traced += st.rays_traced
        total.ms_kernel += st.ms_kernel
        total.ms_total += st.ms_total
        if rec is not None:
            rec[name] = {"ms_kernel": st.ms_kernel, "ms_total": st.ms_total}

    import time
    levels = []   # (n, rgb, spawn, first, child_w, m)
    cur, cur_n, rgb, depth = rays_dev, n, rgb0, 0
    while True:
        rec = {"level": depth, "n": cur_n} if per_level is not None else None
        hits, mask, wo = DeviceBuffer(64 * cur_n), DeviceBuffer(max(cur_n, 16)), DeviceBuffer(24 * cur_n)
        st = Stats()
        query_intersect_device(scene, cur, cur_n, hits, mask, flags, stream, st)
        add(st, rec, "intersect")
        t0 = time.perf_counter()
        rays_wo_device(cur, cur_n, wo, stream)
        if rec is not None:
            rec["rays_wo"] = {"ms_total": (time.perf_counter() - t0) * 1e3}
        st = Stats()
        query_shade_device(scene, hits, wo, mask, cur_n, rgb, None, None, flags, stream, st)
        add(st, rec, "shade")
        wo.free()
        spawn, first = DeviceBuffer(max(cur_n, 16)), DeviceBuffer(8 * cur_n)
        child_rays, child_w = DeviceBuffer(128 * cur_n), DeviceBuffer(16 * cur_n)
        st = Stats()
        m = scatter_rays_device(scene, cur, hits, mask, cur_n, depth, spawn, first, child_rays, child_w, 2 * cur_n, stream,
                                st)
        add(st, rec, "scatter")
        hits.free()
        mask.free()
        if rec is not None:
            rec["children"] = m
            per_level.append(rec)
        levels.append((cur_n, rgb, spawn, first, child_w, m))
        if cur is not rays_dev:
            cur.free()
        if m == 0:
            child_rays.free()
            break
        cur, cur_n, depth = child_rays, m, depth + 1
        rgb = DeviceBuffer(24 * cur_n)
    t0 = time.perf_counter()
    for k in range(len(levels) - 2, -1, -1):
        ln, lrgb, spawn, first, child_w, m = levels[k]
        combine_bounce_device(lrgb, spawn, first, ln, levels[k + 1][1], child_w, m, stream)
    dt = (time.perf_counter() - t0) * 1e3
    total.ms_total += dt
    if per_level is not None:
        per_level.append({"unwind": {"ms_total": dt}})
    for k, lv in enumerate(levels):
        for b in lv[2:5]:
            b.free()
        if k:
            lv[1].free()
    return rgb0, [lv[0] for lv in levels], total


def camera_chunk_rays(n: int) -> None:
    """rt_test_camera_chunk_rays: items per staging chunk of the batched calls'
    host forms - rays of camera_rays (whole rows, at least one), rays of
    query_intersect / query_occluded / query_radiance, hits of query_shade
    (0: the default, 2^20)."""
    _ok(amd_lib().rt_test_camera_chunk_rays(n), "rt_test_camera_chunk_rays")


def render_multi(scene: Scene, width: int, height: int, mode: int, n_gpus: int, flags: int = RT_FLAG_NONE,
                 stats: Stats | None = None) -> np.ndarray:
    """rt_render_multi: the frame over n_gpus devices of this process."""
    fb = np.zeros((height, width, 3), dtype=np.float64)
    st = stats if stats is not None else Stats()
    rc = amd_lib().rt_render_multi(scene.handle, width, height, mode, flags, n_gpus, fb.ctypes.data_as(_dp),
                                   C.byref(st))
    if rc != RT_OK:
        raise RTError(rc, last_error())
    return fb


def render_rgb8(scene: Scene, width: int, height: int, mode: int, n_gpus: int = 1, flags: int = RT_FLAG_NONE,
                stats: Stats | None = None) -> np.ndarray:
    """rt_render_rgb8: render + toByte on the device(s), RGB bytes."""
    out = np.zeros((height, width, 3), dtype=np.uint8)
    st = stats if stats is not None else Stats()
    rc = amd_lib().rt_render_rgb8(scene.handle, width, height, mode, flags, n_gpus,
                                  out.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(st))
    if rc != RT_OK:
        raise RTError(rc, last_error())
    return out


def dist_rows(H: int, world: int, rank: int, mode: int = RT_MODE_STANDARD) -> list[int]:
    """rt_dist_rows_mode: the output rows rank renders (interleaved strips of
    RT_STRIP_ROWS, paper mode RT_PAPER_STRIP_ROWS)."""
    buf = (C.c_int32 * max(1, H))()
    n = amd_lib().rt_dist_rows_mode(H, world, rank, mode, buf)
    if n < 0:
        raise RTError(n, "rt_dist_rows: bad arguments")
    return list(buf[:n])


class DistRun(C.Structure):
    """rt_test.h rt_test_dist_run."""
    _fields_ = [("world", C.c_int), ("rgb8", C.c_int), ("frames", C.c_int), ("fault_rank", C.c_int),
                ("fault", C.c_int), ("fault_frame", C.c_int), ("timeout_ms", C.c_int), ("msg_cap", C.c_int),
                ("rc", C.POINTER(C.c_int)), ("ms", _dp), ("msgs", C.c_char_p),
                ("frame_scenes", C.POINTER(C.c_void_p)), ("alt_scene", C.c_void_p), ("split", _dp)]


(FAULT_NONE, FAULT_TRACE, FAULT_SETUP, FAULT_DESC_H, FAULT_DESC_FLAGS, FAULT_ABSENT, FAULT_DESC_SCENE,
 FAULT_DESC_SHED) = range(8)
RANK_ABSENT = 1


def dist_threads(scene: Scene, width: int, height: int, mode: int, world: int, frames: int = 1,
                 fault: int = FAULT_NONE, fault_rank: int = -1, fault_frame: int = 0, timeout_ms: int = 0,
                 rgb8: bool = False, flags: int = RT_FLAG_NONE, frame_scenes=None, alt_scene=None,
                 split_out: np.ndarray | None = None):
    """rt_test_dist_threads: `frames` distributed frames with `world` ranks
    running concurrently on the current device (one host thread, stream set
    and workspace per rank; RCCL replaced by a same-device transport), with an
    optional fault on one rank in one frame.  frame_scenes: one Scene (or
    None = `scene`) per frame, rendered in sequence on the same ranks;
    alt_scene: the scene FAULT_DESC_SCENE gives the faulty rank; split_out:
    float64 [frames, world, 10], filled with each rank's rt_dist_frame_split
    after each successful frame.  Returns (root frames
    [frames, H, W, 3] - zeros where the root's call failed -, rc [frames,
    world], ms [frames, world], messages [frames][world])."""
    lib = amd_lib()
    cap = 512
    rc = np.zeros((frames, world), dtype=np.int32)
    ms = np.zeros((frames, world), dtype=np.float64)
    msgs = C.create_string_buffer(frames * world * cap)
    out = np.zeros((frames, height, width, 3), dtype=np.uint8 if rgb8 else np.float64)
    run = DistRun(world, 1 if rgb8 else 0, frames, fault_rank, fault, fault_frame, timeout_ms, cap,
                  rc.ctypes.data_as(C.POINTER(C.c_int)), ms.ctypes.data_as(_dp), C.cast(msgs, C.c_char_p))
    keep = []
    if frame_scenes is not None:
        assert len(frame_scenes) == frames
        arr = (C.c_void_p * frames)(*[(x.handle.value if x is not None else None) for x in frame_scenes])
        keep.append(arr)
        run.frame_scenes = C.cast(arr, C.POINTER(C.c_void_p))
    if alt_scene is not None:
        run.alt_scene = alt_scene.handle.value
    if split_out is not None:
        assert split_out.shape == (frames, world, 10) and split_out.dtype == np.float64 and split_out.flags.c_contiguous
        run.split = split_out.ctypes.data_as(_dp)
    if rgb8:
        r = lib.rt_test_dist_threads(scene.handle, width, height, mode, flags, C.byref(run), None,
                                     out.ctypes.data_as(C.POINTER(C.c_uint8)))
    else:
        r = lib.rt_test_dist_threads(scene.handle, width, height, mode, flags, C.byref(run),
                                     out.ctypes.data_as(_dp), None)
    if r != RT_OK:
        raise RTError(r, last_error())
    raw = msgs.raw
    text = [[raw[(f * world + k) * cap:(f * world + k + 1) * cap].split(b"\0", 1)[0].decode("utf-8", "replace")
             for k in range(world)] for f in range(frames)]
    return out, rc, ms, text


def render_dist_sim(scene: Scene, width: int, height: int, mode: int, world: int, rgb8: bool = False,
                    flags: int = RT_FLAG_NONE) -> np.ndarray:
    """rt_test_render_dist_sim: one distributed frame with `world` ranks
    running concurrently on the current device (rt_test_dist_threads)."""
    lib = amd_lib()
    if rgb8:
        out = np.zeros((height, width, 3), dtype=np.uint8)
        rc = lib.rt_test_render_dist_sim(scene.handle, width, height, mode, flags, world, 1, None,
                                         out.ctypes.data_as(C.POINTER(C.c_uint8)))
    else:
        out = np.zeros((height, width, 3), dtype=np.float64)
        rc = lib.rt_test_render_dist_sim(scene.handle, width, height, mode, flags, world, 0, out.ctypes.data_as(_dp),
                                         None)
    if rc != RT_OK:
        raise RTError(rc, last_error())
    return out


def oracle_render(scene: Scene, width: int, height: int, mode: int, row0: int = 0, row1: int | None = None,
                  threads: int = 1):
    """CPU oracle restricted to output rows [row0,row1).  TEST ONLY."""
    if row1 is None:
        row1 = height
    fb = np.zeros((row1 - row0, width, 3), dtype=np.float64)
    st = OracleStats()
    rc = oracle_lib().oracle_render_rows(scene.desc_ptr, width, height, mode, row0, row1, fb.ctypes.data_as(_dp),
                                         C.byref(st), threads)
    if rc != 0:
        raise RuntimeError("oracle_render_rows failed")
    return fb, st


def oracle_trace(scene: Scene, origins, dirs):
    """Tracer::trace(Ray(o, d)) of every ray through the oracle: (rgb (n, 3),
    n_intersect (n,), n_occluded (n,)), the colour and the Scene::intersect /
    Scene::occluded calls of each ray.  TEST ONLY.

    Per ray, a 1x1 standard frame of a copy of the scene whose camera has eye
    = o, P = o + d and a zero-size screen: generate_ray_subpixel then maps
    every jitter draw to P (camera.h:68-78), so the frame is the mean of 8
    evaluations of Tracer::trace(Ray(o, P - o)) and its ray counts are 8x the
    ray's own.  The ray the oracle traces is therefore (o + d) - o as rounded
    in float64: hand the GPU oracle_trace_dirs(origins, dirs)."""
    lib = oracle_lib()
    o = np.asarray(origins, dtype=np.float64)
    d = np.asarray(dirs, dtype=np.float64)
    if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
        raise ValueError(f"origins and dirs must both be (n, 3) arrays, got {o.shape} and {d.shape}")
    n = len(o)
    P = o + d
    desc = SceneDesc.from_buffer_copy(scene.desc)   # (shares the scene's arrays: keep `scene` alive)
    desc.camera.Lx = desc.camera.Ly = 0.0
    desc.camera.dpi = 1
    rgb, ni, no = np.zeros((n, 3)), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    px = np.zeros(3)
    pp, st = px.ctypes.data_as(_dp), OracleStats()
    for k in range(n):
        desc.camera.eye[:] = o[k].tolist()
        desc.camera.P[:] = P[k].tolist()
        if lib.oracle_render_rows(C.byref(desc), 1, 1, RT_MODE_STANDARD, 0, 1, pp, C.byref(st), 1) != 0:
            raise RuntimeError("oracle_render_rows failed")
        assert st.rays_intersect % 8 == 0 and st.rays_occluded % 8 == 0, (k, st.rays_intersect, st.rays_occluded)
        rgb[k], ni[k], no[k] = px, st.rays_intersect // 8, st.rays_occluded // 8
    return rgb, ni, no


def oracle_frame_rays(scene: Scene):
    """The standard frame's own 8 W H jittered rays (tracer.cpp:284-293:
    oracle_jitter + Camera::generate_ray_subpixel through the oracle) in frame
    order: (origins, dirs), each (H, W, 8, 3), output row first, samples in
    the order the frame sums them.  TEST ONLY."""
    lib = oracle_lib()
    W, H = scene.width, scene.height
    jit = np.zeros(16 * W * H)
    lib.oracle_jitter(0, len(jit), jit.ctypes.data_as(_dp))
    jit = jit.reshape(H, W, 8, 2)   # (loop row, x, sample, dx / dy)
    o, d = np.zeros((H, W, 8, 3)), np.zeros((H, W, 8, 3))
    o3, d3 = (C.c_double * 3)(), (C.c_double * 3)()
    desc = scene.desc_ptr
    for y in range(H):   # loop row y is output row H - 1 - y (tracer.cpp:297)
        for x in range(W):
            for s in range(8):
                lib.oracle_camera_ray(desc, x, y, jit[y, x, s, 0], jit[y, x, s, 1], 1, o3, d3)
                o[H - 1 - y, x, s], d[H - 1 - y, x, s] = tuple(o3), tuple(d3)
    return o, d


def oracle_trace_dirs(origins, dirs) -> np.ndarray:
    """The directions oracle_trace really traces: (o + d) - o in float64."""
    o = np.asarray(origins, dtype=np.float64)
    return (o + np.asarray(dirs, dtype=np.float64)) - o


def oracle_shade(scene: Scene, hits, wo, lights=None):
    """shade_lambert_phong(scene, hit, wo) of every hit: (rgb (n, 3),
    n_occluded (n,)), the colour and the Scene::occluded calls of each.  TEST
    ONLY.  A numpy restatement of shading.cpp:31-138, statement by statement
    in float64, whose Scene::occluded is answered by oracle_occluded (the
    pinned oracle); what oracle_trace cannot do: a wo that is not -d, a hit
    point that is not a ray's.  hits: a HIT_DTYPE array (t, p, n, mat; a mat
    outside [0, n_materials) is a null material: magenta, no query); lights:
    None = the scene's point lights, else [(pos, intensity), ...] instead.
    std::max(a, b) is a < b ? b : a and std::min(a, b) is b < a ? b : a, which
    is what decides for a NaN; tests/test_shade_plan.py holds the restatement
    to the oracle's own shading."""
    hits = np.asarray(hits, dtype=HIT_DTYPE)
    wo_all = np.asarray(wo, dtype=np.float64)
    n_all = len(hits)
    d = scene.desc
    rgb = np.empty((n_all, 3))
    rgb[:] = (1.0, 0.0, 1.0)   # shading.cpp:33
    n_occ = np.zeros(n_all, dtype=np.int64)
    idx = np.flatnonzero((hits["mat"] >= 0) & (hits["mat"] < d.n_materials))
    if not len(idx):
        return rgb, n_occ
    mats = [d.materials[i] for i in range(d.n_materials)]
    field = lambda f: np.array([getattr(m, f) for m in mats])[hits["mat"][idx]]   # noqa: E731
    albedo = np.array([list(m.albedo) for m in mats])[hits["mat"][idx]]
    ambient = np.array([list(m.ambient) for m in mats])[hits["mat"][idx]]
    kd, ks, shin = field("kd"), field("ks"), field("shininess")
    p, n, t, wo = hits["p"][idx], hits["n"][idx], hits["t"][idx], wo_all[idx]
    if lights is None:
        lights = [(list(d.lights[i].pos), list(d.lights[i].intensity)) for i in range(d.n_lights)]
    smax = lambda a, b: np.where(a < b, b, a)   # noqa: E731  (std::max)
    dot = lambda a, b: a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]   # noqa: E731

    def normalized(v):   # core.h:95-101
        L = np.sqrt(dot(v, v))
        return np.where((L > 1e-6)[:, None], v / L[:, None], np.array([0.0, 1.0, 0.0]))

    def combine(a, b):
        return 1.0 - (1.0 - a) * (1.0 - b)

    def occluded(need, wi, tmax):
        occ = np.zeros(len(idx), dtype=bool)
        k = np.flatnonzero(need)
        if len(k):
            occ[k] = oracle_occluded(scene, so[k], wi[k], eps[k], tmax[k])
            n_occ[idx[k]] += 1
        return occ

    def light_term(lit, E, wi, ndotl, I, diffuse_scale):
        E_d = albedo * I * (kd * ndotl * diffuse_scale if diffuse_scale is not None else kd * ndotl)[:, None]
        ndw = dot(n, wi)
        r = normalized((2.0 * ndw)[:, None] * n - wi)
        rdotv = smax(0.0, dot(r, wo))
        spec = np.power(rdotv, shin) * ks
        E_s = np.where((ks > 0.0)[:, None], I * spec[:, None], 0.0)
        return np.where(lit[:, None], combine(E, combine(E_d, E_s)), E)

    with np.errstate(all="ignore"):
        E = ambient * np.array(list(d.ambient))
        eps = smax(1e-3, 1e-4 * t)
        so = p + n * eps[:, None]
        inf = np.full(len(idx), np.inf)
        for li in range(d.n_dir_lights):
            L = d.dir_lights[li]
            wi = normalized(np.tile(-np.array(list(L.dir)), (len(idx), 1)))
            ndotl = smax(0.0, dot(n, wi))
            need = ~(ndotl <= 0.0)
            lit = need & ~occluded(need, wi, inf)
            E = light_term(lit, E, wi, ndotl, np.tile(np.array(list(L.radiance)), (len(idx), 1)), None)
        for pos, inten in lights:
            tl = np.array([float(v) for v in pos]) - p
            d2 = dot(tl, tl)
            d2 = np.where(d2 <= 0.01, 0.01, d2)
            dist = np.sqrt(d2)
            wi = tl / dist[:, None]
            ndotl = smax(0.0, dot(n, wi))
            max_t = dist - eps
            need = ~(ndotl <= 0.0) & ~(max_t <= eps)
            lit = need & ~occluded(need, wi, max_t)
            ed = smax(0.5, dist)
            falloff = 1.0 / (ed * ed)
            I = np.array([float(v) for v in inten]) * (falloff * 2.0)[:, None]
            E = light_term(lit, E, wi, ndotl, I, 1.5)
        rgb[idx] = np.where(E < 1.5, E, 1.5)   # std::min(1.5, E)
    return rgb, n_occ


def oracle_shade_hits(scene: Scene, hits, wo, mask=None, lights=None, miss_rgb=None):
    """oracle_shade_hits (oracle/oracle.h): the oracle's own shade() of every
    hit, with query_shade's arguments: (rgb (n, 3), n_occluded (n,)).  Entries
    with mask 0 are not shaded: miss_rgb (None: the scene's background) and no
    Scene::occluded call.  What oracle_shade restates in numpy, in the C the
    frames are held to, so it can judge bits (and follows oracle_pow).  TEST ONLY."""
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    n = len(hits)
    w = np.ascontiguousarray(wo, dtype=np.float64)
    if w.shape != (n, 3):
        raise ValueError(f"wo must be an (n, 3) array for n = {n} hits, got {w.shape}")
    arr, nl = _light_array(lights)
    rgb, no = np.zeros((n, 3)), np.zeros(n, dtype=np.uint64)
    rc = _oracle_pow_lib().oracle_shade_hits(scene.desc_ptr, n, hits.ctypes.data_as(C.c_void_p), w.ctypes.data_as(_dp),
                                        C.cast(arr, C.c_void_p) if arr is not None else None, nl,
                                        rgb.ctypes.data_as(_dp), no.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise RuntimeError("oracle_shade_hits failed")
    no = no.astype(np.int64)
    if mask is not None:
        off = np.asarray(mask).reshape(n) == 0
        rgb[off] = list(scene.desc.background) if miss_rgb is None else [float(v) for v in miss_rgb]
        no[off] = 0
    return rgb, no


def oracle_paper_resolve(hits, mask, rgb, W: int, H: int, row0: int, n_rows: int):
    """(fb (n_rows, W, 3), edge (n_rows, W)) of paper_resolve's inputs: a
    vectorised numpy restatement of Tracer::get_edge_strength, get_luminance,
    apply_crosshatch (tracer.cpp:123-205) and the pixel of tracer.cpp:264-279
    over stored records, statement by statement in float64.  TEST ONLY.
    std::max(a, b) is a < b ? b : a and std::min(a, b) is b < a ? b : a; '%'
    truncates toward zero (np.fmod on integers)."""
    in0, in1 = max(0, row0 - 1), min(H, row0 + n_rows + 1)
    hits = np.asarray(hits, dtype=HIT_DTYPE).reshape(in1 - in0, W)
    rgb = np.asarray(rgb, dtype=np.float64).reshape(in1 - in0, W, 3)
    hit = np.ones((in1 - in0, W), dtype=bool) if mask is None else np.asarray(mask).reshape(in1 - in0, W) != 0
    smax = lambda a, b: np.where(a < b, b, a)   # noqa: E731
    smin = lambda a, b: np.where(b < a, b, a)   # noqa: E731
    ys, xs = np.meshgrid(np.arange(row0, row0 + n_rows), np.arange(W), indexing="ij")
    at = lambda a, y, x: a[y - in0, x]   # noqa: E731
    ch, ct, cn, cm = at(hit, ys, xs), at(hits["t"], ys, xs), at(hits["n"], ys, xs), at(hits["mat"], ys, xs)
    max_edge = np.zeros((n_rows, W))
    valid = np.zeros((n_rows, W), dtype=np.int64)
    with np.errstate(all="ignore"):
        for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            nx, ny = xs + dx, ys + dy
            ok = ~((nx < 0) | (nx >= W) | (ny < 0) | (ny >= H))   # tracer.cpp:151
            nx, ny = np.where(ok, nx, xs), np.where(ok, ny, ys)
            valid += ok
            nh, nt, nn, nm = at(hit, ny, nx), at(hits["t"], ny, nx), at(hits["n"], ny, nx), at(hits["mat"], ny, nx)
            differ = ok & (ch != nh)
            max_edge = np.where(differ, smax(max_edge, 0.9), max_edge)
            both = ok & ~differ & ch & nh
            min_d, max_d = smin(ct, nt), smax(ct, nt)
            depth = both & (min_d > 1e-4) & (max_d / min_d > 3.0)
            max_edge = np.where(depth, smax(max_edge, 0.6), max_edge)
            nd = cn[..., 0] * nn[..., 0] + cn[..., 1] * nn[..., 1] + cn[..., 2] * nn[..., 2]
            max_edge = np.where(both & (nd < 0.2), smax(max_edge, 0.5), max_edge)
            max_edge = np.where(both & (cm != nm) & (nd < 0.7), smax(max_edge, 0.3), max_edge)
        edge = np.where(valid < 4, max_edge * 0.5, max_edge)
        base = at(rgb, ys, xs)
        lum = 0.299 * base[..., 0] + 0.587 * base[..., 1] + 0.114 * base[..., 2]
        darkness = 1.0 - lum
        diag1 = np.fmod(xs + ys, 4) < 1
        diag2 = np.fmod(xs - ys, 4) < 1
        horizontal = np.fmod(ys, 4) < 1
        draw = np.select(
            [darkness > 0.8, darkness > 0.65, darkness > 0.5, darkness > 0.35, darkness > 0.2, darkness > 0.12],
            [(diag1 & diag2) | horizontal, (diag1 & diag2) | (horizontal & (np.fmod(xs + ys, 3) == 0)),
             (diag1 & diag2) | (horizontal & (np.fmod(xs + ys, 4) == 0)), diag1 | (horizontal & (np.fmod(xs + ys, 3) == 0)),
             diag1, diag1 & (np.fmod(xs + ys, 8) < 2)], False)
        hatch = np.where(lum < 0.15, 0.0, np.where(draw, 0.0, 1.0))
        out = np.where(edge > 0.3, hatch * (1.0 - (edge - 0.3) * 0.4), hatch)
        out = np.where(edge > 0.8, 0.0, np.where(edge > 0.5, 0.2, out))
    return np.repeat(out[..., None], 3, axis=2), edge


def oracle_scatter(scene: Scene, rays, hits, mask=None, depth: int = 0):
    """scatter_rays' result from a vectorised numpy restatement of the spawn
    half of Tracer::trace_recursive (tracer.cpp:34-67, reflect / refract /
    has_total_internal_reflection :76-104, Ray::Ray and Dir3::normalized of
    core.h), statement by statement in float64: (spawn, first, child_rays,
    child_w).  std::max(0.0, x) is x if 0.0 < x else 0.0.  TEST ONLY."""
    rays = np.asarray(rays, dtype=RAY_DTYPE)
    hits = np.asarray(hits, dtype=HIT_DTYPE)
    n = len(rays)
    d = scene.desc
    nm = int(d.n_materials)
    mats = np.array([[d.materials[i].kr, d.materials[i].kt, d.materials[i].refractive_index] for i in range(nm)],
                    dtype=np.float64).reshape(nm, 3)
    on = np.ones(n, dtype=bool) if mask is None else np.asarray(mask).reshape(n) != 0
    mat = hits["mat"].astype(np.int64)
    on &= (mat >= 0) & (mat < nm)
    mi = np.where(on, mat, 0)
    if nm:
        kr, kt, ri = mats[mi, 0], mats[mi, 1], mats[mi, 2]
    else:
        kr = kt = ri = np.zeros(n)
    can = int(depth) < int(d.recursion_limit) - 1
    medium = float(d.medium_index)

    def normalized(v):   # core.h:95-101
        L = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
        return np.where((L > 1e-6)[:, None], v / L[:, None], np.array([0.0, 1.0, 0.0]))

    with np.errstate(all="ignore"):
        rd = normalized(rays["d"].astype(np.float64))   # Ray::Ray (core.h:278)
        inc = normalized(rd)                       # r.d.normalized()
        nn, p, ff = hits["n"], hits["p"], hits["front_face"] != 0
        idn = inc[:, 0] * nn[:, 0] + inc[:, 1] * nn[:, 1] + inc[:, 2] * nn[:, 2]
        refl = on & (kr > 0.0) & can
        k = 2.0 * idn
        refl_dir = normalized(inc - nn * k[:, None])
        above, below = p + nn * 1e-6, p - nn * 1e-6
        refl_o = np.where(ff[:, None], above, below)
        eta = np.where(ff, medium / ri, ri / medium)
        cos_i = -idn
        one_m = 1.0 - cos_i * cos_i
        sin_t2 = eta * eta * np.where(0.0 < one_m, one_m, 0.0)
        tir = sin_t2 >= 1.0
        refr = on & (kt > 0.0) & can & ~tir
        cos_t = np.sqrt(1.0 - sin_t2)
        kk = eta * cos_i - cos_t
        refr_dir = normalized(inc * eta[:, None] + nn * kk[:, None])
        refr_o = np.where(ff[:, None], below, above)
    spawn = (refl * RT_SPAWN_REFLECT + refr * RT_SPAWN_REFRACT).astype(np.uint8)
    cnt = refl.astype(np.uint64) + refr.astype(np.uint64)
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.uint64) if n else np.zeros(0, dtype=np.uint64)
    m = int(cnt.sum())
    child = np.zeros(m, dtype=RAY_DTYPE)
    w = np.zeros(m)
    child["tmin"], child["tmax"] = 1e-4, np.inf
    j1 = first[refl].astype(np.int64)
    child["o"][j1], child["d"][j1], w[j1] = refl_o[refl], refl_dir[refl], kr[refl]
    j2 = (first[refr] + refl[refr]).astype(np.int64)
    child["o"][j2], child["d"][j2], w[j2] = refr_o[refr], refr_dir[refr], kt[refr]
    return spawn, first, child, w


def oracle_combine_bounce(rgb, spawn, first, child_rgb, child_w) -> np.ndarray:
    """combine_bounce's result from a numpy restatement of tracer.cpp:47, :66
    with combine and scale of shading.cpp:6-22: per channel 1.0 - (1.0 - a) *
    (1.0 - c * w); a child index past the children is skipped.  TEST ONLY."""
    out = np.array(rgb, dtype=np.float64, copy=True).reshape(-1, 3)
    spawn = np.asarray(spawn, dtype=np.uint8)
    first = np.asarray(first, dtype=np.uint64)
    crgb = np.asarray(child_rgb, dtype=np.float64).reshape(-1, 3)
    cw = np.asarray(child_w, dtype=np.float64).reshape(-1)
    m = len(cw)
    with np.errstate(all="ignore"):
        for bit in (1, 2):
            j = first + (spawn & 1).astype(np.uint64) if bit == 2 else first   # (wraps mod 2^64, as the C does)
            sel = ((spawn & bit) != 0) & (j < np.uint64(m))
            js = j[sel].astype(np.int64)
            e = crgb[js] * cw[js][:, None]
            out[sel] = 1.0 - (1.0 - out[sel]) * (1.0 - e)
    return out


def oracle_radiance_bounces(scene: Scene, rays, scatter=None, combine=None, peel_first: bool = False):
    """Tracer::trace of an rt_ray array as the bounce loop on the CPU: per
    level oracle_scene_intersect -> rays_wo -> oracle_shade_hits, then
    `scatter` (default: the host form scatter_rays; signature (scene, rays,
    hits, mask, depth)), then `combine` (default: combine_bounce) from the last
    level up.  Returns (rgb (n, 3), level sizes, Scene::intersect calls,
    Scene::occluded calls).  peel_first: only level 0 is looped; its children
    are traced by oracle_trace_rays on a copy of the scene with recursion_limit
    - 1 (Tracer::trace_recursive(child, 1)).  TEST ONLY."""
    scatter = scatter or (lambda sc, r, h, m, depth: scatter_rays(sc, r, h, m, depth))
    combine = combine or combine_bounce
    rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE).reshape(-1)
    n = len(rays)
    limit = int(scene.desc.recursion_limit)
    if limit <= 0 or n == 0:
        return np.zeros((n, 3)), [], 0, 0
    levels, n_isect, n_occl, depth = [], 0, 0, 0
    while True:
        ok, hits = oracle_scene_intersect(scene, rays)
        n_isect += len(rays)
        rgb, no = oracle_shade_hits(scene, hits, rays_wo(rays), ok.astype(np.uint8))
        n_occl += int(no.sum())
        spawn, first, child, w = scatter(scene, rays, hits, ok.astype(np.uint8), depth)
        levels.append([len(rays), rgb, spawn, first, w])
        if len(child) == 0:
            break
        if peel_first:
            sub = with_recursion_limit(scene, limit - 1)
            crgb, ni, no = oracle_trace_rays(sub, child["o"], child["d"])
            n_isect += int(ni.sum())
            n_occl += int(no.sum())
            levels.append([len(child), crgb, None, None, None])
            break
        rays, depth = child, depth + 1
    for k in range(len(levels) - 2, -1, -1):
        ln, rgb, spawn, first, w = levels[k]
        levels[k][1] = combine(rgb, spawn, first, levels[k + 1][1], w)
    return levels[0][1], [lv[0] for lv in levels], n_isect, n_occl


def oracle_primary_hits(scene: Scene, W: int | None = None, H: int | None = None) -> np.ndarray:
    """The pixel-centre primary hits of the frame (Camera::generate_ray +
    Scene::intersect(r, 1e-4, inf) through the oracle), one record per pixel:
    hit (bool), d (the ray direction) and the Hit fields.  W x H: the frame
    (None: the camera's own size).  TEST ONLY."""
    lib = oracle_lib()
    W, H = scene.width if W is None else W, scene.height if H is None else H
    dirs = np.zeros((W * H, 3))
    hits = np.zeros(W * H, dtype=HIT_DTYPE)
    ok = np.zeros(W * H, dtype=np.uint8)
    lib.oracle_primary_hits.argtypes = [C.POINTER(SceneDesc), C.c_int, C.c_int, _dp, C.c_void_p, C.c_void_p]
    lib.oracle_primary_hits(scene.desc_ptr, W, H, dirs.ctypes.data_as(_dp), hits.ctypes.data_as(C.c_void_p),
                            ok.ctypes.data_as(C.c_void_p))
    rec = np.zeros(W * H, dtype=[("hit", "?"), ("d", "<f8", (3,)), ("t", "<f8"), ("p", "<f8", (3,)),
                                 ("n", "<f8", (3,)), ("mat", "<i4"), ("front_face", "<i4")])
    rec["hit"], rec["d"] = ok.astype(bool), dirs
    for f in ("t", "p", "n", "mat", "front_face"):
        rec[f] = hits[f]
    return rec


def oracle_node_intersect(scene: Scene, node: int, origins, dirs, tmin=1e-4, tmax=np.inf):
    """oracle_node_intersect (oracle/oracle.h) ray by ray: (hit flags, rt_hit
    records; a miss: mat -1 and zeros, as the device reports one)."""
    rays = make_rays(origins, dirs, tmin, tmax)
    lib, desc = oracle_lib(), scene.desc_ptr
    hit = np.zeros(len(rays), dtype=bool)
    rec = np.zeros(len(rays), dtype=HIT_DTYPE)
    rec["mat"] = -1
    h = OracleHit()
    for k, r in enumerate(rays):
        o, d = np.ascontiguousarray(r["o"]), np.ascontiguousarray(r["d"])
        hit[k] = bool(lib.oracle_node_intersect(desc, node, o.ctypes.data_as(_dp), d.ctypes.data_as(_dp),
                                                float(r["tmin"]), float(r["tmax"]), C.byref(h)))
        if hit[k]:
            rec[k] = (h.t, tuple(h.p), tuple(h.n), h.mat, h.front_face)
    return hit, rec


def oracle_node_interval(scene: Scene, node: int, origins, dirs):
    """oracle_node_interval ray by ray: (enter, exit, ok) as query_node_interval
    returns them (t = tEnter / tExit, the out-parameters, not the records' own
    Hit::t; zeros with mat -1 where ok is False)."""
    rays = make_rays(origins, dirs)
    lib, desc = oracle_lib(), scene.desc_ptr
    ok = np.zeros(len(rays), dtype=bool)
    enter, ex = np.zeros(len(rays), dtype=HIT_DTYPE), np.zeros(len(rays), dtype=HIT_DTYPE)
    enter["mat"] = ex["mat"] = -1
    h0, h1 = OracleHit(), OracleHit()
    t0, t1 = C.c_double(), C.c_double()
    for k, r in enumerate(rays):
        o, d = np.ascontiguousarray(r["o"]), np.ascontiguousarray(r["d"])
        ok[k] = bool(lib.oracle_node_interval(desc, node, o.ctypes.data_as(_dp), d.ctypes.data_as(_dp), C.byref(t0),
                                              C.byref(t1), C.byref(h0), C.byref(h1)))
        if ok[k]:
            enter[k] = (t0.value, tuple(h0.p), tuple(h0.n), h0.mat, h0.front_face)
            ex[k] = (t1.value, tuple(h1.p), tuple(h1.n), h1.mat, h1.front_face)
    return enter, ex, ok


def oracle_occluded(scene: Scene, origins, dirs, tmin, tmax) -> np.ndarray:
    """Scene::occluded of every ray through the oracle, as bools.  TEST ONLY."""
    lib = oracle_lib()
    o = np.ascontiguousarray(origins, dtype=np.float64)
    d = np.ascontiguousarray(dirs, dtype=np.float64)
    n = len(o)
    t0 = np.ascontiguousarray(np.broadcast_to(np.asarray(tmin, dtype=np.float64), (n,)))
    t1 = np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, dtype=np.float64), (n,)))
    out = np.zeros(n, dtype=np.uint8)
    lib.oracle_scene_occluded_batch.argtypes = [C.POINTER(SceneDesc), C.c_int, _dp, _dp, _dp, _dp, C.c_void_p]
    lib.oracle_scene_occluded_batch(scene.desc_ptr, n, o.ctypes.data_as(_dp), d.ctypes.data_as(_dp),
                                    t0.ctypes.data_as(_dp), t1.ctypes.data_as(_dp), out.ctypes.data_as(C.c_void_p))
    return out.astype(bool)


def ref_render(scene: Scene, width: int, height: int, mode: int):
    """The reference's own Tracer::render (oracle/_ref, container only)."""
    fb = np.zeros((height, width, 3), dtype=np.float64)
    ni, no = C.c_uint64(), C.c_uint64()
    ref_lib().ref_render(scene.desc_ptr, width, height, mode, fb.ctypes.data_as(_dp), C.byref(ni), C.byref(no))
    return fb, int(ni.value), int(no.value)


def _ray_args(rays):
    rays = np.asarray(rays, dtype=RAY_DTYPE)
    cols = [np.ascontiguousarray(rays[f], dtype=np.float64) for f in ("o", "d", "tmin", "tmax")]
    return len(rays), cols, [c.ctypes.data_as(_dp) for c in cols]


def _hits_of(ok, hits):
    rec = np.zeros(len(ok), dtype=HIT_DTYPE)
    for k in np.flatnonzero(ok):
        h = hits[k]
        rec[k] = (h.t, tuple(h.p), tuple(h.n), h.mat, h.front_face)
    return ok.astype(bool), rec


def ref_scene_intersect(scene: Scene, rays):
    """The reference's own Scene::intersect of an rt_ray array (oracle/_ref,
    container only): (hit flags, HIT_DTYPE records; a miss is zeros)."""
    lib = ref_lib()
    n, _keep, (o, d, t0, t1) = _ray_args(rays)
    ok, hits = (C.c_int * n)(), (OracleHit * n)()
    lib.ref_scene_intersect_batch.argtypes = [C.POINTER(SceneDesc), C.c_int, _dp, _dp, _dp, _dp, C.POINTER(C.c_int),
                                              C.POINTER(OracleHit)]
    lib.ref_scene_intersect_batch(scene.desc_ptr, n, o, d, t0, t1, ok, hits)
    return _hits_of(np.array(ok[:], dtype=np.int32), hits)


def ref_scene_occluded(scene: Scene, rays) -> np.ndarray:
    """The reference's own Scene::occluded of an rt_ray array, as bools (container only)."""
    lib = ref_lib()
    n, _keep, (o, d, t0, t1) = _ray_args(rays)
    ok = (C.c_int * n)()
    lib.ref_scene_occluded_batch.argtypes = [C.POINTER(SceneDesc), C.c_int, _dp, _dp, _dp, _dp, C.POINTER(C.c_int)]
    lib.ref_scene_occluded_batch(scene.desc_ptr, n, o, d, t0, t1, ok)
    return np.array(ok[:], dtype=np.int32).astype(bool)


def oracle_scene_intersect(scene: Scene, rays):
    """Scene::intersect of an rt_ray array through the oracle: (hit flags,
    HIT_DTYPE records; a miss is zeros).  TEST ONLY."""
    lib = oracle_lib()
    n, (o, d, t0, t1), _ptrs = _ray_args(rays)
    ok, hits = np.zeros(n, dtype=np.int32), (OracleHit * n)()
    for k in range(n):
        ok[k] = lib.oracle_scene_intersect(scene.desc_ptr, o[k].ctypes.data_as(_dp), d[k].ctypes.data_as(_dp),
                                           float(t0[k]), float(t1[k]), C.byref(hits[k]))
    return _hits_of(ok, hits)


def _trace_rays(lib, fn, scene: Scene, origins, dirs):
    o = np.ascontiguousarray(origins, dtype=np.float64)
    d = np.ascontiguousarray(dirs, dtype=np.float64)
    if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
        raise ValueError(f"origins and dirs must both be (n, 3) arrays, got {o.shape} and {d.shape}")
    n = len(o)
    rgb, ni, no = np.zeros((n, 3)), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    f = getattr(lib, fn)
    f.argtypes = [C.POINTER(SceneDesc), C.c_int, _dp, _dp, _dp, C.c_void_p, C.c_void_p]
    f(scene.desc_ptr, n, o.ctypes.data_as(_dp), d.ctypes.data_as(_dp), rgb.ctypes.data_as(_dp),
      ni.ctypes.data_as(C.c_void_p), no.ctypes.data_as(C.c_void_p))
    return rgb, ni.astype(np.int64), no.astype(np.int64)


def oracle_trace_rays(scene: Scene, origins, dirs):
    """Tracer::trace(Ray(o, d)) of every ray through the oracle, the ray built
    once by the Ray constructor: (rgb (n, 3), n_intersect (n,), n_occluded
    (n,)).  What oracle_trace gives for finite rays (up to its mean of 8 equal
    samples), and the reference's answer where a component is not finite:
    oracle_trace's ray passes through the camera and is normalised twice,
    which turns an infinite direction into (0, 1, 0).  TEST ONLY."""
    return _trace_rays(oracle_lib(), "oracle_trace_rays", scene, origins, dirs)


def ref_trace(scene: Scene, origins, dirs):
    """The reference's own Tracer::trace(Ray(o, d)) of every ray (oracle/_ref, container only)."""
    return _trace_rays(ref_lib(), "ref_trace_batch", scene, origins, dirs)


def ref_shade(scene: Scene, hits, wo):
    """The reference's own shade_lambert_phong of every hit (a HIT_DTYPE array)
    and view direction: (rgb (n, 3), n_occluded (n,)) (oracle/_ref, container only)."""
    lib = ref_lib()
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    w = np.ascontiguousarray(wo, dtype=np.float64)
    n = len(hits)
    rgb, no = np.zeros((n, 3)), np.zeros(n, dtype=np.uint64)
    lib.ref_shade_batch.argtypes = [C.POINTER(SceneDesc), C.c_int, C.c_void_p, _dp, _dp, C.c_void_p]
    lib.ref_shade_batch(scene.desc_ptr, n, hits.ctypes.data_as(C.c_void_p), w.ctypes.data_as(_dp),
                        rgb.ctypes.data_as(_dp), no.ctypes.data_as(C.c_void_p))
    return rgb, no.astype(np.int64)


def to_rgb8(fb: np.ndarray) -> np.ndarray:
    fb = np.ascontiguousarray(fb, dtype=np.float64)
    out = np.zeros(fb.shape, dtype=np.uint8)
    host_lib().rt_framebuffer_to_rgb8(fb.ctypes.data_as(_dp), fb.size // 3, out.ctypes.data_as(C.POINTER(C.c_uint8)))
    return out


def write_png(path: str, rgb8: np.ndarray, threads: int = 1) -> None:
    rgb8 = np.ascontiguousarray(rgb8, dtype=np.uint8)
    h, w = rgb8.shape[:2]
    rc = host_lib().rt_write_png(path.encode(), rgb8.ctypes.data_as(C.POINTER(C.c_uint8)), w, h, threads)
    if rc != RT_OK:
        raise RTError(rc, f"rt_write_png failed ({rc})")
