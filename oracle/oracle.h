/*
 * oracle.h — CPU restatement of the reference ray-trace path.
 *
 * TEST INFRASTRUCTURE ONLY.  Only tests/, __graft_entry__.smoke() and the
 * cpu_baseline leg of bench.py may load liboracle.so.  The product path
 * (librtamd.so, the `ray` CLI) never links or calls it.
 *
 * Pinning: oracle/_ref/ is the reference's own hot path
 * (raytracer/src/{tracer,shading,scene,geometry,csg,transform}.cpp) compiled
 * from /root/reference by oracle/Makefile with our harness
 * oracle/ref_harness.cpp; tests/golden/ holds framebuffers, ray counts and
 * per-primitive KAT vectors produced by it (script: tests/golden/make_golden.py).
 * The oracle is checked bit-for-bit against those fixtures.
 */
#ifndef RT_ORACLE_H
#define RT_ORACLE_H

#include <stdint.h>

#include "rt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct oracle_stats {
    uint64_t rays_intersect;   /* Scene::intersect calls (scene.cpp:10) */
    uint64_t rays_occluded;    /* Scene::occluded calls  (scene.cpp:33) */
    uint64_t ops[16];          /* rt_op_counter */
} oracle_stats;

typedef struct oracle_hit {    /* geometry.h:25-46 Hit */
    double t;
    double p[3];
    double n[3];
    int32_t mat;               /* material index, -1 = nullptr */
    int32_t front_face;
} oracle_hit;

/* Tracer::render restricted to OUTPUT rows [row0,row1) (top row first).
 * fb receives (row1-row0)*W*3 doubles.  n_threads>1 splits the rows into
 * bands; each band fast-forwards its own mt19937 to the band's first word. */
int oracle_render_rows(const rt_scene_desc* d, int W, int H, int mode, int row0, int row1,
                       double* fb, oracle_stats* st, int n_threads);

/* Primitive-level queries (Primitive::intersect / ::interval) on node `node`.
 * The ray is built as Ray(o, d) (direction normalised, core.h:278). */
int oracle_node_intersect(const rt_scene_desc* d, int node, const double o[3], const double dir[3],
                          double tmin, double tmax, oracle_hit* out);
int oracle_node_interval(const rt_scene_desc* d, int node, const double o[3], const double dir[3],
                         double* t0, double* t1, oracle_hit* h0, oracle_hit* h1);

/* Scene-level queries. */
int oracle_scene_intersect(const rt_scene_desc* d, const double o[3], const double dir[3],
                           double tmin, double tmax, oracle_hit* out);
int oracle_scene_occluded(const rt_scene_desc* d, const double o[3], const double dir[3],
                          double tmin, double tmax);

/* oracle_scene_occluded for n rays (o, dir: 3n doubles; tmin, tmax: n). */
int oracle_scene_occluded_batch(const rt_scene_desc* d, int n, const double* o, const double* dir, const double* tmin,
                                const double* tmax, uint8_t* out);
/* Tracer::trace (tracer.cpp:12-14) of Ray(o, dir) for n rays: rgb (3n) and each
 * ray's own Scene::intersect / Scene::occluded calls.  The ray is built once,
 * by the Ray constructor, so non-finite components arrive as they are (a ray
 * that goes through the camera is normalised twice). */
int oracle_trace_rays(const rt_scene_desc* d, int n, const double* o, const double* dir, double* rgb,
                      uint64_t* n_isect, uint64_t* n_occl);
/* The specular power, process-wide.  Mode 0 (the default) is libm pow, the
 * reference: every fixture under tests/golden is bit-equal to it.  Mode 1
 * returns the correctly rounded x^k from the two pow(rdotv, shininess) calls
 * of shade() wherever the device takes pow_spec (rt_device.hpp: an integer
 * exponent in [0, 1024); in oracle_shade_hits, whose wo is the caller's, also
 * |x| <= 2) and libm everywhere else: the oracle the FP64 kernels are held to
 * bit for bit (tests/test_gpu_rounding.py).  Set it only between calls. */
void oracle_set_pow(int mode);
int oracle_get_pow(void);
/* out[i] = that power of (x[i], y[i]) in the current mode; any_x as above. */
void oracle_spec_pow(int n, const double* x, const double* y, int any_x, double* out);

/* shade_lambert_phong(scene, Hit{t, p, n, mat of hits[i]}, wo[3i..]) for n
 * caller-given hits, the static shade() itself: rgb (3n) and each hit's own
 * Scene::occluded calls (n_occl, may be NULL).  A mat outside [0, n_materials)
 * is a null material.  n_lights < 0: the scene's point lights; >= 0: `lights`
 * instead of them, for this call. */
int oracle_shade_hits(const rt_scene_desc* d, int n, const oracle_hit* hits, const double* wo, const rt_light* lights,
                      int n_lights, double* rgb, uint64_t* n_occl);

/* The pixel-centre primary hit of every pixel of the W x H frame, pixel (i, j)
 * at index j*W + i: Camera::generate_ray(i, j) -> dirs, Scene::intersect(r,
 * 1e-4, inf) -> ok, hits. */
int oracle_primary_hits(const rt_scene_desc* d, int W, int H, double* dirs, oracle_hit* hits, uint8_t* ok);

/* Camera::generate_ray (subpixel=0) / generate_ray_subpixel (subpixel=1). */
void oracle_camera_ray(const rt_scene_desc* d, int i, int j, double dx, double dy, int subpixel,
                       double o[3], double dir[3]);

/* Jitter stream: the n-th uniform(-0.5,0.5) draw of std::mt19937(12345)
 * (tracer.cpp:284-293).  Fills out[k] for k in [first, first+count). */
void oracle_jitter(uint64_t first, uint64_t count, double* out);
/* Raw tempered mt19937(12345) outputs [first, first+count). */
void oracle_mt_words(uint64_t first, uint64_t count, uint32_t* out);

#ifdef __cplusplus
}
#endif
#endif
