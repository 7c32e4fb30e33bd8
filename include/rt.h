/*
 * rt.h — C-ABI of the MI355X-native per-pixel ray-trace path.
 *
 * This is the drop-in boundary for the reference's hot path
 * (alp-aydin/Raytracing-Project).  Every entry point is plain C: pointers,
 * sizes and integer error codes, no C++ types, no exceptions, no torch types.
 *
 * Reference seams replaced (paths relative to the reference repo root):
 *   rt_scene_load_json_text  <- jsonio::load_scene_from_json_text
 *                               raytracer/src/json_loader.cpp:458-490
 *   rt_scene_load_json_file  <- jsonio::load_scene_from_json
 *                               raytracer/src/json_loader.cpp:499-503
 *   rt_render                <- Tracer::render (standard + paper mode)
 *                               raytracer/src/tracer.cpp:247-305, tracer.h:18-35
 *   rt_render_multi          <- Tracer::render over the GPUs of one node (row
 *                               strips + RCCL gather)
 *   rt_render_rgb8           <- Tracer::render + framebuffer_to_mat_bgr8
 *                               (main.cpp:19-34, 74-89) on the device
 *   rt_dist_* / rt_render_dist <- the same for one process per GPU
 *   rt_render_rows_device    <- the same loop restricted to a set of output
 *                               rows (multi-GPU row tiling)
 *   rt_frame_begin/trace/end <- the same loop, split so that row chunks can
 *                               be gathered while later chunks are traced
 *   rt_scatter_rows_device   <- (no reference equivalent: places gathered row
 *                               bands into the full framebuffer on rank 0)
 *   rt_query_intersect       <- Scene::intersect, a batch of rays
 *                               raytracer/src/scene.cpp:10-24
 *   rt_query_occluded        <- Scene::occluded, a batch of rays
 *                               raytracer/src/scene.cpp:33-42
 *   rt_query_node_intersect  <- Primitive::intersect of one node, a batch of rays
 *   rt_query_node_interval   <- Primitive::interval of one node, a batch of rays
 *                               raytracer/src/geometry.h:62-75 (and every override)
 *   rt_query_radiance        <- Tracer::trace, a batch of rays
 *                               raytracer/src/tracer.cpp:12-73
 *   rt_query_shade           <- shade_lambert_phong, a batch of hits
 *                               raytracer/src/shading.cpp:31-138
 *   rt_camera_rays           <- Camera::generate_ray / generate_ray_subpixel for
 *                               the pixels of a set of rows, raytracer/src/camera.h:44-78
 *   rt_resolve_samples       <- the frame's sample sum and scale
 *                               raytracer/src/tracer.cpp:291-296
 *   rt_scatter_rays          <- the spawn half of Tracer::trace_recursive: reflect,
 *                               refract, has_total_internal_reflection, the 1e-6
 *                               origin offsets and the depth gate, a batch of hits
 *                               raytracer/src/tracer.cpp:34-67, 76-104
 *   rt_combine_bounce        <- its unwind half: combine(total, scale(I, k))
 *                               raytracer/src/tracer.cpp:47, 66, shading.cpp:6-22
 *   rt_query_radiance_depth  <- Tracer::trace_recursive(r, depth), a batch of rays
 *                               raytracer/src/tracer.h:46, tracer.cpp:22-73
 *   rt_framebuffer_to_rgb8   <- framebuffer_to_mat_bgr8 / toByte
 *                               raytracer/src/main.cpp:19-34, core.h:313-316
 *   rt_write_png             <- cv::imwrite (main.cpp:86-89)
 *
 * The scene is held in a flattened intermediate representation
 * (rt_scene_desc) produced by the host loader.  The same struct is consumed
 * by the GPU renderer and by the CPU oracle under oracle/ (test only).
 *
 * Library split:
 *   librt_host.so — loader, IR, PNG writer (pure host C++17, no HIP).
 *   librtamd.so   — HIP/gfx950 renderer; links librt_host.so.
 */
#ifndef RT_H
#define RT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 6   /* 2: rt_scene_desc gained directional lights
                              3: rt_stats gained the output-path timings; multi-GPU
                                 and device-output entry points (rt_render_multi,
                                 rt_render_rgb8, rt_dist_*)
                              4: rt_shutdown, device-buffer utilities, rt_dist_reduce_max /
                                 rt_dist_barrier
                              5: rt_dist_set_timeout, per-frame rank agreement,
                                 rt_host_register / rt_host_unregister
                              6: rt_dist_frame_split, rt_warmup; the frame descriptor
                                 carries the scene hash and the root strip shed
                              (still 6: the batched ray queries rt_query_intersect /
                               rt_query_occluded and their *_device forms, rt_ray and
                               rt_hit, are pure additions, as are the radiance queries
                               rt_query_radiance / rt_query_radiance_device, the
                               shading queries rt_query_shade / rt_query_shade_device,
                               the camera rays and sample resolve rt_camera_rays /
                               rt_camera_rays_device / rt_resolve_samples /
                               rt_resolve_samples_device, and the paper-frame links
                               rt_rays_wo / rt_rays_wo_device / rt_paper_resolve /
                               rt_paper_resolve_device, and the node queries
                               rt_query_node_intersect / rt_query_node_interval and
                               their *_device forms, and the bounce-loop links
                               rt_scatter_rays / rt_combine_bounce /
                               rt_query_radiance_depth and their *_device forms) */

/* ---------------------------------------------------------------- errors */
enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID_ARG = -1,   /* null pointer / bad size                      */
    RT_ERR_PARSE = -2,         /* "JSON parse error: ..." (json_loader.cpp:485) */
    RT_ERR_PROCESSING = -3,    /* "JSON processing error: ..." (:487)          */
    RT_ERR_IO = -4,            /* "Cannot open JSON file: ..." (:501) / PNG write */
    RT_ERR_HIP = -5,           /* HIP runtime failure (message in rt_last_error) */
    RT_ERR_UNSUPPORTED = -6,   /* scene exceeds a compiled device limit          */
    RT_ERR_NO_DEVICE = -7      /* no HIP device / extension missing             */
};

/* Last error message of the calling thread ("" if none). */
const char* rt_last_error(void);
int rt_abi_version(void);

/* -------------------------------------------------------- scene IR types */
enum rt_node_kind {
    RT_NODE_SPHERE = 0,       /* geometry.h:79-109     Sphere                    */
    RT_NODE_HALFSPACE = 1,    /* geometry.h:112-158    HalfSpace                 */
    RT_NODE_POKEBALL = 2,     /* geometry.h:161-242    Pokeball                  */
    RT_NODE_TRANSLATION = 3,  /* transform.h:87-111    Translation               */
    RT_NODE_SCALING = 4,      /* transform.h:117-141   Scaling                   */
    RT_NODE_ROTATION = 5,     /* transform.h:150-185   Rotation                  */
    RT_NODE_CSG = 6           /* csg.h:13-49           CSG                       */
};

enum rt_csg_op { RT_CSG_UNION = 0, RT_CSG_INTERSECTION = 1, RT_CSG_DIFFERENCE = 2 };

enum rt_pokeball_region {
    RT_PB_TOP = 0, RT_PB_BOTTOM = 1, RT_PB_BELT = 2, RT_PB_RING = 3, RT_PB_BUTTON = 4
};

/* Material — geometry.h:5-22.  Every JSON colour block instance (and each
 * of a pokeball's five region materials) gets its own index: the paper-mode
 * edge detector compares material identity (tracer.cpp:170). */
typedef struct rt_material {
    double albedo[3];
    double ambient[3];
    double kd, ks, kr, kt;
    double shininess;
    double refractive_index;
} rt_material;

/* Parameter layout of rt_node.v per kind:
 *   SPHERE      v[0..2]=centre  v[3]=radius
 *   HALFSPACE   v[0..2]=p0      v[3..5]=unit normal (normalised as geometry.h:124-134)
 *   POKEBALL    v[0..2]=centre  v[3]=radius  v[4]=belt_half  v[5]=button_outer
 *               v[6]=ring_width v[7..9]=unit button_dir (Dir3::normalized)
 *   TRANSLATION/SCALING/ROTATION
 *               v[0..11]  = forward matrix rows 0..2 (4 columns, row-major)
 *               v[12..23] = inverse matrix rows 0..2 (Matrix4::inverse, core.h:239)
 *   CSG         (no parameters; op in rt_node.op)
 * aux[] keeps the raw constructor inputs (used only to rebuild reference
 * objects in oracle/_ref): HALFSPACE aux[0..2]=normal as given,
 * POKEBALL aux[0..2]=button_dir as given, ROTATION aux[0]=angle in radians,
 * TRANSLATION/SCALING aux[0..2]=factors.
 * Children: a (transform subject / CSG left), b (CSG right); -1 if unused.
 * Materials: mat (sphere / halfspace), mats[5] (pokeball, rt_pokeball_region order). */
typedef struct rt_node {
    int32_t kind;
    int32_t a, b;
    int32_t op;        /* rt_csg_op for CSG; axis 0/1/2 for ROTATION */
    int32_t mat;
    int32_t mats[5];
    double v[24];
    double aux[4];
} rt_node;

typedef struct rt_light {      /* scene.h:21-26 PointLight */
    double pos[3];
    double intensity[3];
} rt_light;

/* scene.h:10-15 DirectionalLight.  The JSON loader never creates one
 * (json_loader.cpp has no key for it); they are reachable through
 * rt_scene_from_desc, as the reference's Scene::dir_lights is through its API,
 * and shaded before the point lights (shading.cpp:45-76). */
typedef struct rt_dir_light {
    double dir[3];             /* direction from the light toward the scene (incident) */
    double radiance[3];
} rt_dir_light;

typedef struct rt_camera {     /* camera.h:7-79 Camera + ScreenSpec */
    double eye[3];
    double P[3];
    double Lx, Ly;
    int32_t dpi;
    int32_t pad_;
} rt_camera;

typedef struct rt_scene_desc {
    rt_camera camera;
    double background[3];      /* scene.h:40 */
    double ambient[3];         /* scene.h:43 */
    double medium_index;       /* scene.h:45 */
    int32_t recursion_limit;   /* scene.h:47 (default 5) */
    int32_t n_lights;
    const rt_light* lights;
    int32_t n_materials;
    int32_t n_nodes;
    const rt_material* materials;
    const rt_node* nodes;
    int32_t n_objects;         /* top-level objects, in JSON order */
    int32_t pad_;
    const int32_t* objects;    /* node index of each top-level object */
    int32_t n_dir_lights;      /* scene.h:36 dir_lights (ABI 2) */
    int32_t pad2_;
    const rt_dir_light* dir_lights;
} rt_scene_desc;

/* ScreenSpec::nx/ny (camera.h:19-21): max(1, int(round(L * dpi))). */
int rt_camera_width(const rt_camera* cam);
int rt_camera_height(const rt_camera* cam);

/* -------------------------------------------------------- scene handles */
typedef struct rt_scene rt_scene;   /* opaque: owns the IR arrays */

/* Parse JSON text with the reference schema.  On failure *out is NULL and
 * rt_last_error() holds the message (same prefixes as the reference). */
int rt_scene_load_json_text(const char* text, size_t len, rt_scene** out);
int rt_scene_load_json_file(const char* path, rt_scene** out);
/* Deep-copy a caller-built IR into an owned scene. */
int rt_scene_from_desc(const rt_scene_desc* desc, rt_scene** out);
const rt_scene_desc* rt_scene_get_desc(const rt_scene* s);
void rt_scene_destroy(rt_scene* s);

/* ------------------------------------------------------------- render */
enum rt_mode { RT_MODE_STANDARD = 0, RT_MODE_PAPER = 1 };

typedef struct rt_stats {
    uint64_t rays_intersect;   /* Scene::intersect calls, reference definition (scene.cpp:10) */
    uint64_t rays_occluded;    /* Scene::occluded calls (scene.cpp:33)                         */
    uint64_t rays_traced;      /* intersect+occluded queries actually evaluated on device      */
    uint64_t pixels;
    double ms_rng;             /* jitter-stream generation (device); ~0 for a standard frame
                                  whose draws are resident from an earlier frame of the same
                                  size and rows (RT_JITTER_CACHE_MB): nothing is generated    */
    double ms_kernel;          /* trace kernels (device)                                        */
    double ms_total;           /* whole call, host wall clock                                   */
    uint64_t ops[16];          /* per-op counters when RT_FLAG_COUNT_OPS is set (rt_op_counter) */
    /* ABI 3: the rest of the frame's wall clock */
    double ms_gather;          /* multi-GPU: RCCL gather of the row strips + placement on the root (device) */
    double ms_tobyte;          /* device toByte + RGB packing (rt_render_rgb8)                      */
    double ms_d2h;             /* device -> host copy of the result                                 */
    int32_t n_gpus;            /* devices that rendered                                             */
    int32_t pad_;
} rt_stats;

/* Op counters used by the FLOP model. */
enum rt_op_counter {
    RT_OPC_SPHERE_ISECT = 0,    /* Sphere::intersect calls                 */
    RT_OPC_SPHERE_ISECT_HIT,    /*   ... that hit                          */
    RT_OPC_SPHERE_IVL,          /* Sphere::interval calls (incl. pokeball)  */
    RT_OPC_SPHERE_IVL_HIT,      /*   ... that produced an interval         */
    RT_OPC_HALF_ISECT,          /* HalfSpace::intersect calls              */
    RT_OPC_HALF_ISECT_HIT,
    RT_OPC_HALF_IVL,
    RT_OPC_POKE_REGION,         /* Pokeball::pick_region_material          */
    RT_OPC_CSG_COMBINE,         /* CSG::interval combine steps             */
    RT_OPC_XFORM,               /* transform ray mappings                  */
    RT_OPC_SHADE_LIGHT,         /* per-light shading evaluations           */
    RT_OPC_SHADE_SPEC,          /* ... with a specular pow()               */
    RT_OPC_SECONDARY,           /* reflection/refraction spawns            */
    RT_OPC_CULLED,              /* subtree evaluations skipped by a wave-uniform bound cull */
    RT_OPC_LIGHT_EVAL,          /* point-light loop iterations in shading  */
    RT_OPC_SHADE_CALL           /* shade_lambert_phong calls with a material */
};

enum rt_flags {
    RT_FLAG_NONE = 0,
    RT_FLAG_COUNT_OPS = 1,      /* fill rt_stats.ops (slower, instrumented kernels) */
    RT_FLAG_NO_CULL = 2,        /* disable wave-uniform bounding-sphere culling    */
    RT_FLAG_FP32 = 4,           /* NON-PARITY fast path: trace in
                                   FP32 on float copies of the scene; framebuffer stays
                                   double.  Not within the 1e-5 parity tolerance.   */
    RT_FLAG_NO_BVH = 8,         /* scenes of more than 256 top-level objects (the wave
                                   BVH threshold kWaveBvhMin, scene_compile.hpp) and no
                                   eager programs: wave-level culling without the wave
                                   BVH (A/B; results are identical).  No effect on
                                   smaller scenes, which never build the BVH.        */
    RT_FLAG_FORCE_BVH = 16,     /* a scene that has a wave BVH uses it on every frame.
                                   Without this flag (or RT_FLAG_NO_BVH) the first two
                                   frames of a frame shape try it on and off and later
                                   frames take the faster (identical results). */
    RT_FLAG_RAY_BVH = 32        /* rt_query_intersect / rt_query_occluded and their
                                   _device forms: every ray walks a bounding-ball tree
                                   over the scene's objects on its own instead of the
                                   flat object list - for incoherent batches (baking,
                                   probes, visibility) on scenes of many objects.  The
                                   results are the bytes of the same call without the
                                   flag (hits, masks, stats counts), non-finite rays
                                   included.  It changes the kernel only for a scene
                                   that has a wave list (more than 256 top-level
                                   objects, no eager programs), without
                                   RT_FLAG_NO_CULL, within the standard device stacks;
                                   otherwise it is accepted and the flat kernel runs.
                                   The tree is uploaded by the first such query of a
                                   scene and stays resident with it.  The node,
                                   radiance, shade and scatter calls and the frames
                                   accept the bit and ignore it. */
};

/* Tracer::render: render the whole frame into a caller-owned host buffer of
 * W*H*3 doubles (row-major, top row first, RGB), exactly like the
 * reference's std::vector<Color>.  W,H must be > 0 (the reference returns
 * silently otherwise, tracer.cpp:248 — here RT_ERR_INVALID_ARG).
 * Uses the current HIP device; blocks until done. */
int rt_render(const rt_scene* s, int W, int H, int mode, int flags,
              double* fb_host, rt_stats* stats);

/* Tracer::render over n_gpus HIP devices of THIS process (n_gpus <= 0: all
 * visible devices): every device renders interleaved strips of RT_STRIP_ROWS
 * (paper mode: RT_PAPER_STRIP_ROWS) output rows (a weighted round robin over the strips, rotated every
 * round, device 0 lighter for its placement work: rt_dist_rows_mode), and the strips reach
 * device 0 through RCCL ncclGather over xGMI (one collective per row chunk,
 * overlapped with the tracing of the next chunk) before the one D2H copy into
 * fb_host.  The result is bit-identical to rt_render (same kernels, same
 * jitter-stream offsets).  n_gpus == 1 is rt_render. */
int rt_render_multi(const rt_scene* s, int W, int H, int mode, int flags, int n_gpus, double* fb_host,
                    rt_stats* stats);

/* Tracer::render followed by framebuffer_to_mat_bgr8's toByte
 * (main.cpp:19-34, core.h:313-316) on the device(s), RGB order, top row
 * first: only 3 bytes per pixel cross xGMI and PCIe.
 * This is the CLI's path (`ray ... --gpus N`). */
int rt_render_rgb8(const rt_scene* s, int W, int H, int mode, int flags, int n_gpus, uint8_t* rgb8_host,
                   rt_stats* stats);

/* ------------------------------------------- one process per GPU (RCCL)
 * For launchers that start one process per device (torchrun, MPI): rank 0
 * calls rt_dist_get_id and hands the RT_DIST_ID_BYTES bytes to every rank,
 * each rank binds its current HIP device with rt_dist_create, and every
 * frame each rank calls rt_render_dist[_rgb8]: it renders its strips
 * (rt_dist_rows) and rank 0 receives the whole frame in its device buffer
 * (the ncclGather of rt_render_multi).  Non-root ranks pass NULL.  The call
 * returns when this rank's part (and on rank 0 the whole frame) is done;
 * stats are this rank's (ray counts of its rows). */
#define RT_STRIP_ROWS 8          /* standard mode */
#define RT_PAPER_STRIP_ROWS 30   /* paper mode: + 2 neighbour rows per strip = 32, four 8-row waves */
#define RT_DIST_ID_BYTES 128
typedef struct rt_dist rt_dist;
int rt_dist_get_id(uint8_t id[RT_DIST_ID_BYTES]);
int rt_dist_create(const uint8_t id[RT_DIST_ID_BYTES], int world, int rank, rt_dist** out);
void rt_dist_destroy(rt_dist* d);
int rt_render_dist(rt_dist* d, const rt_scene* s, int W, int H, int mode, int flags, double* fb_root_dev,
                   void* hip_stream, rt_stats* stats);
int rt_render_dist_rgb8(rt_dist* d, const rt_scene* s, int W, int H, int mode, int flags, uint8_t* rgb8_root_dev,
                        void* hip_stream, rt_stats* stats);
/* Max-reduction of n doubles over all ranks of d, in place on the host
 * (ncclAllReduce on the rank's collective stream; world 1 without a
 * communicator: unchanged), and a barrier built on it.  Launcher plumbing
 * for callers without a collective layer of their own (bench.py's max-over-
 * ranks timing). */
int rt_dist_reduce_max(rt_dist* d, double* vals_host, int n);
int rt_dist_barrier(rt_dist* d);
/* Failure behaviour of rt_render_dist[_rgb8] with more than one rank.  Every
 * rank issues every collective of a frame whatever happens locally, and the
 * ranks agree twice per frame through small RCCL max-reductions: before the
 * first gather on the frame descriptor (W, H, mode, output kind, flags) and
 * on each rank's setup status; before the last gather on each rank's trace
 * status.  So a rank-local failure makes EVERY rank return an error (the
 * failing rank its own; the others RT_ERR_INVALID_ARG for a descriptor
 * mismatch, RT_ERR_HIP naming the failed ranks otherwise) and the next frame
 * renders normally.  A wait for peers that exceeds the rank's timeout (or an
 * RCCL asynchronous error) aborts the communicator (ncclCommAbort) and returns
 * RT_ERR_HIP; that handle then refuses frames and must be destroyed.  The
 * timeout is RT_DIST_TIMEOUT_MS from the environment at creation (default
 * 120000) or rt_dist_set_timeout. */
int rt_dist_set_timeout(rt_dist* d, int timeout_ms);
/* This rank's split of its last successful collective frame (world > 1, or a
 * forced-collective world 1), in ms, for diagnosing a multi-GPU run from one
 * line (bench.py puts every rank's split into its JSON):
 *   out[0] the whole call (host)        out[1] the frame agreement's reduction (device)
 *   out[2] host wait for its verdict    out[3] this rank's gathers (device, sum)
 *   out[4] the root's placements (device, sum; 0 elsewhere)
 *   out[5] the last chunk's gather      out[6] the last chunk's placement (device)
 *   out[7] host time from the last enqueue to the call's return
 *   out[8] the communicator's rank count (ncclCommCount)
 *   out[9] output rows this rank traced
 * Writes min(n, 10) entries and returns that count. */
int rt_dist_frame_split(rt_dist* d, double* out, int n);
/* The partition of an FP64 frame: writes the output rows of `rank`
 * (ascending) to rows_out (room for H entries) and returns their count; <0
 * on bad arguments.  (RGB8 frames weight every rank equally.)
 * rt_dist_rows is the standard-mode partition (RT_STRIP_ROWS); paper mode
 * uses RT_PAPER_STRIP_ROWS strips (rt_dist_rows_mode). */
int rt_dist_rows(int H, int world, int rank, int32_t* rows_out);
int rt_dist_rows_mode(int H, int world, int rank, int mode, int32_t* rows_out);

/* Render an arbitrary set of OUTPUT rows (top-row-first indices) into a
 * compact device buffer fb_rows_dev[n_rows][W][3] on the given HIP stream
 * (NULL = default stream).  rows_host lists the rows, distinct, in any order
 * (a duplicate is RT_ERR_INVALID_ARG).  Only the jitter-stream segments those
 * rows consume are generated.  Blocks until done. */
int rt_render_rows_device(const rt_scene* s, int W, int H, int mode, int flags,
                          const int32_t* rows_host, int n_rows,
                          double* fb_rows_dev, void* hip_stream, rt_stats* stats);

/* Frame pipeline: rt_render_rows_device split into an asynchronous begin /
 * trace / end, so that a multi-GPU rank can hand finished row chunks to a
 * collective (RCCL on its own stream) while the next chunks are traced
 * (SURVEY.md §8e).  rt_frame_begin validates the rows (as
 * rt_render_rows_device), uploads the scene and enqueues the jitter stream of
 * ALL the listed rows; rt_frame_trace enqueues the trace of list entries
 * [ri0, ri1) into fb_rows_dev[0 .. ri1-ri0) (each list entry traced once)
 * on trace_stream (NULL = the frame's stream; another stream first waits for
 * begin's work, so consecutive chunks on two streams overlap their launch
 * tails); rt_frame_end joins every stream used, waits, fills stats and frees
 * the frame — call it exactly once per begun frame, also after an error.
 * begin/trace only enqueue work.  One frame per device at a time (begin
 * blocks while another frame of the same device is open). */
typedef struct rt_frame rt_frame;
int rt_frame_begin(const rt_scene* s, int W, int H, int mode, int flags, const int32_t* rows_host, int n_rows,
                   void* hip_stream, rt_frame** out);
int rt_frame_trace(rt_frame* f, int ri0, int ri1, double* fb_rows_dev, void* trace_stream);
int rt_frame_end(rt_frame* f, rt_stats* stats);

/* fb_dev[rows[i]][*] = src_dev[i][*] for i < n_rows (device copy, W*3 doubles per row);
 * slots with rows[i] < 0 (padding) are skipped. */
int rt_scatter_rows_device(const double* src_dev, const int32_t* rows_dev, int n_rows,
                           int W, double* fb_dev, void* hip_stream);

/* Device-side toByte + RGB packing: rgb8_dev[W*H*3]. */
int rt_framebuffer_to_rgb8_device(const double* fb_dev, size_t n_pixels,
                                  uint8_t* rgb8_dev, void* hip_stream);

/* ------------------------------------------------------- ray queries
 * Scene::intersect (closest hit, scene.cpp:10-24) and Scene::occluded (any
 * hit in a segment, scene.cpp:33-42) for a batch of caller-given rays: the
 * reference's two other public seams on its hot path (picking, visibility
 * probes, collision, light baking), on the device.
 *
 * A ray is the reference's Ray(o, d): d is normalised as in core.h:278 (a
 * direction of length <= 1e-6 becomes (0, 1, 0)), and t, tmin, tmax are in
 * world units along the normalised direction; tmax may be +inf.  The closest
 * hit applies each object's own accept rule with the tightening tmax, so ties
 * resolve exactly as in the reference; occluded is "any object's intersect in
 * [tmin, tmax]".  FP64, the parity path; the scene's camera plays no part.
 *
 * Non-finite rays.  A ray with a NaN or an infinity in o, d, tmin or tmax (or
 * a d whose length overflows or underflows) is no error: it gets the
 * reference's own result for that ray, which follows from the reference's
 * comparisons all being false on a NaN.  That result may be a hit with
 * t = NaN (a NaN or infinite origin, or an infinite direction, "hits" every
 * sphere and keeps the last object's record: t, p, n NaN, front_face 0,
 * occluded 1); a NaN direction, or one of length <= 1e-6, is (0, 1, 0), one
 * of infinite length the zero vector; tmin = NaN rejects nothing on a leaf.
 * Such a ray affects no other ray of the batch: every other ray's record is
 * the bytes it has in a batch without it, with and without RT_FLAG_NO_CULL.
 * The same holds for rt_query_radiance's rays and for rt_query_shade's hits
 * and wo under hit_mask = 1 (tests/test_gpu_leaves.py). */
typedef struct rt_ray {        /* 64 B */
    double o[3];
    double d[3];
    double tmin, tmax;
} rt_ray;
typedef struct rt_hit {        /* 64 B; geometry.h:25-46 Hit */
    double t;
    double p[3];
    double n[3];
    int32_t mat;               /* material index; -1 for a hit on a null material (rt_node.mat
                                  == -1, the reference's mat{nullptr}: t, p, n are the hit's)
                                  and on a miss (every other field 0): hit_mask tells them apart */
    int32_t front_face;
} rt_hit;
/* hits_host[i] = Scene::intersect(rays_host[i]) for i < n; hit_mask_host (may
 * be NULL) receives 1 for a hit and 0 for a miss.  Rays and results cross to
 * the device and back in chunks of bounded size.  flags: RT_FLAG_NONE or
 * RT_FLAG_NO_CULL (identical results; RT_FLAG_NO_BVH / RT_FLAG_FORCE_BVH
 * have no effect: queries walk the flat object list, whose results equal the
 * wave BVH's) or RT_FLAG_RAY_BVH (identical results: each ray walks the ray
 * BVH, see rt_flags); RT_FLAG_FP32 and RT_FLAG_COUNT_OPS are RT_ERR_UNSUPPORTED, as
 * is a scene beyond the device stacks.  n == 0 is RT_OK without a launch.
 * stats (may be NULL): rays_intersect = rays_traced = n, ms_kernel, ms_total.
 * Uses the current HIP device and shares its resident scene copy with the
 * frames (a query after a frame of the same scene uploads nothing, nor a
 * frame after a query); waits for an open frame of the device; blocks until
 * done. */
int rt_query_intersect(const rt_scene* s, const rt_ray* rays_host, size_t n, int flags, rt_hit* hits_host,
                       uint8_t* hit_mask_host, rt_stats* stats);
/* occluded_host[i] = Scene::occluded(rays_host[i]) as 1 / 0;
 * stats->rays_occluded = rays_traced = n. */
int rt_query_occluded(const rt_scene* s, const rt_ray* rays_host, size_t n, int flags, uint8_t* occluded_host,
                      rt_stats* stats);
/* The same with rays and results already on the device, enqueued on
 * hip_stream (NULL = the default stream); blocks until done. */
int rt_query_intersect_device(const rt_scene* s, const rt_ray* rays_dev, size_t n, int flags, rt_hit* hits_dev,
                              uint8_t* hit_mask_dev, void* hip_stream, rt_stats* stats);
int rt_query_occluded_device(const rt_scene* s, const rt_ray* rays_dev, size_t n, int flags, uint8_t* occluded_dev,
                             void* hip_stream, rt_stats* stats);

/* ------------------------------------------------------ node queries
 * Primitive::intersect and Primitive::interval (geometry.h:62-75), the virtual
 * pair every sphere, half-space, pokeball, transform and CSG node overrides,
 * of ONE node of the scene graph for a batch of caller-given rays: per-object
 * picking with the caller's own range whatever stands in front, inside /
 * outside classification of points (the reference's rule is enter.t < 1e-6 &&
 * exit.t > 1e-6, csg.cpp:92-94), thickness and X-ray images (exit.t - enter.t),
 * voxelisation and volume estimates of a CSG solid, collision sweeps against
 * one body, a preview of one operand of a CSG tree.
 *
 * node is an index into rt_scene_get_desc(s)->nodes: any node, not only a
 * top-level object's (objects[k] is top-level object k's); outside
 * [0, n_nodes) it is RT_ERR_INVALID_ARG.  The scene's other objects, its
 * lights and its camera play no part.  The ray is Ray(o, d) as for the other
 * queries (core.h:278).
 *
 * hits_host[i] = Primitive::intersect(node, Ray(rays_host[i].o, rays_host[i].d),
 * rays_host[i].tmin, rays_host[i].tmax): the reference's Hit exactly as
 * rt_query_intersect reports one (mat = -1 on a null material; all zero with
 * mat = -1 on a miss; hit_mask_host, which may be NULL, tells them apart).  A
 * degenerate Scaling never hits (transform.cpp:97).
 *
 * (enter_host[i], exit_host[i]) = Primitive::interval(node, Ray(rays_host[i].o,
 * rays_host[i].d)); tmin and tmax of rt_ray are NOT READ, interval has no
 * range.  enter.t is tEnter and exit.t is tExit, the call's out-parameters -
 * not the reference records' own Hit::t, which under a transform keeps a stale
 * local value nothing reads.  p, n, mat and front_face are what the reference
 * leaves in enterHit / exitHit, the odd cases included: a half-space's infinite
 * end has t = -inf / +inf, p = the ray's origin and the plane's face normal
 * (geometry.cpp:117-147); a CSG that contains the origin enters at t = 0 with
 * p = o, n = (0, 0, 0), the origin material of csg.cpp:120 and front_face = 1;
 * a difference's re-faced normals follow csg.cpp:139-150; a transform maps p
 * and n back and projects both t (transform.cpp:55-82).  Only the FIRST inside
 * interval along the ray is reported, as in the reference (csg.cpp:151): a
 * caller walks the further spans by querying again from beyond exit.t.  Where
 * interval returns false both records are zero with mat = -1 and
 * ok_mask_host[i] = 0.  ok_mask_host may be NULL, and so may either of
 * enter_host / exit_host, but not all three.  enter_host with ok_mask_host is
 * valid input for rt_query_shade[_device] as it is.
 *
 * Non-finite rays get the reference's answer and change no other ray's bytes,
 * as for the ray queries above.  flags: RT_FLAG_NONE or RT_FLAG_NO_CULL
 * (identical bytes: these kernels have no cull; RT_FLAG_NO_BVH /
 * RT_FLAG_FORCE_BVH have no effect); RT_FLAG_FP32 and RT_FLAG_COUNT_OPS are
 * RT_ERR_UNSUPPORTED, as is a node whose OWN subtree nests deeper than the
 * device stacks (the frames' limits and message; refused on the host before
 * any launch).  n == 0 is RT_OK without a launch; every argument check comes
 * before any device work.  stats (may be NULL): rays_intersect = rays_traced =
 * n for both calls (one primitive query per ray), ms_kernel, ms_total.  Per
 * ray 64 B cross to the device and 64 B (intersect) or 128 B (interval) plus
 * 1 B back, in chunks of bounded size.  Uses the current HIP device and shares
 * its resident scene copy with the frames and the other queries, which a node
 * query leaves as it was; the node's compiled program is built and uploaded
 * the first time that node is queried and kept with the resident scene (that
 * first query's compile counts in rt_setup_times[0]).  Waits for an open frame
 * of the device; blocks until done. */
int rt_query_node_intersect(const rt_scene* s, int node, const rt_ray* rays_host, size_t n, int flags,
                            rt_hit* hits_host, uint8_t* hit_mask_host, rt_stats* stats);
int rt_query_node_interval(const rt_scene* s, int node, const rt_ray* rays_host, size_t n, int flags,
                           rt_hit* enter_host, rt_hit* exit_host, uint8_t* ok_mask_host, rt_stats* stats);
/* The same with rays and results already on the device, enqueued on
 * hip_stream (NULL = the default stream); blocks until done. */
int rt_query_node_intersect_device(const rt_scene* s, int node, const rt_ray* rays_dev, size_t n, int flags,
                                   rt_hit* hits_dev, uint8_t* hit_mask_dev, void* hip_stream, rt_stats* stats);
int rt_query_node_interval_device(const rt_scene* s, int node, const rt_ray* rays_dev, size_t n, int flags,
                                  rt_hit* enter_dev, rt_hit* exit_dev, uint8_t* ok_mask_dev, void* hip_stream,
                                  rt_stats* stats);

/* -------------------------------------------------- radiance queries
 * Tracer::trace(const Ray&) (tracer.cpp:12-73) for a batch of caller-given
 * rays: the radiance along each ray - closest hit, Phong shading with a shadow
 * ray to every light (directional lights first), reflection and refraction
 * recursion - in standard-mode semantics: a miss returns the background,
 * recursion_limit <= 0 black, a hit on a null material the direct term only.
 * This is the seam for light baking, irradiance probes, reflection captures,
 * adaptive resampling and camera models other than the scene's flat screen:
 * the scene's camera plays no part, and there is no jitter or averaging.
 *
 * rgb_host[3i .. 3i+2] = Tracer::trace(Ray(rays_host[i].o, rays_host[i].d)).
 * The ray is Ray(o, d) as for the other queries (d normalised as in
 * core.h:278, a direction of length <= 1e-6 becomes (0, 1, 0)); tmin and tmax
 * of rt_ray are NOT READ: Tracer::trace always queries [1e-4, inf), and every
 * secondary ray follows the reference.  Per ray 64 B cross to the device and
 * 24 B back, in chunks of bounded size.  flags: RT_FLAG_NONE or
 * RT_FLAG_NO_CULL (byte-identical results; RT_FLAG_NO_BVH / RT_FLAG_FORCE_BVH
 * have no effect); RT_FLAG_FP32 and RT_FLAG_COUNT_OPS are RT_ERR_UNSUPPORTED,
 * as is a scene or recursion depth beyond the device stacks (the frames' own
 * limit and message).  n == 0 is RT_OK without a launch.  stats (may be NULL):
 * rays_intersect / rays_occluded are the Scene::intersect / Scene::occluded
 * calls that tracing these n rays makes (the quantities a frame reports),
 * rays_traced their sum, pixels 0, ms_kernel, ms_total.  Uses the current HIP
 * device and shares its resident scene copy with the frames and the other
 * queries; waits for an open frame of the device; blocks until done. */
int rt_query_radiance(const rt_scene* s, const rt_ray* rays_host, size_t n, int flags, double* rgb_host,
                      rt_stats* stats);
/* The same with rays and colours already on the device, enqueued on
 * hip_stream (NULL = the default stream); blocks until done. */
int rt_query_radiance_device(const rt_scene* s, const rt_ray* rays_dev, size_t n, int flags, double* rgb_dev,
                             void* hip_stream, rt_stats* stats);

/* --------------------------------------------------- shading queries
 * shade_lambert_phong(scene, hit, wo) (shading.h, shading.cpp:31-138) for a
 * batch of caller-given surface points: ambient, then every directional light,
 * then every point light with its shadow ray, combined and clamped as in the
 * reference.  This is the seam for light baking (a lightmap texel or a probe
 * is a point with a normal, not a ray), for deferred shading of a G-buffer
 * (rt_query_intersect once, then shade its hits) and for relighting the same
 * hits under other point lights without a new scene.  For wo = -d it is
 * Tracer::trace at recursion depth 1.
 *
 * rgb[3i .. 3i+2] = shade_lambert_phong(scene, Hit{t, p, n, mat of hits[i]},
 * wo[3i .. 3i+2]).  Of an rt_hit, t, p, n and mat are read (t sets the shadow
 * epsilon max(1e-3, 1e-4 t)); front_face is NOT READ.  n and wo are used as
 * given, not normalised, as in the reference.  wo is required.
 * Material index: mat == -1 gives magenta (1, 0, 1) (shading.cpp:33) without
 * a Scene::occluded call; any other mat outside [0, n_materials) is shaded as
 * a null material too and no table is read, in the host and device forms
 * alike: a garbage index never reads out of bounds.
 * hit_mask (may be NULL: every entry is shaded): where hit_mask[i] == 0,
 * nothing of hits[i] or wo[i] is interpreted, no occlusion query is made and
 * rgb[i] is miss_rgb, or the scene's background when miss_rgb is NULL; so
 * rt_query_intersect's (hits, hit_mask) output is a valid input as it is.
 * Light override: n_lights < 0: the scene's own point lights (lights is
 * ignored); n_lights == 0: no point lights (ambient and directional lights
 * only); n_lights > 0: these point lights instead of the scene's, for this
 * call only (lights == NULL is RT_ERR_INVALID_ARG).  Directional lights, the
 * ambient term and the materials are always the scene's.  lights and miss_rgb
 * are HOST memory in both forms.  The override leaves the device's resident
 * scene alone: a frame or query of s after it uploads nothing and renders as
 * before.
 * Per entry 89 B cross to the device (64 B hit, 24 B wo, 1 B mask) and 24 B
 * back, in chunks of bounded size.  flags: RT_FLAG_NONE or RT_FLAG_NO_CULL
 * (byte-identical results; RT_FLAG_NO_BVH / RT_FLAG_FORCE_BVH have no effect);
 * RT_FLAG_FP32 and RT_FLAG_COUNT_OPS are RT_ERR_UNSUPPORTED, as is a scene
 * beyond the device stacks (the frames' own limit and message).  n == 0 is
 * RT_OK without a launch, whatever the pointers (the flags are still checked).
 * stats (may be NULL): rays_occluded = the Scene::occluded calls the batch
 * makes, by the reference's definition; rays_intersect 0; rays_traced =
 * rays_occluded; pixels 0, n_gpus 1, ms_kernel, ms_total.  Uses the current HIP
 * device and shares its resident scene copy with the frames and the other
 * queries; waits for an open frame of the device; blocks until done. */
int rt_query_shade(const rt_scene* s, const rt_hit* hits_host, const double* wo_host, const uint8_t* hit_mask_host,
                   size_t n, const rt_light* lights, int n_lights, const double* miss_rgb, int flags,
                   double* rgb_host, rt_stats* stats);
/* The same with hits, wo, mask and colours already on the device (e.g.
 * rt_query_intersect_device's output, in place), enqueued on hip_stream (NULL
 * = the default stream); blocks until done. */
int rt_query_shade_device(const rt_scene* s, const rt_hit* hits_dev, const double* wo_dev, const uint8_t* hit_mask_dev,
                          size_t n, const rt_light* lights, int n_lights, const double* miss_rgb, int flags,
                          double* rgb_dev, void* hip_stream, rt_stats* stats);

/* ------------------------------------- camera rays and sample resolve
 * The first and the last link of a frame composed from the queries, on the
 * device: Camera::generate_ray / Camera::generate_ray_subpixel
 * (camera.h:44-78) for every pixel of a set of output rows, and the frame's
 * `acc += trace(...)` over its samples followed by `acc * (1.0 / spp)`
 * (tracer.cpp:291-296).  So
 *   frame = rt_resolve_samples(rt_query_radiance(rt_camera_rays(camera)))
 * with every buffer on the device, and because the camera is an argument the
 * same resident scene can be rendered from another camera (a moved eye, a
 * stereo pair, a crop at another dpi) without a new scene handle.
 *
 * cam: any camera; &rt_scene_get_desc(s)->camera is the scene's.  W, H mean
 * what they mean for rt_render; the camera's own nx x ny (rt_camera_width /
 * rt_camera_height) enter the formulas exactly as in the frames.  rows_host
 * lists OUTPUT rows, top row first, distinct, in any order, as for
 * rt_render_rows_device; NULL with n_rows == H: all rows in order.  A
 * duplicate or out-of-range row is RT_ERR_INVALID_ARG.  List entry ri, column
 * x (and sample s) go to
 *   rays[ri*W + x]                  RT_RAYS_CENTRE
 *   rays[(ri*W + x)*RT_SPP + s]     RT_RAYS_JITTERED, samples in the order the
 *                                   frame sums them.
 * RT_RAYS_CENTRE: Camera::generate_ray(x, row), including camera.h:47-49 (a
 * pixel outside the camera's nx x ny gives Ray{eye, (0, 0, -1)}).
 * RT_RAYS_JITTERED: output row r is loop row y = H-1-r (tracer.cpp:297);
 * sample s of pixel (x, y) takes draws 2*((y*W + x)*8 + s) and + 1 of the
 * reference's std::mt19937(12345) stream as (dx, dy), and the ray is
 * generate_ray_subpixel(x, y, dx, dy).  The draws are the frames' own: they
 * live in the frames' jitter cache under the frames' key (W, H, rows), so a
 * standard frame of the same size and rows after this call generates nothing,
 * nor this call after such a frame (RT_JITTER_CACHE_MB = 0 or a request beyond
 * the budget: generated into a transient buffer, as for such a frame).
 * o and d are what the reference's Ray holds; tmin = 1e-4 and tmax = +inf, the
 * interval Tracer::trace, trace_paper and get_edge_strength query: the output
 * is valid input for rt_query_intersect[_device] and
 * rt_query_radiance[_device] as it is.
 * n_rows == 0 is RT_OK without a launch.  NULL cam, W <= 0, H <= 0, an unknown
 * kind, or a NULL output with n_rows > 0 is RT_ERR_INVALID_ARG; every argument
 * check comes before any device work.  stats (may be NULL): pixels = n_rows*W,
 * ms_rng (the jitter generation; ~0 when the draws were resident), ms_kernel,
 * ms_total, n_gpus = 1; the ray counts are 0.  Both forms use the current HIP
 * device, wait for an open frame of the device and block until done; the host
 * form runs the device form's kernel over row chunks of bounded size through
 * the queries' staging buffer. */
enum rt_camera_rays_kind { RT_RAYS_CENTRE = 0, RT_RAYS_JITTERED = 1 };
#define RT_SPP 8   /* samples per pixel of a standard frame (tracer.cpp:283) */
int rt_camera_rays_device(const rt_camera* cam, int W, int H, int kind, const int32_t* rows_host, int n_rows,
                          rt_ray* rays_dev, void* hip_stream, rt_stats* stats);
int rt_camera_rays(const rt_camera* cam, int W, int H, int kind, const int32_t* rows_host, int n_rows,
                   rt_ray* rays_host, rt_stats* stats);
/* fb[3p + c] = (((0 + rgb[(p*spp + 0)*3 + c]) + rgb[(p*spp + 1)*3 + c]) + ...)
 * * (1.0 / spp) for p < n_pixels, c < 3, in that order: the frame's own sum and
 * scale for spp = RT_SPP.  1 <= spp <= 64, anything else is
 * RT_ERR_INVALID_ARG, as is a NULL buffer with n_pixels > 0 or an fb that
 * overlaps rgb.  n_pixels == 0 is RT_OK.  The device form runs on hip_stream
 * (NULL = the default stream) of the current device and blocks until done; the
 * host form is a plain loop in librt_host.so and needs no device. */
int rt_resolve_samples_device(const double* rgb_dev, size_t n_pixels, int spp, double* fb_dev, void* hip_stream);
int rt_resolve_samples(const double* rgb_host, size_t n_pixels, int spp, double* fb_host);

/* ------------------------------------ paper frames from the queries
 * The two links that make a paper-mode frame (tracer.cpp:258-281) a
 * composition of the queries, with every buffer on the device:
 *   paper = rt_paper_resolve(hits, mask, rt_query_shade(hits, rt_rays_wo(rays), mask, miss_rgb = (1,1,1)))
 *   where (hits, mask) = rt_query_intersect(rays), rays = rt_camera_rays(cam, RT_RAYS_CENTRE).
 * trace_paper (tracer.cpp:111-120) is the shading of the centre rays' hits on
 * white; what remains is the stencil of Tracer::get_edge_strength
 * (tracer.cpp:133-178), get_luminance (:123-125) and apply_crosshatch
 * (:188-205) over that G-buffer.  Because the camera and the lights are
 * arguments of the earlier links, a paper frame of the resident scene can be
 * rendered from any camera and under rt_query_shade's light override, and the
 * edge strength is an output of its own (an outline pass over any frame).
 *
 * rt_rays_wo: wo[3i .. 3i+2] = (-Ray(rays[i].o, rays[i].d).d).normalized(), the
 * wo that Tracer::trace and trace_paper hand to shade_lambert_phong
 * (tracer.cpp:30, :115).  The Ray constructor's own normalisation comes first
 * (core.h:278: a direction of length <= 1e-6, or NaN, becomes (0, 1, 0)), then
 * Dir3::normalized of the negation.  o, tmin and tmax are NOT READ.  n == 0 is
 * RT_OK without a launch; a NULL buffer with n > 0, or a wo that overlaps rays,
 * is RT_ERR_INVALID_ARG.  The device form runs on hip_stream (NULL = the
 * default stream) of the current device and blocks until done; the host form
 * is a plain loop in librt_host.so and needs no device. */
int rt_rays_wo_device(const rt_ray* rays_dev, size_t n, double* wo_dev, void* hip_stream);
int rt_rays_wo(const rt_ray* rays_host, size_t n, double* wo_host);
/* rt_paper_resolve: output rows [row0, row0 + n_rows) of a W x H paper frame.
 * Paper mode does not flip: the output row is y of generate_ray(x, y), so the
 * rows of rt_camera_rays(..., RT_RAYS_CENTRE, rows) line up as they are.
 * Input band: hits, hit_mask and rgb hold frame rows [in0, in1) =
 * [max(0, row0 - 1), min(H, row0 + n_rows + 1)): the band plus the halo rows
 * that exist inside the frame.  Pixel (x, y) is at index (y - in0)*W + x of
 * each (rgb: 3 doubles per pixel).  A whole frame is row0 = 0, n_rows = H and
 * has no halo; the band form tiles a frame whose records exceed a buffer (the
 * hits of 7680x4320 are 2.1 GB) and splits one over several devices.
 * edge[(y - row0)*W + x] = get_edge_strength(x, y) from the stored records:
 * neighbours in the order (-1,0) (1,0) (0,-1) (0,1); one outside W x H is
 * skipped and not counted as valid; "hits" is hit_mask != 0 (NULL: every entry
 * is a hit); the 0.9 (hit against miss), 0.6 (min t > 1e-4 and max t / min t >
 * 3), 0.5 (n . n' < 0.2) and 0.3 (mat != mat' and n . n' < 0.7) rules read t, n
 * and mat of rt_hit; material identity is the index (-1 equals -1, as the
 * reference's two null pointers do); the result is halved when fewer than 4
 * neighbours are valid.  std::min / std::max and every comparison behave as in
 * the reference on NaN and infinity.  p and front_face are NOT READ.
 * fb[((y - row0)*W + x)*3 ..] is the pixel of tracer.cpp:266-279 from base =
 * rgb of the pixel, L = 0.299 r + 0.587 g + 0.114 b (left to right, no
 * contraction), the edge strength and apply_crosshatch(base, L, x, y).  rgb is
 * read for every pixel, misses included: the reference's white for a miss is
 * the caller's miss_rgb = (1, 1, 1) in rt_query_shade.  A NaN luminance takes
 * no hatch branch and gives white.
 * Either output may be NULL, but not both; rgb may be NULL only when fb is.
 * RT_ERR_INVALID_ARG: W <= 0, H <= 0, row0 < 0, n_rows < 0, row0 + n_rows > H,
 * a NULL hits with n_rows > 0, or an output that overlaps an input; every
 * argument check comes before any device work.  n_rows == 0 is RT_OK without a
 * launch.  stats (may be NULL): pixels = n_rows*W, ms_kernel, ms_total, n_gpus
 * = 1; the ray counts are 0.  The device form uses the current HIP device,
 * enqueues on hip_stream (NULL = the default stream), waits for an open frame
 * of the device and blocks until done.  It needs no scene and uploads nothing:
 * the resident scene copy is left alone.  The host form is a plain loop in
 * librt_host.so, compiled without FP contraction, and needs no device: it is
 * the statement of the rules the device form matches bit for bit. */
int rt_paper_resolve_device(const rt_hit* hits_dev, const uint8_t* hit_mask_dev, const double* rgb_dev, int W, int H,
                            int row0, int n_rows, double* fb_dev, double* edge_dev, void* hip_stream, rt_stats* stats);
int rt_paper_resolve(const rt_hit* hits_host, const uint8_t* hit_mask_host, const double* rgb_host, int W, int H,
                     int row0, int n_rows, double* fb_host, double* edge_host);

/* ------------------------------------------------ bounce-by-bounce tracing
 * The recursion of Tracer::trace_recursive (tracer.cpp:22-73) as links of its
 * own, so that a caller can run it level by level with every buffer on the
 * device and read, reweight, stop or replace rays between bounces:
 *   level k:  (hits, mask) = rt_query_intersect(rays_k)
 *             direct_k     = rt_query_shade(hits, rt_rays_wo(rays_k), mask)   (miss_rgb NULL: the background)
 *             rays_k+1     = rt_scatter_rays(rays_k, hits, mask, depth = k)   until it spawns nothing
 *   unwind:   direct_k     = rt_combine_bounce(direct_k, spawn_k, first_k, direct_k+1, w_k+1)  from the last level up
 * direct_0 is then rt_query_radiance(rays_0) bit for bit, with the same
 * Scene::intersect / Scene::occluded totals (tests/test_gpu_bounce.py;
 * rtamd.radiance_bounces_device is this loop).
 *
 * rt_scatter_rays: the spawn half (tracer.cpp:34-67) for a batch of parents,
 * parent i being (rays[i], hits[i]).  r = Ray(rays[i].o, rays[i].d), the
 * constructor's normalisation as in every query; only d is read, o, tmin and
 * tmax are NOT READ.  A parent spawns nothing where hit_mask[i] == 0 (a NULL
 * mask: every entry is a hit), where hits[i].mat == -1, and where hits[i].mat
 * lies outside [0, n_materials) (a null material, as in rt_query_shade; in the
 * last two cases no table is read).  can = (int64)depth < (int64)recursion_limit
 * - 1; any int depth is accepted.  With incident = r.d.normalized() and n, p,
 * front_face of the hit as stored (n is not normalised):
 *   reflection, if kr > 0.0 && can:
 *     direction reflect(incident, n).normalized(), reflect = incident -
 *     (2.0 * incident.dot(n)) * n; origin front_face ? p + n*1e-6 : p - n*1e-6;
 *     weight kr
 *   refraction, if kt > 0.0 && can and there is no total internal reflection:
 *     eta = front_face ? medium / ri : ri / medium; cos_i = -incident.dot(n);
 *     sin_t2 = eta*eta*std::max(0.0, 1.0 - cos_i*cos_i); TIR is sin_t2 >= 1.0 (a
 *     NaN is not TIR, as in the reference); direction (eta*incident + (eta*cos_i -
 *     sqrt(1.0 - sin_t2))*n).normalized(); origin with the opposite sign of the
 *     reflection's; weight kt
 * Every comparison behaves as the reference's does on NaN; normalized() of a
 * NaN or short vector is (0, 1, 0).
 * spawn[i] holds the bits RT_SPAWN_REFLECT | RT_SPAWN_REFRACT, first[i] the
 * number of children of parents 0 .. i-1; the children are compacted in parent
 * order, a parent's reflection before its refraction, so the same input gives
 * the same bytes on every run.  Child j is child_rays[j] with weight child_w[j].
 * A child ray holds the origin and THE DIRECTION HANDED TO THE Ray CONSTRUCTOR
 * (the .normalized() results above), not the constructor's own result - unlike
 * rt_camera_rays, which stores what the reference's Ray holds - and tmin = 1e-4,
 * tmax = +inf.  The query that traces it next builds Ray(o, d) exactly as
 * tracer.cpp:45 / :64 do; that is what makes the composition equal
 * rt_query_radiance to the bit (one normalisation more or fewer moves last bits).
 * *n_children_host (HOST memory in both forms; may not be NULL) always receives
 * the total m.  m > child_cap is RT_ERR_INVALID_ARG with m written, spawn and
 * first complete, and nothing written beyond child_cap entries of either child
 * buffer; child_cap >= 2n can never fail (child_cap == 0 with NULL child
 * buffers sizes a call).  n == 0 is RT_OK with m = 0 and no launch.  A NULL
 * scene, n_children_host, or (with n > 0) rays, hits, spawn, first, or a NULL
 * child buffer with child_cap > 0, or an output that overlaps an input or
 * another output, is RT_ERR_INVALID_ARG; every argument check comes before any
 * device work.  There is no flags argument: the call makes no scene query.
 * stats (may be NULL): every count 0; ms_kernel, ms_total, n_gpus = 1 (the
 * host form: ms_total only).  The device form uses the current HIP device and
 * its resident scene copy (the materials, medium index and recursion limit),
 * which it shares with the frames and queries and leaves as it was: after a
 * query of the same scene it uploads nothing.  It enqueues on hip_stream (NULL
 * = the default stream), waits for an open frame of the device and blocks
 * until done.  One launch takes up to 2^30 parents; a larger n runs as several,
 * the child index carried across them.  The host form is a plain loop in
 * librt_host.so over the scene's own rt_scene_desc, compiled without FP
 * contraction, and needs no device: it is the statement of the rules the
 * device form matches bit for bit. */
#define RT_SPAWN_REFLECT 1
#define RT_SPAWN_REFRACT 2
int rt_scatter_rays_device(const rt_scene* s, const rt_ray* rays_dev, const rt_hit* hits_dev, const uint8_t* hit_mask_dev,
                           size_t n, int depth, uint8_t* spawn_dev, uint64_t* first_dev, rt_ray* child_rays_dev,
                           double* child_w_dev, size_t child_cap, size_t* n_children_host, void* hip_stream,
                           rt_stats* stats);
int rt_scatter_rays(const rt_scene* s, const rt_ray* rays_host, const rt_hit* hits_host, const uint8_t* hit_mask_host,
                    size_t n, int depth, uint8_t* spawn_host, uint64_t* first_host, rt_ray* child_rays_host,
                    double* child_w_host, size_t child_cap, size_t* n_children_host, rt_stats* stats);
/* rt_combine_bounce: the unwind half (tracer.cpp:47, :66).  rgb holds 3n
 * doubles, the parents' direct colours in and their totals out:
 *   total = rgb[i]
 *   if spawn[i] & 1: total = combine(total, child_rgb[j] * child_w[j]), j = first[i]
 *   if spawn[i] & 2: the same with j = first[i] + (spawn[i] & 1)
 * per channel combine(a, b) = 1.0 - (1.0 - a)*(1.0 - b) and the scale c * w
 * (shading.cpp:6-22, in that order, no contraction).  A child index >=
 * n_children is skipped in both forms: a garbage index never reads out of
 * bounds.  A NULL rgb, spawn or first with n > 0, a NULL child buffer with
 * n_children > 0, or an rgb that overlaps child_rgb (or another input) is
 * RT_ERR_INVALID_ARG; n == 0 is RT_OK.  The device form has one lane per
 * parent, needs no scene and uploads nothing; it runs on hip_stream (NULL = the
 * default stream) of the current device and blocks until done.  The host form
 * is a plain loop in librt_host.so and needs no device. */
int rt_combine_bounce_device(double* rgb_dev, const uint8_t* spawn_dev, const uint64_t* first_dev, size_t n,
                             const double* child_rgb_dev, const double* child_w_dev, size_t n_children, void* hip_stream);
int rt_combine_bounce(double* rgb_host, const uint8_t* spawn_host, const uint64_t* first_host, size_t n,
                      const double* child_rgb_host, const double* child_w_host, size_t n_children);
/* rt_query_radiance_depth: rt_query_radiance[_device] started at a recursion
 * depth: rgb[3i .. 3i+2] = Tracer::trace_recursive(Ray(rays[i].o, rays[i].d),
 * depth) (tracer.h:46).  Every test in trace_recursive compares depth with the
 * limit only, so this is rt_query_radiance of the same scene with
 * recursion_limit - depth for its limit (computed in 64 bits, clamped to int):
 * the same kernels, chosen for that limit, on the resident scene, which is
 * left alone (a frame or query of s after it uploads nothing and renders as
 * before).  depth = 0 gives rt_query_radiance's bytes and counts; depth >=
 * recursion_limit gives black and zero counts; the children of
 * rt_scatter_rays(depth = k) are traced with depth = k + 1.  Flags, refusals
 * (a remaining depth beyond the device stacks included) and stats are
 * rt_query_radiance's. */
int rt_query_radiance_depth(const rt_scene* s, const rt_ray* rays_host, size_t n, int flags, int depth, double* rgb_host,
                            rt_stats* stats);
int rt_query_radiance_depth_device(const rt_scene* s, const rt_ray* rays_dev, size_t n, int flags, int depth,
                                   double* rgb_dev, void* hip_stream, rt_stats* stats);

/* ------------------------------------------------------------ host I/O */
/* toByte(v) = round(clamp01(v)*255) (core.h:316), RGB order. */
void rt_framebuffer_to_rgb8(const double* fb, size_t n_pixels, uint8_t* rgb8);
/* Write an 8-bit RGB PNG (zlib deflate, n_threads > 1 parallelises the deflate). */
int rt_write_png(const char* path, const uint8_t* rgb8, int W, int H, int n_threads);

/* Number of HIP devices visible (0 when none / driver not loaded). */
int rt_device_count(void);

/* ------------------------------------------ device buffers and teardown
 * For callers with no device-memory layer of their own (a cgo / JNI / ctypes
 * binding, tests, bench.py): plain HIP allocations and copies on the
 * library's own HIP runtime, so a process needs no second one.  All return
 * an rt_status; sizes are bytes. */
int rt_set_device(int device);                       /* hipSetDevice for this thread        */
int rt_device_alloc(size_t bytes, void** dev_out);   /* hipMalloc, zero-filled              */
int rt_device_free(void* dev);
int rt_memcpy_h2d(void* dev, const void* host, size_t bytes);
int rt_memcpy_d2h(void* host, const void* dev, size_t bytes);
int rt_device_synchronize(void);
int rt_stream_create(void** stream_out);             /* non-blocking HIP stream              */
int rt_stream_destroy(void* stream);
/* Page-lock an existing host buffer (hipHostRegister) so that the output
 * copies of rt_render_rgb8 / rt_render_multi into it run as direct DMA
 * instead of through the runtime's pageable staging: for callers that render
 * many frames into the same buffer (registering 25 MB costs ~50 ms, so the
 * one-frame `ray` CLI does not).  Unregister before freeing it. */
int rt_host_register(void* host, size_t bytes);
int rt_host_unregister(void* host);
/* One-time setup costs of this process so far, host wall clock in ms:
 * out[0] scene compile + upload (first frame of each scene), out[1] jitter
 * checkpoint-table builds / extensions, out[2] first trace-kernel launch
 * (loads the kernels' code object onto the device), out[3] first jitter-fill
 * launch (its code object), out[4] device allocations (hipMalloc), out[5]
 * page-locked host allocations, out[6] stream / event creation; and the
 * split of the LAST frame (not cumulative): out[7] rt_frame_begin, out[8]
 * its rt_frame_trace calls, out[9] rt_frame_end, out[10] the device-group
 * setup of the last rt_render_multi / rt_render_rgb8 call; out[11] the
 * one-time copy-engine warm-up (host time, overlapped with the first
 * frame's trace).  min(n, 12) entries are written. */
int rt_setup_times(double* out, int n);
/* One-time preparation a caller can start early, e.g. on a helper thread
 * while its main thread initialises HIP or parses the scene:
 *   RT_WARM_HOST    host-only: the jitter stream's jump-tree tap lists (read
 *                   from lib/mt19937_tree.polys; ~3 ms), cached for the process
 *   RT_WARM_DEVICE  loads the FP64 render kernels' code object onto the
 *                   current device (~5 ms at a process's first trace launch)
 * Thread-safe; the frames that follow find the work done. */
enum { RT_WARM_HOST = 1, RT_WARM_DEVICE = 2 };
int rt_warmup(int what);
/* Release every device resource the library caches (per-device workspaces,
 * resident scenes, jitter tables and jitter draws, the rt_render_multi device groups with
 * their RCCL communicators).  No render may be in flight; later calls
 * re-create what they need.  The `ray` CLI calls it before exit when it
 * rendered on several GPUs (RCCL communicators); a one-GPU run leaves the
 * device memory to process exit. */
int rt_shutdown(void);

#ifdef __cplusplus
}
#endif
#endif /* RT_H */
