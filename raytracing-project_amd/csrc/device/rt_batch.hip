// rt_batch.hip — the batched entry points of librtamd, on the frames' workspace
// (rt_workspace.hpp) through one driver, BatchCall.  What each computes and
// where its kernels are:
//   query_impl        Scene::intersect / ::occluded (scene.cpp:10-42), rt_query_kernels.hpp; with the frames'
//                     counters Tracer::trace (tracer.cpp:12-73), rt_radiance_kernels.hpp; _depth: at a depth
//   shade_impl        shade_lambert_phong (shading.cpp:31-138), rt_shade_kernels.hpp
//   node_impl         Primitive::intersect / ::interval of one node (geometry.h:62-75), rt_node_kernels.hpp
//   camera_rays_impl  camera.h:44-78 on the frames' jitter draws; resolve: tracer.cpp:291-296, rt_camera_f64.hip
//   scatter_impl      the spawn half of Tracer::trace_recursive (tracer.cpp:34-67), combine: the unwind half,
//                     rt_bounce_f64.hip;  rt_paper_resolve_device, rt_rays_wo_device: rt_paper_f64.hip
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "rt_bounce.hpp"
#include "rt_camera.hpp"
#include "rt_paper.hpp"
#include "rt_workspace.hpp"

using namespace rtw;
using rtamd::kCounterWords;
using rtamd::NodeParams;
using rtamd::QueryParams;
using rtamd::RadianceParams;
using rtamd::SceneView;
using rtamd::ShadeParams;

namespace {

// ------------------------------------------------------ batched-call driver
// What every batched entry point (the ray, radiance and shading queries, the
// camera rays, the paper resolve) shares.  An entry point is its argument
// checks, a BatchCall, its buffers and parameter block, and one run() whose
// callbacks stage a chunk in, launch, and stage it out.  (The sizes of a
// launch and of a chunk: kLaunchItems, g_chunk_items, rt_workspace.hpp.)
constexpr int kKnownFlags =
    RT_FLAG_COUNT_OPS | RT_FLAG_NO_CULL | RT_FLAG_FP32 | RT_FLAG_NO_BVH | RT_FLAG_FORCE_BVH | RT_FLAG_RAY_BVH;

// One batched call on stream st.  Made first (it takes the call's start time);
// zero_stats() once the arguments that are checked before the stats are fine;
// open() before the first use of the device.  From open() on the call holds
// the workspace like a frame, and its session drains st when the call ends,
// however it ends (WorkspaceSession).
struct BatchCall {
    const char* what;
    hipStream_t st;
    rt_stats* stats = nullptr;
    const SClock::time_point t_start = SClock::now();
    WorkspaceSession ses;
    Workspace* ws = nullptr;   // ses.ws
    bool counting = false;     // counters(): finish() reduces the slots
    double ms_kernel = 0.0;    // run(): the chunks' launches, by the workspace's events

    BatchCall(const char* what_, hipStream_t st_) : what(what_), st(st_) {}
    int fail(const char* msg, int rc) const {
        rtamd::set_last_error(std::string(what) + ": " + msg);
        return rc;
    }
    // what the queries on a scene check first: the scene, the flag bits, the
    // flags' combinations
    int check_scene_flags(const rt_scene* s, int flags) const {
        if (!s) return fail("scene is NULL", RT_ERR_INVALID_ARG);
        if (flags & ~kKnownFlags) return fail("unknown flag bits", RT_ERR_INVALID_ARG);
        return rtamd::check_query_flags(flags);
    }
    void zero_stats(rt_stats* stats_) {
        stats = stats_;
        if (!stats) return;
        std::memset(stats, 0, sizeof(*stats));
        stats->n_gpus = 1;
    }
    int open() {
        const int rv = ses.open(what, st);
        ws = ses.ws;
        return rv;
    }
    // s resident in the workspace, the variant `pick` chooses for it, and its
    // view with the flat object list (a batch's items are arbitrary)
    // (pick_desc: the variant is chosen for that description instead of s's own:
    // rt_query_radiance_depth's copy with the remaining depth for its limit)
    int scene(const rt_scene* s, int flags,
              int (*pick)(const rtamd::CompiledScene&, const rt_scene_desc&, int, rtamd::KernelVariant*),
              rtamd::KernelVariant& kv, SceneView& S, const rt_scene_desc* pick_desc = nullptr) {
        const rt_scene_desc& d = *rt_scene_get_desc(s);
        int rv = scene_resident(*ws, s, d, false, st);
        if (rv == RT_OK) rv = pick(ws->scene.sc.cs, pick_desc ? *pick_desc : d, flags, &kv);
        if (rv != RT_OK) return rv;
        scene_view(*ws, d, flags, S);
        S.n_chunks = 0;
        return RT_OK;
    }
    // the frames' ray counter slots, zero before the first launch
    int counters() {
        int rv = counters_ready(*ws, st);
        if (rv == RT_OK) rv = ensure_ctr_host(*ws, kCounterWords);
        counting = rv == RT_OK;
        return rv;
    }
    // n items in chunks of at most `chunk`, each chunk in launches of at most
    // launch_max: in(c0, cn) stages items [c0, c0 + cn) in, launch(c0, l0, ln)
    // launches the chunk's items [l0, l0 + ln), out(c0, cn) stages the results
    // out; each returns RT_OK or the error to end with.  A chunk is complete
    // when the next begins (the chunk buffers and the events are reused).  A
    // call on device memory is one chunk of n with nothing to stage.
    template <class In, class Launch, class Out>
    int run(size_t n, size_t chunk, size_t launch_max, In&& in, Launch&& launch, Out&& out) {
        hipEvent_t* ev = ws->sync.ev;
        for (size_t c0 = 0; c0 < n; c0 += chunk) {
            const size_t cn = std::min(chunk, n - c0);
            int rv = in(c0, cn);
            if (rv != RT_OK) return rv;
            HIP_TRY(hipEventRecord(ev[1], st));
            for (size_t l0 = 0; l0 < cn && rv == RT_OK; l0 += launch_max) rv = launch(c0, l0, std::min(launch_max, cn - l0));
            if (rv != RT_OK) return rv;
            HIP_TRY(hipEventRecord(ev[2], st));
            rv = out(c0, cn);
            if (rv != RT_OK) return rv;
            HIP_TRY(hipStreamSynchronize(st));
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev[1], ev[2]) == hipSuccess) ms_kernel += ms;
        }
        return RT_OK;
    }
    static int no_staging(size_t, size_t) { return RT_OK; }
    // The call's good end: a counting call's slots summed as a frame's end reads
    // them (ctr(0), ctr(1): the Scene::intersect / Scene::occluded calls; the
    // slots are left zero), and the times.
    int finish() {
        if (counting) {
            HIP_TRY(launch_reduce_counters(st, ws->frame.counters.as<unsigned long long>(), ws->frame.ctr_host, nullptr, 0, 0));
            HIP_TRY(hipStreamSynchronize(st));
            ws->frame.counters_zero = true;
        }
        if (stats) {
            stats->ms_kernel = ms_kernel;
            stats->ms_total = ms_since(t_start);
        }
        return RT_OK;
    }
    uint64_t ctr(int word) const { return ((volatile unsigned long long*)ws->frame.ctr_host)[word]; }
};

// ------------------------------------------------------------- ray queries
// rt_query_{intersect,occluded,radiance}[_device]: kind rtamd::kQueryIsect /
// kQueryOccl / kQueryRadiance (results: hits and mask / mask / rgb, three
// doubles per ray).  host: rays and results are host memory, moved through the
// workspace's chunk buffers; else device memory, traced in place on st.  A
// radiance query counts its Scene::intersect / Scene::occluded calls.
// depth (radiance only; null: 0): Tracer::trace_recursive(r, *depth).  Every
// test there compares depth with the limit only (tracer.cpp:26, 38, 51), so it
// is the trace of a scene whose limit is recursion_limit - depth: the kernel is
// picked for that limit (its refusals too) and launched with it in this call's
// SceneView; the resident scene is what it was.
int query_impl(const char* what, const rt_scene* s, int kind, const rt_ray* rays, size_t n, int flags, rt_hit* hits,
               uint8_t* mask, double* rgb, bool host, hipStream_t st, rt_stats* stats, const int* depth = nullptr) {
    BatchCall call(what, st);
    const bool isect = kind == rtamd::kQueryIsect, radiance = kind == rtamd::kQueryRadiance;
    int rv = call.check_scene_flags(s, flags);
    if (rv != RT_OK) return rv;
    call.zero_stats(stats);
    if (n == 0) return RT_OK;
    if (!rays) return call.fail("rays is NULL", RT_ERR_INVALID_ARG);
    if (radiance ? !rgb : isect ? !hits : !mask) return call.fail("the result buffer is NULL", RT_ERR_INVALID_ARG);
    rtamd::KernelVariant kv;
    SceneView S;
    rt_scene_desc at_depth = *rt_scene_get_desc(s);
    if (depth) {
        const int64_t left = (int64_t)at_depth.recursion_limit - (int64_t)*depth;
        at_depth.recursion_limit = (int)std::min<int64_t>(std::max<int64_t>(left, INT32_MIN), INT32_MAX);
    }
    rv = call.open();
    if (rv == RT_OK)
        rv = call.scene(s, flags, radiance ? rtamd::pick_radiance_variant : rtamd::pick_query_variant, kv, S,
                        depth ? &at_depth : nullptr);
    if (rv == RT_OK && radiance) rv = call.counters();
    if (rv != RT_OK) return rv;
    if (depth) S.rec_limit = at_depth.recursion_limit;
    Workspace& ws = *call.ws;
    QueryBuffers& q = ws.q;
    const rtamd::CompiledScene& cs = ws.scene.sc.cs;
    // RT_FLAG_RAY_BVH: the ray-BVH row of the variant where the scene has the tree (frame_plan.hpp use_ray_bvh)
    const bool ray_bvh = !radiance && rtamd::use_ray_bvh(cs, kv, flags);
    if (ray_bvh) {
        rv = ray_bvh_resident(ws, st);
        if (rv != RT_OK) return rv;
    }
    const size_t chunk = host ? std::min(n, g_chunk_items.load()) : n;
    if (host) {
        HIP_TRY(q.rays.ensure(chunk * sizeof(rt_ray)));
        if (isect) HIP_TRY(q.hits.ensure(chunk * sizeof(rt_hit)));
        if (mask) HIP_TRY(q.mask.ensure(chunk));
        if (radiance) HIP_TRY(q.rgb.ensure(chunk * 3 * sizeof(double)));
    }
    // a chunk on the device: the staging buffers, or the caller's (one chunk)
    const rt_ray* d_rays = host ? q.rays.as<rt_ray>() : rays;
    rt_hit* d_hits = !isect ? nullptr : host ? q.hits.as<rt_hit>() : hits;
    uint8_t* d_mask = !mask ? nullptr : host ? q.mask.as<uint8_t>() : mask;
    double* d_rgb = !radiance ? nullptr : host ? q.rgb.as<double>() : rgb;
    rv = call.run(
        n, chunk, kLaunchItems,
        [&](size_t c0, size_t cn) -> int {
            if (host) HIP_TRY(hipMemcpyAsync(q.rays.p, rays + c0, cn * sizeof(rt_ray), hipMemcpyHostToDevice, st));
            return RT_OK;
        },
        [&](size_t, size_t l0, size_t ln) -> int {
            if (radiance) {
                RadianceParams P;
                P.n = ln;
                P.rays = d_rays + l0;
                P.rgb = d_rgb + 3 * l0;
                P.counters = ws.frame.counters.as<unsigned long long>();
                HIP_TRY(rtamd::launch_radiance(kv, st, S, P));
            } else if (ray_bvh) {
                rtamd::RayBvhParams P{};
                P.n = ln;
                P.rays = d_rays + l0;
                P.hits = d_hits ? d_hits + l0 : nullptr;
                P.mask = d_mask ? d_mask + l0 : nullptr;
                P.nodes = ws.scene.rnodes.as<rtamd::RayBvhNode>();
                P.n_nodes = (int)cs.rnodes.size();
                P.n_lead = cs.rlead;
                HIP_TRY(rtamd::launch_ray_bvh(kv, kind, st, S, P));
            } else {
                QueryParams P;
                P.n = ln;
                P.rays = d_rays + l0;
                P.hits = d_hits ? d_hits + l0 : nullptr;
                P.mask = d_mask ? d_mask + l0 : nullptr;
                HIP_TRY(rtamd::launch_query(kv, kind, st, S, P));
            }
            return RT_OK;
        },
        [&](size_t c0, size_t cn) -> int {
            if (!host) return RT_OK;
            if (isect) HIP_TRY(hipMemcpyAsync(hits + c0, d_hits, cn * sizeof(rt_hit), hipMemcpyDeviceToHost, st));
            if (mask) HIP_TRY(hipMemcpyAsync(mask + c0, d_mask, cn, hipMemcpyDeviceToHost, st));
            if (radiance) HIP_TRY(hipMemcpyAsync(rgb + 3 * c0, d_rgb, cn * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
            return RT_OK;
        });
    if (rv == RT_OK) rv = call.finish();
    if (rv != RT_OK || !stats) return rv;
    stats->rays_intersect = radiance ? call.ctr(0) : isect ? n : 0;
    stats->rays_occluded = radiance ? call.ctr(1) : isect ? 0 : n;
    stats->rays_traced = stats->rays_intersect + stats->rays_occluded;
    return RT_OK;
}

// rt_query_shade[_device]: shade_lambert_phong of n caller-given hits.  host:
// hits / wo / mask / rgb are host memory, moved through the workspace's chunk
// buffers; else device memory, shaded in place on st.  lights / miss_rgb are
// host memory in both forms.  n_lights >= 0: the call's own point lights, in a
// workspace buffer of their own (uploaded through the page-locked arena);
// only this call's SceneView points there, so the resident scene (its lights,
// the scene cache) is what it was.  The Scene::occluded calls are counted.
int shade_impl(const char* what, const rt_scene* s, const rt_hit* hits, const double* wo, const uint8_t* mask, size_t n,
               const rt_light* lights, int n_lights, const double* miss_rgb, int flags, double* rgb, bool host,
               hipStream_t st, rt_stats* stats) {
    BatchCall call(what, st);
    int rv = call.check_scene_flags(s, flags);
    if (rv != RT_OK) return rv;
    call.zero_stats(stats);
    if (n == 0) return RT_OK;
    if (!hits) return call.fail("hits is NULL", RT_ERR_INVALID_ARG);
    if (!wo) return call.fail("wo is NULL", RT_ERR_INVALID_ARG);
    if (!rgb) return call.fail("the result buffer is NULL", RT_ERR_INVALID_ARG);
    if (n_lights > 0 && !lights) return call.fail("lights is NULL with n_lights > 0", RT_ERR_INVALID_ARG);
    rtamd::KernelVariant kv;
    SceneView S;
    rv = call.open();
    if (rv == RT_OK) rv = call.scene(s, flags, rtamd::pick_shade_variant, kv, S);
    if (rv != RT_OK) return rv;
    Workspace& ws = *call.ws;
    QueryBuffers& q = ws.q;
    if (n_lights >= 0) {
        // this call's point lights: k_shade (WV = 0) reads nothing else by light number
        HIP_TRY(q.lights.ensure(n_lights ? (size_t)n_lights * sizeof(rt_light) : 16));
        HIP_TRY(rtamd::upload_async(&ws.up, q.lights.p, lights, (size_t)n_lights * sizeof(rt_light), st));
        S.lights = q.lights.p;
        S.n_lights = n_lights;
    }
    rv = call.counters();
    if (rv != RT_OK) return rv;
    const size_t chunk = host ? std::min(n, g_chunk_items.load()) : n;
    if (host) {
        HIP_TRY(q.hits.ensure(chunk * sizeof(rt_hit)));
        HIP_TRY(q.wo.ensure(chunk * 3 * sizeof(double)));
        if (mask) HIP_TRY(q.mask.ensure(chunk));
        HIP_TRY(q.rgb.ensure(chunk * 3 * sizeof(double)));
    }
    // a chunk on the device: the staging buffers, or the caller's (one chunk)
    ShadeParams P0;
    P0.hits = host ? q.hits.as<rt_hit>() : hits;
    P0.wo = host ? q.wo.as<double>() : wo;
    P0.mask = !mask ? nullptr : host ? q.mask.as<uint8_t>() : mask;
    P0.rgb = host ? q.rgb.as<double>() : rgb;
    for (int c = 0; c < 3; ++c) P0.miss[c] = miss_rgb ? miss_rgb[c] : rt_scene_get_desc(s)->background[c];
    P0.counters = ws.frame.counters.as<unsigned long long>();
    rv = call.run(
        n, chunk, kLaunchItems,
        [&](size_t c0, size_t cn) -> int {
            if (!host) return RT_OK;
            HIP_TRY(hipMemcpyAsync(q.hits.p, hits + c0, cn * sizeof(rt_hit), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(q.wo.p, wo + 3 * c0, cn * 3 * sizeof(double), hipMemcpyHostToDevice, st));
            if (mask) HIP_TRY(hipMemcpyAsync(q.mask.p, mask + c0, cn, hipMemcpyHostToDevice, st));
            return RT_OK;
        },
        [&](size_t, size_t l0, size_t ln) -> int {
            ShadeParams P = P0;
            P.n = ln;
            P.hits += l0;
            P.wo += 3 * l0;
            if (P.mask) P.mask += l0;
            P.rgb += 3 * l0;
            HIP_TRY(rtamd::launch_shade(kv, st, S, P));
            return RT_OK;
        },
        [&](size_t c0, size_t cn) -> int {
            if (host) HIP_TRY(hipMemcpyAsync(rgb + 3 * c0, P0.rgb, cn * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
            return RT_OK;
        });
    if (rv == RT_OK) rv = call.finish();
    if (rv != RT_OK || !stats) return rv;
    stats->rays_occluded = call.ctr(1);
    stats->rays_traced = stats->rays_occluded;
    return RT_OK;
}

// ------------------------------------------------------------ node queries
// rt_query_node_{intersect,interval}[_device]: kind rtamd::kNodeIsect (enter:
// the hits; ex unused) / kNodeIvl (enter / ex: the enterHit / exitHit records).
// host: rays and results are host memory, moved through the workspace's chunk
// buffers (the ray queries' rays / hits / mask, and exit); else device memory,
// evaluated in place on st.
int node_impl(const char* what, const rt_scene* s, int node, int kind, const rt_ray* rays, size_t n, int flags,
              rt_hit* enter, rt_hit* ex, uint8_t* mask, bool host, hipStream_t st, rt_stats* stats) {
    BatchCall call(what, st);
    const bool isect = kind == rtamd::kNodeIsect;
    int rv = call.check_scene_flags(s, flags);
    if (rv != RT_OK) return rv;
    const rt_scene_desc& d = *rt_scene_get_desc(s);
    if (node < 0 || node >= d.n_nodes) return call.fail("node is outside [0, n_nodes)", RT_ERR_INVALID_ARG);
    call.zero_stats(stats);
    if (n == 0) return RT_OK;
    if (!rays) return call.fail("rays is NULL", RT_ERR_INVALID_ARG);
    if (isect ? !enter : (!enter && !ex && !mask)) return call.fail("the result buffer is NULL", RT_ERR_INVALID_ARG);
    rv = call.open();
    if (rv != RT_OK) return rv;
    Workspace& ws = *call.ws;
    QueryBuffers& q = ws.q;
    rv = scene_resident(ws, s, d, false, st);
    const NodeProg* np = nullptr;
    if (rv == RT_OK) rv = node_program_resident(ws, d, node, kind, flags, st, &np);
    if (rv != RT_OK) return rv;
    SceneView S;
    scene_view(ws, d, flags, S);
    S.n_chunks = 0;
    const size_t chunk = host ? std::min(n, g_chunk_items.load()) : n;
    if (host) {
        HIP_TRY(q.rays.ensure(chunk * sizeof(rt_ray)));
        if (enter) HIP_TRY(q.hits.ensure(chunk * sizeof(rt_hit)));
        if (ex) HIP_TRY(q.exit.ensure(chunk * sizeof(rt_hit)));
        if (mask) HIP_TRY(q.mask.ensure(chunk));
    }
    // a chunk on the device: the staging buffers, or the caller's (one chunk)
    const rt_ray* d_rays = host ? q.rays.as<rt_ray>() : rays;
    rt_hit* d_enter = !enter ? nullptr : host ? q.hits.as<rt_hit>() : enter;
    rt_hit* d_exit = !ex ? nullptr : host ? q.exit.as<rt_hit>() : ex;
    uint8_t* d_mask = !mask ? nullptr : host ? q.mask.as<uint8_t>() : mask;
    rv = call.run(
        n, chunk, kLaunchItems,
        [&](size_t c0, size_t cn) -> int {
            if (host) HIP_TRY(hipMemcpyAsync(q.rays.p, rays + c0, cn * sizeof(rt_ray), hipMemcpyHostToDevice, st));
            return RT_OK;
        },
        [&](size_t, size_t l0, size_t ln) -> int {
            NodeParams P;
            P.n = ln;
            P.rays = d_rays + l0;
            P.enter = d_enter ? d_enter + l0 : nullptr;
            P.exit = d_exit ? d_exit + l0 : nullptr;
            P.mask = d_mask ? d_mask + l0 : nullptr;
            P.ops = np->ops.as<rtamd::DevOp>();
            P.n_ops = (int)np->host.size();
            P.node = node;
            HIP_TRY(rtamd::launch_node(np->kv, kind, st, S, P));
            return RT_OK;
        },
        [&](size_t c0, size_t cn) -> int {
            if (!host) return RT_OK;
            if (enter) HIP_TRY(hipMemcpyAsync(enter + c0, d_enter, cn * sizeof(rt_hit), hipMemcpyDeviceToHost, st));
            if (ex) HIP_TRY(hipMemcpyAsync(ex + c0, d_exit, cn * sizeof(rt_hit), hipMemcpyDeviceToHost, st));
            if (mask) HIP_TRY(hipMemcpyAsync(mask + c0, d_mask, cn, hipMemcpyDeviceToHost, st));
            return RT_OK;
        });
    if (rv == RT_OK) rv = call.finish();
    if (rv != RT_OK || !stats) return rv;
    stats->rays_intersect = stats->rays_traced = n;   // (one primitive query per ray)
    return RT_OK;
}

// ------------------------------------------------------------- camera rays
// rt_camera_rays[_device]: the rays of list entries [0, n_rows) of a W x H
// frame seen through cam (k_camera_rays, rt_camera_f64.hip).  host: rays is
// host memory, filled through the workspace's ray staging buffer (the
// queries') in row chunks of at most g_chunk_items rays (at least one row);
// else device memory, written in place on st.  Jittered rays read the frames'
// draws (jitter_plan_ready / jitter_draws: the frames' plan, checkpoint table,
// cache key and fill), one acquisition for the whole list whatever the chunks.
int camera_rays_impl(const char* what, const rt_camera* cam, int W, int H, int kind, const int32_t* rows_host, int n_rows,
                     rt_ray* rays, bool host, hipStream_t st, rt_stats* stats) {
    BatchCall call(what, st);
    if (!cam) return call.fail("cam is NULL", RT_ERR_INVALID_ARG);
    if (W <= 0 || H <= 0) return call.fail("W and H must be > 0", RT_ERR_INVALID_ARG);
    if (kind != RT_RAYS_CENTRE && kind != RT_RAYS_JITTERED) return call.fail("unknown kind", RT_ERR_INVALID_ARG);
    if ((size_t)W * RT_SPP >= ((size_t)1 << 31)) return call.fail("W is beyond one launch's row", RT_ERR_INVALID_ARG);
    if (n_rows < 0 || n_rows > H) return call.fail("bad rows", RT_ERR_INVALID_ARG);
    if (!rows_host && n_rows != 0 && n_rows != H) return call.fail("rows is NULL with n_rows != H", RT_ERR_INVALID_ARG);
    const bool jittered = kind == RT_RAYS_JITTERED;
    std::vector<int32_t> all_rows;
    bool in_order = true;   // entry ri is row ri
    int rv = RT_OK;
    if (!rows_host) {
        all_rows.resize(n_rows);
        for (int r = 0; r < n_rows; ++r) all_rows[r] = r;
        rows_host = all_rows.data();
    } else if ((rv = check_rows(what, H, rows_host, n_rows, &in_order)) != RT_OK) {
        return rv;
    }
    call.zero_stats(stats);
    if (n_rows == 0) return RT_OK;
    if (!rays) return call.fail("the ray buffer is NULL", RT_ERR_INVALID_ARG);
    rv = call.open();
    if (rv != RT_OK) return rv;
    Workspace& ws = *call.ws;
    QueryBuffers& q = ws.q;
    hipEvent_t* ev = ws.sync.ev;
    rtamd::CameraParams P{};
    for (int i = 0; i < 3; ++i) {
        P.eye[i] = cam->eye[i];
        P.P[i] = cam->P[i];
    }
    P.Lx = cam->Lx;
    P.Ly = cam->Ly;
    P.cam_nx = rt_camera_width(cam);
    P.cam_ny = rt_camera_height(cam);
    P.W = W;
    P.H = H;
    rtamd::JitterCache::Entry* jent = nullptr;
    float ms_rng = 0.f;
    if (jittered) {
        rtamd::StdPlan plan;   // (host source of the rows upload: alive until st is drained)
        rv = jitter_plan_ready(ws, W, H, rows_host, n_rows, st, plan);
        if (rv != RT_OK) return rv;
        HIP_TRY(hipEventRecord(ev[0], st));
        bool filled = false;
        rv = jitter_draws(ws, what, W, H, n_rows, plan, st, &jent, &filled);
        if (rv != RT_OK) return rv;
        HIP_TRY(hipEventRecord(ev[1], st));
        // (the plan's vectors must outlive the upload: wait here, once per call)
        HIP_TRY(hipStreamSynchronize(st));
        if (filled) rtamd::note_launch("rtamd", "k_mt_fill_w");
        (void)hipEventElapsedTime(&ms_rng, ev[0], ev[1]);
        P.rows = jent->rows();
        P.jrow = jent->rows() + n_rows;
        P.jit = jent->jit();
    } else if (!in_order) {
        HIP_TRY(q.cam_rows.ensure((size_t)n_rows * sizeof(int32_t)));
        HIP_TRY(rtamd::upload_async(&ws.up, q.cam_rows.p, rows_host, (size_t)n_rows * sizeof(int32_t), st));
        P.rows = q.cam_rows.as<int32_t>();
    }
    const size_t per_row = (size_t)W * (jittered ? RT_SPP : 1);
    // list entries of one launch: the grid's y extent; of one host chunk: its rays
    const size_t launch_rows = 65535;
    const size_t chunk_rows = host ? std::min<size_t>(n_rows, std::max<size_t>(1, g_chunk_items.load() / per_row)) : n_rows;
    if (host) HIP_TRY(q.rays.ensure(chunk_rows * per_row * sizeof(rt_ray)));
    rt_ray* d_rays = host ? q.rays.as<rt_ray>() : rays;
    rv = call.run(
        n_rows, chunk_rows, launch_rows, BatchCall::no_staging,
        [&](size_t c0, size_t l0, size_t ln) -> int {
            P.ri0 = (int)(c0 + l0);
            P.n_rows = (int)ln;
            P.rays = d_rays + l0 * per_row;
            HIP_TRY(rtd::launch_camera_rays(jittered, st, P));
            return RT_OK;
        },
        [&](size_t c0, size_t cn) -> int {
            if (host) HIP_TRY(hipMemcpyAsync(rays + c0 * per_row, d_rays, cn * per_row * sizeof(rt_ray), hipMemcpyDeviceToHost, st));
            return RT_OK;
        });
    if (rv != RT_OK) return rv;
    // st has run to its end: the draws and the rows list this call wrote are
    // complete, and later frames or calls of its key may read them
    ws.frame.jcache.complete(jent);
    rv = call.finish();
    if (rv != RT_OK || !stats) return rv;
    stats->pixels = (uint64_t)n_rows * W;
    stats->ms_rng = ms_rng;
    return RT_OK;
}

// ------------------------------------------------------------- bounce loop
// rt_scatter_rays_device: the children of n parents (rays[i], hits[i]) at
// recursion depth `depth`, compacted in parent order (rt_bounce_f64.hip: count,
// scan, emit per launch group of g_scatter_items parents; the group's child
// total is read back and carried into the next group's first index).  Every
// buffer is device memory but n_children.  Reads the resident scene's
// materials, medium index and recursion limit and leaves the resident copy as
// it was.
int scatter_impl(const char* what, const rt_scene* s, const rt_ray* rays, const rt_hit* hits, const uint8_t* mask, size_t n,
                 int depth, uint8_t* spawn, uint64_t* first, rt_ray* child_rays, double* child_w, size_t child_cap,
                 size_t* n_children, hipStream_t st, rt_stats* stats) {
    BatchCall call(what, st);
    int rv = rtamd::scatter_check(what, s, rays, hits, mask, n, spawn, first, child_rays, child_w, child_cap, n_children,
                                  false);
    if (rv != RT_OK) return rv;
    call.zero_stats(stats);
    *n_children = 0;
    if (n == 0) return RT_OK;
    rv = call.open();
    if (rv != RT_OK) return rv;
    Workspace& ws = *call.ws;
    DBuf& tmp = ws.q.scatter_tmp;
    const rt_scene_desc& d = *rt_scene_get_desc(s);
    rv = scene_resident(ws, s, d, false, st);
    if (rv != RT_OK) return rv;
    const size_t group = std::min(std::max<size_t>(g_scatter_items.load(), 1), kLaunchItems);
    // [0, 8): the group's child total; behind it the scan's words
    HIP_TRY(tmp.ensure(8 + rtamd::scatter_count_words(std::min(n, group)) * sizeof(uint32_t)));
    rtamd::ScatterParams P0{};
    P0.mats = ws.scene.mats.p;
    P0.n_mats = d.n_materials;
    P0.can = rtamd::bounce_can_spawn(depth, d.recursion_limit) ? 1 : 0;
    P0.medium_index = d.medium_index;
    P0.child_rays = child_rays;
    P0.child_w = child_w;
    P0.child_cap = child_cap;
    P0.total = tmp.as<uint64_t>();
    P0.counts = tmp.as<uint32_t>() + 2;
    uint64_t m = 0;
    rv = call.run(
        n, n, group, BatchCall::no_staging,
        [&](size_t, size_t l0, size_t ln) -> int {
            rtamd::ScatterParams P = P0;
            P.rays = rays + l0;
            P.hits = hits + l0;
            P.mask = mask ? mask + l0 : nullptr;
            P.n = ln;
            P.spawn = spawn + l0;
            P.first = first + l0;
            P.base = m;
            HIP_TRY(rtd::launch_scatter(st, P));
            uint64_t got = 0;
            HIP_TRY(hipMemcpyAsync(&got, P.total, sizeof(got), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            m += got;
            return RT_OK;
        },
        BatchCall::no_staging);
    if (rv == RT_OK) rv = call.finish();
    if (rv != RT_OK) return rv;
    *n_children = (size_t)m;
    if (m > child_cap)
        return call.fail((std::to_string(m) + " children exceed child_cap " + std::to_string(child_cap)).c_str(),
                         RT_ERR_INVALID_ARG);
    return RT_OK;
}

}  // namespace

// ------------------------------------------------------------------ C-ABI
extern "C" int rt_query_intersect(const rt_scene* s, const rt_ray* rays_host, size_t n, int flags, rt_hit* hits_host,
                                  uint8_t* hit_mask_host, rt_stats* stats) {
    return query_impl("rt_query_intersect", s, rtamd::kQueryIsect, rays_host, n, flags, hits_host, hit_mask_host, nullptr,
                      true, nullptr, stats);
}

extern "C" int rt_query_occluded(const rt_scene* s, const rt_ray* rays_host, size_t n, int flags, uint8_t* occluded_host,
                                 rt_stats* stats) {
    return query_impl("rt_query_occluded", s, rtamd::kQueryOccl, rays_host, n, flags, nullptr, occluded_host, nullptr, true,
                      nullptr, stats);
}

extern "C" int rt_query_intersect_device(const rt_scene* s, const rt_ray* rays_dev, size_t n, int flags, rt_hit* hits_dev,
                                         uint8_t* hit_mask_dev, void* hip_stream, rt_stats* stats) {
    return query_impl("rt_query_intersect_device", s, rtamd::kQueryIsect, rays_dev, n, flags, hits_dev, hit_mask_dev,
                      nullptr, false, (hipStream_t)hip_stream, stats);
}

extern "C" int rt_query_occluded_device(const rt_scene* s, const rt_ray* rays_dev, size_t n, int flags,
                                        uint8_t* occluded_dev, void* hip_stream, rt_stats* stats) {
    return query_impl("rt_query_occluded_device", s, rtamd::kQueryOccl, rays_dev, n, flags, nullptr, occluded_dev, nullptr,
                      false, (hipStream_t)hip_stream, stats);
}

extern "C" int rt_query_node_intersect(const rt_scene* s, int node, const rt_ray* rays_host, size_t n, int flags,
                                       rt_hit* hits_host, uint8_t* hit_mask_host, rt_stats* stats) {
    return node_impl("rt_query_node_intersect", s, node, rtamd::kNodeIsect, rays_host, n, flags, hits_host, nullptr,
                     hit_mask_host, true, nullptr, stats);
}

extern "C" int rt_query_node_interval(const rt_scene* s, int node, const rt_ray* rays_host, size_t n, int flags,
                                      rt_hit* enter_host, rt_hit* exit_host, uint8_t* ok_mask_host, rt_stats* stats) {
    return node_impl("rt_query_node_interval", s, node, rtamd::kNodeIvl, rays_host, n, flags, enter_host, exit_host,
                     ok_mask_host, true, nullptr, stats);
}

extern "C" int rt_query_node_intersect_device(const rt_scene* s, int node, const rt_ray* rays_dev, size_t n, int flags,
                                              rt_hit* hits_dev, uint8_t* hit_mask_dev, void* hip_stream,
                                              rt_stats* stats) {
    return node_impl("rt_query_node_intersect_device", s, node, rtamd::kNodeIsect, rays_dev, n, flags, hits_dev, nullptr,
                     hit_mask_dev, false, (hipStream_t)hip_stream, stats);
}

extern "C" int rt_query_node_interval_device(const rt_scene* s, int node, const rt_ray* rays_dev, size_t n, int flags,
                                             rt_hit* enter_dev, rt_hit* exit_dev, uint8_t* ok_mask_dev, void* hip_stream,
                                             rt_stats* stats) {
    return node_impl("rt_query_node_interval_device", s, node, rtamd::kNodeIvl, rays_dev, n, flags, enter_dev, exit_dev,
                     ok_mask_dev, false, (hipStream_t)hip_stream, stats);
}

extern "C" int rt_query_radiance(const rt_scene* s, const rt_ray* rays_host, size_t n, int flags, double* rgb_host,
                                 rt_stats* stats) {
    return query_impl("rt_query_radiance", s, rtamd::kQueryRadiance, rays_host, n, flags, nullptr, nullptr, rgb_host, true,
                      nullptr, stats);
}

extern "C" int rt_query_radiance_device(const rt_scene* s, const rt_ray* rays_dev, size_t n, int flags, double* rgb_dev,
                                        void* hip_stream, rt_stats* stats) {
    return query_impl("rt_query_radiance_device", s, rtamd::kQueryRadiance, rays_dev, n, flags, nullptr, nullptr, rgb_dev,
                      false, (hipStream_t)hip_stream, stats);
}

extern "C" int rt_query_radiance_depth(const rt_scene* s, const rt_ray* rays_host, size_t n, int flags, int depth,
                                       double* rgb_host, rt_stats* stats) {
    return query_impl("rt_query_radiance_depth", s, rtamd::kQueryRadiance, rays_host, n, flags, nullptr, nullptr, rgb_host,
                      true, nullptr, stats, &depth);
}

extern "C" int rt_query_radiance_depth_device(const rt_scene* s, const rt_ray* rays_dev, size_t n, int flags, int depth,
                                              double* rgb_dev, void* hip_stream, rt_stats* stats) {
    return query_impl("rt_query_radiance_depth_device", s, rtamd::kQueryRadiance, rays_dev, n, flags, nullptr, nullptr,
                      rgb_dev, false, (hipStream_t)hip_stream, stats, &depth);
}

extern "C" int rt_scatter_rays_device(const rt_scene* s, const rt_ray* rays_dev, const rt_hit* hits_dev,
                                      const uint8_t* hit_mask_dev, size_t n, int depth, uint8_t* spawn_dev,
                                      uint64_t* first_dev, rt_ray* child_rays_dev, double* child_w_dev, size_t child_cap,
                                      size_t* n_children_host, void* hip_stream, rt_stats* stats) {
    return scatter_impl("rt_scatter_rays_device", s, rays_dev, hits_dev, hit_mask_dev, n, depth, spawn_dev, first_dev,
                        child_rays_dev, child_w_dev, child_cap, n_children_host, (hipStream_t)hip_stream, stats);
}

extern "C" int rt_combine_bounce_device(double* rgb_dev, const uint8_t* spawn_dev, const uint64_t* first_dev, size_t n,
                                        const double* child_rgb_dev, const double* child_w_dev, size_t n_children,
                                        void* hip_stream) {
    const int rc = rtamd::combine_check("rt_combine_bounce_device", rgb_dev, spawn_dev, first_dev, n, child_rgb_dev,
                                        child_w_dev, n_children);
    if (rc != RT_OK || !n) return rc;
    rtamd::CombineParams P;
    P.rgb = rgb_dev;
    P.spawn = spawn_dev;
    P.first = first_dev;
    P.n = n;
    P.child_rgb = child_rgb_dev;
    P.child_w = child_w_dev;
    P.n_children = n_children;
    HIP_TRY(rtd::launch_combine_bounce((hipStream_t)hip_stream, P));
    HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
    return RT_OK;
}

extern "C" int rt_query_shade(const rt_scene* s, const rt_hit* hits_host, const double* wo_host,
                              const uint8_t* hit_mask_host, size_t n, const rt_light* lights, int n_lights,
                              const double* miss_rgb, int flags, double* rgb_host, rt_stats* stats) {
    return shade_impl("rt_query_shade", s, hits_host, wo_host, hit_mask_host, n, lights, n_lights, miss_rgb, flags,
                      rgb_host, true, nullptr, stats);
}

extern "C" int rt_query_shade_device(const rt_scene* s, const rt_hit* hits_dev, const double* wo_dev,
                                     const uint8_t* hit_mask_dev, size_t n, const rt_light* lights, int n_lights,
                                     const double* miss_rgb, int flags, double* rgb_dev, void* hip_stream,
                                     rt_stats* stats) {
    return shade_impl("rt_query_shade_device", s, hits_dev, wo_dev, hit_mask_dev, n, lights, n_lights, miss_rgb, flags,
                      rgb_dev, false, (hipStream_t)hip_stream, stats);
}

extern "C" int rt_camera_rays_device(const rt_camera* cam, int W, int H, int kind, const int32_t* rows_host, int n_rows,
                                     rt_ray* rays_dev, void* hip_stream, rt_stats* stats) {
    return camera_rays_impl("rt_camera_rays_device", cam, W, H, kind, rows_host, n_rows, rays_dev, false,
                            (hipStream_t)hip_stream, stats);
}

extern "C" int rt_camera_rays(const rt_camera* cam, int W, int H, int kind, const int32_t* rows_host, int n_rows,
                              rt_ray* rays_host, rt_stats* stats) {
    return camera_rays_impl("rt_camera_rays", cam, W, H, kind, rows_host, n_rows, rays_host, true, nullptr, stats);
}

extern "C" int rt_resolve_samples_device(const double* rgb_dev, size_t n_pixels, int spp, double* fb_dev,
                                         void* hip_stream) {
    const auto fail = [](const char* msg) {
        rtamd::set_last_error(std::string("rt_resolve_samples_device: ") + msg);
        return (int)RT_ERR_INVALID_ARG;
    };
    if (spp < 1 || spp > 64) return fail("spp must be in [1, 64]");
    if (!n_pixels) return RT_OK;
    if (!rgb_dev || !fb_dev) return fail("NULL buffer");
    const uintptr_t a = reinterpret_cast<uintptr_t>(rgb_dev), b = reinterpret_cast<uintptr_t>(fb_dev);
    if (b < a + n_pixels * spp * 3 * sizeof(double) && a < b + n_pixels * 3 * sizeof(double)) return fail("fb overlaps rgb");
    rtamd::ResolveParams P;
    P.rgb = rgb_dev;
    P.n_pixels = n_pixels;
    P.spp = spp;
    P.fb = fb_dev;
    HIP_TRY(rtd::launch_resolve_samples((hipStream_t)hip_stream, P));
    HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
    return RT_OK;
}

extern "C" int rt_rays_wo_device(const rt_ray* rays_dev, size_t n, double* wo_dev, void* hip_stream) {
    const int rc = rtamd::rays_wo_check("rt_rays_wo_device", rays_dev, n, wo_dev);
    if (rc != RT_OK || !n) return rc;
    rtamd::RaysWoParams P;
    P.rays = rays_dev;
    P.n = n;
    P.wo = wo_dev;
    HIP_TRY(rtd::launch_rays_wo((hipStream_t)hip_stream, P));
    HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
    return RT_OK;
}

// rt_paper_resolve_device: k_paper_resolve (rt_paper_f64.hip) over the
// caller's device buffers.  No scene: nothing is uploaded and the resident
// scene copy is not touched.  A batched call (BatchCall: the workspace's
// events time the kernel) of one chunk and one launch.
extern "C" int rt_paper_resolve_device(const rt_hit* hits_dev, const uint8_t* hit_mask_dev, const double* rgb_dev, int W,
                                       int H, int row0, int n_rows, double* fb_dev, double* edge_dev, void* hip_stream,
                                       rt_stats* stats) {
    const hipStream_t st = (hipStream_t)hip_stream;
    BatchCall call("rt_paper_resolve_device", st);
    int rc = rtamd::paper_resolve_check(call.what, hits_dev, hit_mask_dev, rgb_dev, W, H, row0, n_rows, fb_dev, edge_dev);
    if (rc != RT_OK) return rc;
    call.zero_stats(stats);
    if (n_rows == 0) return RT_OK;
    rc = call.open();
    if (rc != RT_OK) return rc;
    rtamd::PaperResolveParams P;
    P.hits = hits_dev;
    P.mask = hit_mask_dev;
    P.rgb = rgb_dev;
    P.W = W;
    P.H = H;
    P.row0 = row0;
    P.n_rows = n_rows;
    P.fb = fb_dev;
    P.edge = edge_dev;
    rc = call.run(
        n_rows, n_rows, n_rows, BatchCall::no_staging,
        [&](size_t, size_t, size_t) -> int {
            HIP_TRY(rtd::launch_paper_resolve(st, P));
            return RT_OK;
        },
        BatchCall::no_staging);
    if (rc == RT_OK) rc = call.finish();
    if (rc == RT_OK && stats) stats->pixels = (uint64_t)n_rows * W;
    return rc;
}
