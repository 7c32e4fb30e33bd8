// rt_render.hip — gfx950 render kernels and the librtamd C-ABI.
//
// Standard mode (Tracer::render, tracer.cpp:282-300):
//   k_std: one lane per (pixel, sample); a wave covers 4x2 pixels x 8 samples,
//   a 256-thread block 8x4 pixels.  Samples are summed in order s = 0..7
//   across the 8 lanes of a pixel (cross-lane shuffles), then x 1/8.
// Paper mode (tracer.cpp:258-281):
//   k_paper_primary: one lane per pixel: the primary intersect (shared by
//   trace_paper, the centre probe and the four neighbour probes of
//   get_edge_strength, which all re-trace identical rays) + shading.
//   k_paper_finish: edge strength from the stored neighbour hits + hatch.
// What a frame launches and over which rows is decided in host-only code
// (csrc/host/frame_plan.hpp: pick_variant, plan_std_frame, plan_paper_frame,
// PaperCalls); rt_frame_begin / trace / end here execute that plan.  The
// rt_test_* hooks live in rt_test_hooks.hip.
// The batched entry points run on the frames' workspace through one driver
// (BatchCall: lock, drain, staging arena, counters, chunk loop):
// Ray queries (rt_query_intersect / rt_query_occluded, Scene::intersect /
// Scene::occluded for caller-given rays, scene.cpp:10-42): query_impl, on the
// resident scene; kernels in rt_query_kernels.hpp.
// Radiance queries (rt_query_radiance, Tracer::trace for caller-given rays,
// tracer.cpp:12-73): the same query_impl, with the frames' ray counters;
// kernels in rt_radiance_kernels.hpp.
// Shading queries (rt_query_shade, shade_lambert_phong for caller-given hits,
// shading.cpp:31-138): shade_impl next to it; kernels in rt_shade_kernels.hpp.
// Camera rays and sample resolve (rt_camera_rays / rt_resolve_samples_device,
// camera.h:44-78 and tracer.cpp:291-296): camera_rays_impl, on the frames'
// jitter draws (jitter_plan_ready / jitter_draws, shared with frame_begin);
// kernels in rt_camera_f64.hip.  Paper resolve: rt_paper_resolve_device.
// Node queries (rt_query_node_intersect / rt_query_node_interval,
// Primitive::intersect / ::interval of one node, geometry.h:62-75): node_impl,
// on the resident scene plus the node's own program (node_program_resident);
// kernels in rt_node_kernels.hpp.
// Bounce loop (rt_scatter_rays_device / rt_combine_bounce_device, the spawn and
// the unwind half of Tracer::trace_recursive, tracer.cpp:34-67): scatter_impl on
// the resident scene's materials; kernels in rt_bounce_f64.hip.
// rt_query_radiance_depth is query_impl with the remaining depth for its limit.
#include <hip/hip_runtime.h>

#include <cstdio>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "jitter_cache.hpp"
#include "mt_jump.hpp"
#include "pinned.hpp"
#include "mt_poly.hpp"
#include "rt.h"
#include "rt_bounce.hpp"
#include "rt_camera.hpp"
#include "rt_paper.hpp"
#include "rt_devbuf.hpp"
#include "rt_launch.hpp"
#include "rt_internal.hpp"
#include "rt_test.h"
#include "scene_compile.hpp"

using rtamd::kCounterSlots;
using rtamd::kCounterWords;
using rtamd::NodeParams;
using rtamd::PaperParams;
using rtamd::QueryParams;
using rtamd::RadianceParams;
using rtamd::SceneView;
using rtamd::ShadeParams;
using rtamd::StdParams;

namespace {

__global__ void k_scatter_rows(const double* __restrict__ src, const int32_t* __restrict__ rows, int n_rows, int W,
                               double* __restrict__ dst) {
    const size_t row_len = (size_t)W * 3;
    const size_t total = row_len * n_rows;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / row_len, k = i - r * row_len;
        const int32_t d = rows[r];
        if (d >= 0) dst[(size_t)d * row_len + k] = src[i];
    }
}

__global__ void k_to_rgb8(const double* __restrict__ fb, size_t n, uint8_t* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const double v = fb[i];
        double c = (v < 1.0) ? v : 1.0;   // std::min(1.0, v)
        c = (0.0 < c) ? c : 0.0;          // std::max(0.0, .)
        out[i] = (uint8_t)(int)round(c * 255.0);   // round half away from zero (core.h:316)
    }
}

// The frame's op counters: kCounterSlots x kCounterWords partial sums reduced
// on the device and stored straight into page-locked host memory, so that
// rt_frame_end reads 144 B after one event instead of copying 72 KiB through
// the runtime's pageable staging (which waited ~115 us after the last kernel
// before the copy even started: profiles/r04t_api_timeline.txt).
__global__ void __launch_bounds__(64) k_reduce_counters(unsigned long long* __restrict__ slots,
                                                        unsigned long long* __restrict__ out,
                                                        const unsigned int* __restrict__ gtime, int wpg) {
    // block k < kCounterWords sums word k over the slots (8 independent loads
    // per lane); block kCounterWords + g sums paper-mode list group g's wave
    // times (end - start, mod 2^32) over its wpg waves
    const int k = blockIdx.x, lane = threadIdx.x;
    if (k >= rtamd::kCounterWords) {
        const size_t g = k - rtamd::kCounterWords;
        unsigned v = 0;
        for (int xt = lane; xt < wpg; xt += 64) {
            const unsigned* t = gtime + 2 * (g * wpg + xt);
            v += t[1] - t[0];
        }
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) reinterpret_cast<unsigned int*>(out + rtamd::kCounterWords)[g] = v;
        return;
    }
    // (and leaves the slots zero for the next frame: Workspace::counters_zero)
    unsigned long long v = 0;
#pragma unroll
    for (int sl = lane; sl < rtamd::kCounterSlots; sl += 64) {
        unsigned long long* w = slots + (size_t)sl * rtamd::kCounterWords + k;
        v += *w;
        *w = 0ull;
    }
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) out[k] = v;
}

// ------------------------------------------------------------ host side
using DBuf = rtamd::DevBufT<8>;   // (growth slack 1/8)

// The device-resident copy of one scene (compiled object table + records in
// the launching precision).  A scene handle is immutable, so the copy is
// keyed by its process-unique id and reused by every later frame of that
// scene on the device: the inputs stay resident in HBM between frames.
struct SceneCache {
    bool valid = false;
    uint64_t uid = 0;
    // Wave BVH on or off, decided per scene by measurement (scenes that have
    // one: > kWaveBvhMin objects).  Exact either way (the BVH kernels equal
    // the flat-list ones bit for bit), so the first frame of a frame shape
    // runs with the BVH, the second without, and later frames take the one
    // whose trace kernels were faster: a scene bound by its closest-hit ties
    // ran 0.85x with the BVH (profiles/r04fin_bvh_perf.txt).
    int bvh_trial = 0;       // 0: next frame tries the BVH, 1: tries without, 2: decided
    float bvh_ms[2] = {0.f, 0.f};
    bool bvh_off = false;
    uint64_t bvh_key = 0;    // frame shape of the trial (W, H, mode, rows, flags)
    bool fp32 = false;
    rtamd::CompiledScene cs;
    std::vector<rt_node> nodes;   // host sources of the uploads (kept alive)
    std::vector<rt_material> mats;
    std::vector<rt_light> lights;
    std::vector<rt_dir_light> dlights;
    std::vector<rtamd::NodeR<float>> nodes_f;
    std::vector<rtamd::MatR<float>> mats_f;
    std::vector<rtamd::LightR<float>> lights_f;
    std::vector<rtamd::DLightR<float>> dlights_f;
    std::vector<rtamd::FoldLeafR<float>> fold_f;
};

// RT_BVH_AB (measurement A/B; default 1): 0 = a scene with a wave BVH always
// uses it (no trial frames, SceneCache::bvh_trial).
bool bvh_ab() {
    static const bool on = [] { const char* e = std::getenv("RT_BVH_AB"); return !(e && *e == '0'); }();
    return on;
}

// Device memory of the jitter cache's buffers (jitter_cache.hpp), on the
// current device.  A failed allocation is the cache's to handle (it frees
// entries or takes the uncached buffer), so the runtime's last-error slot is
// cleared: a later launch check must not report it.
void* jitter_alloc(size_t bytes) {
    void* p = nullptr;
    rtamd::SetupTimer tm(rtamd::kSetupAlloc);
    if (hipMalloc(&p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}
void jitter_free(void* p) { (void)hipFree(p); }

// One node's compiled program (compile_node_program) next to the resident
// scene: built and uploaded by the first query of (node, kind), found there by
// every later one.  A leaf has no ops (its row reads the node itself).
struct NodeProg {
    rtamd::KernelVariant kv;          // pick_node_variant: the row and its namespace
    std::vector<rtamd::DevOp> host;   // source of the upload (kept alive)
    DBuf ops;
};

// Per-device workspace (one render at a time per device; guarded by a mutex).
struct Workspace {
    std::mutex mu;
    DBuf nodes, mats, lights, dlights, objs, ops, gb, ctab, lrec, lwrec, lgb;
    DBuf wobjs, wctab, worig, wchunk;   // wave BVH (CompiledScene::wobjs ...)
    DBuf fold;
    DBuf nodes_f, mats_f, lights_f, dlights_f, fold_f;   // float copies (RT_FLAG_FP32)
    // standard mode: the frames' jitter draws and rows lists, resident by
    // (W, H, rows) so that only the first frame of a key generates them
    rtamd::JitterCache jcache{jitter_alloc, jitter_free};
    DBuf ckpt, jscratch, counters;
    DBuf paper_i, paper_d, paper_aux, fb;
    DBuf q_rays, q_hits, q_mask, q_rgb;       // ray queries from host memory: one chunk's rays / hits / flags / colours
    DBuf q_wo;                                // shading queries from host memory: one chunk's view directions
    DBuf q_exit;                              // node interval queries from host memory: one chunk's exit records
    // node queries: the programs of the resident scene's nodes queried so far, by
    // (node, kind); emptied with the resident scene (release_node_programs)
    std::map<std::pair<int, int>, NodeProg> node_progs;
    // ray queries with RT_FLAG_RAY_BVH: the resident scene's ray BVH
    // (CompiledScene::rnodes), uploaded by the first such query of the scene
    // and emptied with it (release_ray_bvh)
    DBuf rnodes;
    bool rnodes_resident = false;
    DBuf q_lights;                            // a shading query's own point lights (never the resident scene's `lights`)
    DBuf cam_rows;                            // rt_camera_rays, centre rays: a rows list that is not 0, 1, 2, ...
    DBuf scatter_tmp;                         // rt_scatter_rays_device: a launch group's child total + its scan's words
    rtamd::JitterTable jtab;                  // mt19937(12345) checkpoint table (resident)
    rtamd::JitterJob jjob;
    rtamd::PinnedArena up;                    // page-locked staging of a frame's uploads (pinned.hpp)
    DBuf gtime;                               // paper mode: primary waves' (start, end) ticks (paper_wave_slot)
    unsigned long long* ctr_host = nullptr;   // page-locked: the frame's reduced counters (k_reduce_counters)
    size_t ctr_host_words = 0;                //   + the paper-mode list-group costs behind them
    // paper mode: measured primary-pass cost of each 8-entry list group of a
    // frame, by the group's first ext index, per frame key (scene, size,
    // mode, flags, rows): the next frame of that key launches its groups
    // costliest first (frame_plan.hpp order_paper_groups)
    std::map<uint64_t, std::vector<uint32_t>> paper_cost;
    bool counters_zero = false;         // the last frame's k_reduce_counters left `counters` zero (no memset)
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<hipEvent_t> tev;   // one per rt_frame_trace call of the open frame (pool)
    std::vector<hipEvent_t> pev;   // paper mode: the end of each call's primary pass (pool)
    hipStream_t aux_st = nullptr;  // render_rows_impl: a paper frame's odd chunks
    SceneCache sc;
};

// Workspaces by (device, slot).  Slot 0 is the process's own; the simulated
// ranks of rt_test_dist_threads run on one device concurrently, each on its
// own host thread with its own slot (rtamd::set_workspace_slot), as separate
// processes would hold separate workspaces.  Never deleted (frames hold
// pointers); emptied by rt_shutdown.
std::mutex g_ws_mu;
std::map<std::pair<int, int>, Workspace*> g_ws;
thread_local int t_ws_slot = 0;

Workspace& workspace(int dev) {
    std::lock_guard<std::mutex> lk(g_ws_mu);
    Workspace*& w = g_ws[{dev, t_ws_slot}];
    if (!w) w = new Workspace;
    return *w;
}

// One-time setup costs of this process (rt_setup_times): host wall time of
// the scene compile + upload enqueue, the jitter checkpoint-table builds, and
// the first launch of the trace kernels and of the jitter fill (a code
// object is loaded onto the device at its first kernel launch).
struct SetupTimes {
    std::mutex mu;
    double scene_ms = 0.0, jtable_ms = 0.0, trace_launch_ms = 0.0, jitter_launch_ms = 0.0;
    double extra[rtamd::kSetupSlots] = {};   // rtamd::note_setup_ms slots (4..)
    bool trace_launched = false, jitter_launched = false;
};
SetupTimes g_setup;
using SClock = std::chrono::steady_clock;
double ms_since(SClock::time_point t) { return std::chrono::duration<double, std::milli>(SClock::now() - t).count(); }

// rt_render's staging frame (host-output path), one per process
std::mutex g_fb_mu;
DBuf g_fb;
int g_fb_dev = 0;

template <class T>
hipError_t upload(DBuf& b, const std::vector<T>& v, hipStream_t st, rtamd::PinnedArena* up = nullptr) {
    size_t bytes = v.size() * sizeof(T);
    hipError_t e = b.ensure(bytes ? bytes : 16);
    if (e != hipSuccess || !bytes) return e;
    return rtamd::upload_async(up, b.p, v.data(), bytes, st);
}

}  // namespace

// One frame in flight on one device (rt_frame_begin .. rt_frame_end).  Holds
// the device workspace lock for its lifetime; every launch is stream-ordered
// on `st`, and every host buffer an async upload reads stays alive here
// until rt_frame_end has synchronised the stream.
struct rt_frame {
    Workspace* ws = nullptr;
    std::unique_lock<std::mutex> lock;
    hipStream_t st = nullptr;
    SceneView S;
    int W = 0, H = 0, mode = 0, n_rows = 0;
    rtamd::KernelVariant kv;                   // the frame's trace kernel (frame_plan.hpp pick_variant)
    bool fp32 = false;
    bool timed = false;                        // paper mode: a launch stored its waves' ticks (PaperParams::gtime)
    int bvh_trial = -1;                        // SceneCache::bvh_trial this frame measures (-1: none)
    std::chrono::steady_clock::time_point t_start;
    rtamd::StdPlan std_plan;                   // standard mode (host source of the rows upload)
    rtamd::JitterCache::Entry* jent = nullptr; //   its buffer in ws->jcache (valid once this frame has ended well)
    const double* jit = nullptr;               //   the draws, 16 per pixel by jitter row
    const int32_t* rows = nullptr;             //   rows | jitter row of each, on the device
    rtamd::PaperPlan paper;                    // paper mode (host source of the aux upload)
    rtamd::PaperCalls paper_calls;             //   its trace calls' lists (host sources of their uploads)
    std::vector<hipStream_t> call_st;          // stream of each trace call (ws.tev[i] its end)
};

namespace {

template <size_t N>
void to_float(float (&dst)[N], const double (&src)[N]) {
    for (size_t i = 0; i < N; ++i) dst[i] = (float)src[i];
}

// Float copies of the scene records for the FP32 kernels (RT_FLAG_FP32).
void make_float_scene(SceneCache& f) {
    f.nodes_f.resize(f.nodes.size());
    for (size_t i = 0; i < f.nodes.size(); ++i) {
        const rt_node& s = f.nodes[i];
        rtamd::NodeR<float>& o = f.nodes_f[i];
        o.kind = s.kind;
        o.a = s.a;
        o.b = s.b;
        o.op = s.op;
        o.mat = s.mat;
        for (int k = 0; k < 5; ++k) o.mats[k] = s.mats[k];
        to_float(o.v, s.v);
        to_float(o.aux, s.aux);
    }
    f.mats_f.resize(f.mats.size());
    for (size_t i = 0; i < f.mats.size(); ++i) {
        const rt_material& s = f.mats[i];
        rtamd::MatR<float>& o = f.mats_f[i];
        to_float(o.albedo, s.albedo);
        to_float(o.ambient, s.ambient);
        o.kd = (float)s.kd;
        o.ks = (float)s.ks;
        o.kr = (float)s.kr;
        o.kt = (float)s.kt;
        o.shininess = (float)s.shininess;
        o.refractive_index = (float)s.refractive_index;
    }
    f.lights_f.resize(f.lights.size());
    for (size_t i = 0; i < f.lights.size(); ++i) {
        to_float(f.lights_f[i].pos, f.lights[i].pos);
        to_float(f.lights_f[i].intensity, f.lights[i].intensity);
    }
    f.dlights_f.resize(f.dlights.size());
    for (size_t i = 0; i < f.dlights.size(); ++i) {
        to_float(f.dlights_f[i].dir, f.dlights[i].dir);
        to_float(f.dlights_f[i].radiance, f.dlights[i].radiance);
    }
    f.fold_f.resize(f.cs.fold.size());
    for (size_t i = 0; i < f.cs.fold.size(); ++i) {
        to_float(f.fold_f[i].c, f.cs.fold[i].c);
        f.fold_f[i].r = (float)f.cs.fold[i].r;
        f.fold_f[i].pc = f.cs.fold[i].pc;
        f.fold_f[i].pad = 0;
    }
}

// The node programs belong to the resident scene: they go when it goes.  (No
// launch reads them then: a call that used one has drained its stream.)
void release_node_programs(Workspace& ws) {
    for (auto& kv : ws.node_progs) kv.second.ops.release();
    ws.node_progs.clear();
}

// The ray BVH belongs to the resident scene as the node programs do.
void release_ray_bvh(Workspace& ws) {
    ws.rnodes.release();
    ws.rnodes_resident = false;
}

// The resident scene's ray BVH, resident too: uploaded on st by the first
// flagged ray query of the scene, which counts in rt_setup_times[0] like the
// scene's own upload; later ones find it.  Frames and unflagged queries never
// come here.  The caller holds the workspace lock, has reset the staging arena
// and made the scene resident.
int ray_bvh_resident(Workspace& ws, hipStream_t st) {
    if (ws.rnodes_resident) return RT_OK;
    const auto t_up = SClock::now();
    struct AddTime {
        SClock::time_point t;
        ~AddTime() {
            std::lock_guard<std::mutex> lk(g_setup.mu);
            g_setup.scene_ms += ms_since(t);
        }
    } add_time{t_up};
    HIP_TRY(upload(ws.rnodes, ws.sc.cs.rnodes, st, &ws.up));
    ws.rnodes_resident = true;
    return RT_OK;
}

// The scene resident in the workspace: compiled and uploaded once (on st), and
// found there by every later frame or ray query of it on the device.  The
// caller holds the workspace lock and has reset the staging arena.
int scene_resident(Workspace& ws, const rt_scene* s, const rt_scene_desc& d, bool fp32, hipStream_t st) {
    SceneCache& sc = ws.sc;
    if (sc.valid && sc.uid == rtamd::scene_uid(s) && sc.fp32 == fp32) return RT_OK;
    // compile + upload the scene once; later frames of it find it resident
    // (uploads from the page-locked arena: plain DMA, no pageable staging)
    const auto t_sc = SClock::now();
    struct AddTime {
        SClock::time_point t;
        ~AddTime() {
            std::lock_guard<std::mutex> lk(g_setup.mu);
            g_setup.scene_ms += ms_since(t);
        }
    } add_scene_time{t_sc};
    sc.valid = false;
    release_node_programs(ws);
    release_ray_bvh(ws);
    try {
        sc.cs = rtamd::compile_scene(d);
    } catch (const std::exception& e) {
        rtamd::set_last_error(std::string("scene compile: ") + e.what());
        return RT_ERR_INVALID_ARG;
    }
    sc.nodes.assign(d.nodes, d.nodes + d.n_nodes);
    for (rt_node& n : sc.nodes)   // pick_region's acos thresholds (device copy only)
        if (n.kind == RT_NODE_POKEBALL) rtamd::pokeball_thresholds(n.v[5], n.v[6], n.v[rtamd::kPokeXb], n.v[rtamd::kPokeXi]);
    sc.mats.assign(d.materials, d.materials + d.n_materials);
    // device material table: K_a premultiplied by the scene's I_a (the
    // reference's E_a = mul(m.ambient, scene.ambient), one double product
    // per channel, shading.cpp:39), and one extra slot whose albedo is the
    // background colour (DevScene::bg_mat)
    for (rt_material& m : sc.mats)
        for (int c = 0; c < 3; ++c) m.ambient[c] = m.ambient[c] * d.ambient[c];
    {
        rt_material bgm{};
        for (int c = 0; c < 3; ++c) bgm.albedo[c] = d.background[c];
        sc.mats.push_back(bgm);
    }
    sc.lights.assign(d.lights, d.lights + d.n_lights);
    sc.dlights.assign(d.dir_lights, d.dir_lights + d.n_dir_lights);
    if (fp32) {
        make_float_scene(sc);
        HIP_TRY(upload(ws.nodes_f, sc.nodes_f, st, &ws.up));
        HIP_TRY(upload(ws.mats_f, sc.mats_f, st, &ws.up));
        HIP_TRY(upload(ws.lights_f, sc.lights_f, st, &ws.up));
        HIP_TRY(upload(ws.dlights_f, sc.dlights_f, st, &ws.up));
        HIP_TRY(upload(ws.fold_f, sc.fold_f, st, &ws.up));
    } else {
        HIP_TRY(upload(ws.nodes, sc.nodes, st, &ws.up));
        HIP_TRY(upload(ws.mats, sc.mats, st, &ws.up));
        HIP_TRY(upload(ws.lights, sc.lights, st, &ws.up));
        HIP_TRY(upload(ws.dlights, sc.dlights, st, &ws.up));
        HIP_TRY(upload(ws.fold, sc.cs.fold, st, &ws.up));
    }
    HIP_TRY(upload(ws.objs, sc.cs.objs, st, &ws.up));
    HIP_TRY(upload(ws.ops, sc.cs.ops, st, &ws.up));
    HIP_TRY(upload(ws.gb, sc.cs.gbounds, st, &ws.up));
    HIP_TRY(upload(ws.ctab, sc.cs.ctab, st, &ws.up));
    HIP_TRY(upload(ws.lrec, sc.cs.lrec, st, &ws.up));
    HIP_TRY(upload(ws.lwrec, sc.cs.lwrec, st, &ws.up));
    HIP_TRY(upload(ws.lgb, sc.cs.lgb, st, &ws.up));
    HIP_TRY(upload(ws.wobjs, sc.cs.wobjs, st, &ws.up));
    HIP_TRY(upload(ws.wctab, sc.cs.wctab, st, &ws.up));
    HIP_TRY(upload(ws.worig, sc.cs.worig, st, &ws.up));
    HIP_TRY(upload(ws.wchunk, sc.cs.wchunk, st, &ws.up));
    sc.uid = rtamd::scene_uid(s);
    sc.fp32 = fp32;
    sc.valid = true;
    sc.bvh_trial = 0;   // (a new scene: its own BVH trial)
    sc.bvh_key = 0;
    return RT_OK;
}

// The launch interface's view of the resident scene (scene_resident) for
// (flags, precision); n_chunks: the wave BVH unless RT_FLAG_NO_BVH (a frame's
// BVH trial may still run without it).
void scene_view(const Workspace& ws, const rt_scene_desc& d, int flags, bool fp32, SceneView& S) {
    const rtamd::CompiledScene& cs = ws.sc.cs;
    S.nodes = fp32 ? ws.nodes_f.p : ws.nodes.p;
    S.mats = fp32 ? ws.mats_f.p : ws.mats.p;
    S.lights = fp32 ? ws.lights_f.p : ws.lights.p;
    S.dlights = fp32 ? ws.dlights_f.p : ws.dlights.p;
    S.fold = fp32 ? ws.fold_f.p : ws.fold.p;
    S.n_dlights = d.n_dir_lights;
    S.objs = ws.objs.as<rtamd::DevObj>();
    S.ops = ws.ops.as<rtamd::DevOp>();
    S.gb = ws.gb.as<float>();
    S.ctab = ws.ctab.as<float>();
    S.lrec = ws.lrec.as<float>();
    S.lwrec = ws.lwrec.as<float>();
    S.lgb = ws.lgb.as<float>();
    S.n_gb = (int)(cs.gbounds.size() / 4);
    S.wobjs = ws.wobjs.as<rtamd::DevObj>();
    S.wctab = ws.wctab.as<float>();
    S.worig = ws.worig.as<int32_t>();
    S.wchunk = ws.wchunk.as<float>();
    S.n_wobjs = (int)cs.wobjs.size();
    S.n_chunks = (flags & RT_FLAG_NO_BVH) ? 0 : (int)(cs.wchunk.size() / 8);
    S.n_lights = d.n_lights;
    S.n_objs = (int)cs.objs.size();
    S.n_bounded = 0;
    for (const auto& o : cs.objs)
        if (o.has_bound && o.kind != rtamd::OBJ_GROUP) ++S.n_bounded;
    S.cam_nx = rt_camera_width(&d.camera);
    S.cam_ny = rt_camera_height(&d.camera);
    S.rec_limit = d.recursion_limit;
    S.cull = (flags & RT_FLAG_NO_CULL) ? 0 : 1;
    {
        static const bool lead_on = [] { const char* e = std::getenv("RT_LEAD"); return !(e && *e == '0'); }();
        S.n_lead = lead_on ? cs.n_lead : 0;   // (RT_LEAD=0: measurement A/B)
    }
    for (int i = 0; i < 3; ++i) {
        S.eye[i] = d.camera.eye[i];
        S.P[i] = d.camera.P[i];
    }
    S.Lx = d.camera.Lx;
    S.Ly = d.camera.Ly;
    S.medium_index = d.medium_index;
    S.bg_mat = d.n_materials;
}

// The page-locked words k_reduce_counters stores into: at least host_words
// (the previous frame's or query's readback is done)
int ensure_ctr_host(Workspace& ws, size_t host_words) {
    if (ws.ctr_host && ws.ctr_host_words >= host_words) return RT_OK;
    if (ws.ctr_host) (void)hipHostFree(ws.ctr_host);
    ws.ctr_host = nullptr;
    ws.ctr_host_words = 0;
    rtamd::SetupTimer tm(rtamd::kSetupPinned);
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&ws.ctr_host), host_words * sizeof(unsigned long long),
                          hipHostMallocDefault));
    ws.ctr_host_words = host_words;
    return RT_OK;
}

// The ray / op counter slots, zero on st before a frame's or a radiance
// query's first launch (the last k_reduce_counters may have left them zero)
int counters_ready(Workspace& ws, hipStream_t st) {
    const size_t ctr_bytes = (size_t)kCounterSlots * kCounterWords * sizeof(unsigned long long);
    const void* before = ws.counters.p;
    HIP_TRY(ws.counters.ensure(ctr_bytes));
    if (!ws.counters_zero || ws.counters.p != before) HIP_TRY(hipMemsetAsync(ws.counters.p, 0, ctr_bytes, st));
    ws.counters_zero = false;   // (until the reduction has run)
    return RT_OK;
}

// The jitter draws of a standard frame's rows, for the frame (frame_begin) and
// for the frame's rays (camera_rays_impl, jittered) alike, in two steps around
// the caller's ms_rng event.  The caller holds the workspace lock, has reset
// the staging arena, and reports its successful end with ws.jcache.complete.
//
// 1. the plan of (W, H, rows), and the checkpoint table reaching the last loop
//    row's stream words (built on the first use, extended only for a larger frame)
int jitter_plan_ready(Workspace& ws, int W, int H, const int32_t* rows_host, int n_rows, hipStream_t st,
                      rtamd::StdPlan& plan) {
    plan = rtamd::plan_std_frame(W, H, rows_host, n_rows, (int64_t)rtamd::kTableK * 624);
    try {   // (the jump polynomials: file read or GF(2) arithmetic, may throw)
        if (plan.n_ckpt > ws.jtab.n_ck) {   // a build or an extension: synchronous
            const auto t_j = SClock::now();
            HIP_TRY(ws.jtab.ensure(plan.n_ckpt, st));
            std::lock_guard<std::mutex> lk(g_setup.mu);
            g_setup.jtable_ms += ms_since(t_j);
        }
    } catch (const std::exception& e) {
        rtamd::set_last_error(std::string("jitter checkpoint table: ") + e.what());
        return RT_ERR_PROCESSING;
    }
    return RT_OK;
}

// 2. the buffer holding the draws and the rows / jitter-row lists, which are a
//    function of (W, H, rows) alone: a key resident in the workspace (its
//    filling call ended successfully, so the draws are complete whatever
//    stream this call runs on) uploads and generates nothing; otherwise the
//    rows upload and the fill are enqueued on st.  *filled (may be null):
//    whether the fill was launched.
int jitter_draws(Workspace& ws, const char* what, int W, int H, int n_rows, const rtamd::StdPlan& sp, hipStream_t st,
                 rtamd::JitterCache::Entry** ent, bool* filled = nullptr) {
    if (filled) *filled = false;
    const rtamd::JitterCache::Got got = ws.jcache.acquire(W, H, sp.rows_jrow, (size_t)n_rows * 16 * W * sizeof(double),
                                                          rtamd::jitter_cache_budget());
    if (!got.e) {
        rtamd::set_last_error(std::string(what) + ": out of device memory for the frame's jitter draws");
        return RT_ERR_HIP;
    }
    *ent = got.e;
    if (got.upload_rows)
        HIP_TRY(rtamd::upload_async(&ws.up, got.e->rows(), sp.rows_jrow.data(), sp.rows_jrow.size() * sizeof(int32_t), st));
    if (got.fill) {
        HIP_TRY(ws.jscratch.ensure(rtamd::mt_fill_scratch_bytes(sp.jranges)));
        ws.jjob.up = &ws.up;
        const auto t_l = SClock::now();
        HIP_TRY(rtamd::mt_launch_fill(ws.jtab, sp.jranges, ws.jjob, ws.jscratch.p, got.e->jit(), st));
        if (filled) *filled = true;
        {
            std::lock_guard<std::mutex> lk(g_setup.mu);
            if (!g_setup.jitter_launched) g_setup.jitter_launch_ms = ms_since(t_l);
            g_setup.jitter_launched = true;
        }
    }
    return RT_OK;
}

int frame_begin(const rt_scene* s, int W, int H, int mode, int flags, const int32_t* rows_host, int n_rows,
                hipStream_t st, rt_frame** out) {
    const auto t_start = std::chrono::steady_clock::now();
    if (!out) { rtamd::set_last_error("rt_frame_begin: out is NULL"); return RT_ERR_INVALID_ARG; }
    *out = nullptr;
    if (!s) { rtamd::set_last_error("rt_render: scene is NULL"); return RT_ERR_INVALID_ARG; }
    if (W <= 0 || H <= 0) { rtamd::set_last_error("rt_render: W and H must be > 0"); return RT_ERR_INVALID_ARG; }
    if (mode != RT_MODE_STANDARD && mode != RT_MODE_PAPER) { rtamd::set_last_error("rt_render: bad mode"); return RT_ERR_INVALID_ARG; }
    if (n_rows < 0 || (n_rows > 0 && !rows_host)) { rtamd::set_last_error("rt_render: bad rows"); return RT_ERR_INVALID_ARG; }
    {
        std::vector<char> seen(H, 0);
        for (int i = 0; i < n_rows; ++i) {
            if (rows_host[i] < 0 || rows_host[i] >= H) { rtamd::set_last_error("rt_render: row out of range"); return RT_ERR_INVALID_ARG; }
            if (seen[rows_host[i]]++) { rtamd::set_last_error("rt_render: duplicate row"); return RT_ERR_INVALID_ARG; }
        }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        rtamd::set_last_error("rt_render: no HIP device available");
        return RT_ERR_NO_DEVICE;
    }
    const rt_scene_desc& d = *rt_scene_get_desc(s);
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::unique_ptr<rt_frame> f(new rt_frame);
    f->ws = &workspace(dev);
    f->lock = std::unique_lock<std::mutex>(f->ws->mu);
    // a failure below may leave uploads of this frame queued on st (some read
    // the page-locked staging arena the next frame_begin resets): drain st
    // before the workspace lock goes (destroyed before f)
    struct DrainOnFail {
        hipStream_t st;
        bool armed = true;
        ~DrainOnFail() {
            if (armed) (void)hipStreamSynchronize(st);
        }
    } drain{st};
    Workspace& ws = *f->ws;
    const bool fp32 = (flags & RT_FLAG_FP32) != 0;
    SceneCache& sc = ws.sc;
    ws.up.reset();   // (the previous frame's uploads completed: its rt_frame_end synchronised)
    {
        const int rv = scene_resident(ws, s, d, fp32, st);
        if (rv != RT_OK) return rv;
    }
    const rtamd::CompiledScene& cs = sc.cs;
    f->st = st;
    f->W = W;
    f->H = H;
    f->mode = mode;
    f->n_rows = n_rows;
    f->fp32 = fp32;
    f->t_start = t_start;
    if (!ws.ev[0]) {
        rtamd::SetupTimer tm(rtamd::kSetupStreams);
        for (int i = 0; i < 4; ++i) HIP_TRY(hipEventCreate(&ws.ev[i]));
    }
    {
        const int rv = counters_ready(ws, st);
        if (rv != RT_OK) return rv;
    }

    SceneView& S = f->S;
    scene_view(ws, d, flags, fp32, S);
    f->bvh_trial = -1;
    if (S.n_chunks > 0 && !(flags & (RT_FLAG_NO_CULL | RT_FLAG_FORCE_BVH)) && bvh_ab()) {
        const uint64_t key = ((uint64_t)(uint32_t)W << 40) ^ ((uint64_t)(uint32_t)H << 20) ^ ((uint64_t)n_rows << 2) ^
                             ((uint64_t)mode << 1) ^ ((uint64_t)(uint32_t)flags << 48);
        if (sc.bvh_key != key) {
            sc.bvh_key = key;
            sc.bvh_trial = 0;
        }
        if (sc.bvh_trial < 2) f->bvh_trial = sc.bvh_trial;
        if (sc.bvh_trial == 1 || (sc.bvh_trial == 2 && sc.bvh_off)) S.n_chunks = 0;
    }
    // the trace kernel (the stack tiers, the culling and plain variants);
    // this frame's BVH trial may run it without the wave BVH
    {
        const int rv = rtamd::pick_variant(cs, d, mode, flags, S.n_chunks > 0, &f->kv);
        if (rv != RT_OK) return rv;
    }

    if (n_rows > 0 && mode == RT_MODE_STANDARD) {
        const int rv = jitter_plan_ready(ws, W, H, rows_host, n_rows, st, f->std_plan);
        if (rv != RT_OK) return rv;
    }
    HIP_TRY(hipEventRecord(ws.ev[0], st));
    if (n_rows > 0 && mode == RT_MODE_STANDARD) {
        const int rv = jitter_draws(ws, "rt_render", W, H, n_rows, f->std_plan, st, &f->jent);
        if (rv != RT_OK) return rv;
        f->jit = f->jent->jit();
        f->rows = f->jent->rows();
    } else if (n_rows > 0) {
        f->paper = rtamd::plan_paper_frame(rtamd::scene_uid(s), W, H, mode, flags, rows_host, n_rows);
        f->paper_calls.reset(&f->paper);
        const rtamd::PaperPlan& pp = f->paper;
        HIP_TRY(ws.paper_aux.ensure(pp.aux_ints() * sizeof(int32_t)));
        HIP_TRY(ws.gtime.ensure(pp.gtime_words() * sizeof(unsigned)));
        HIP_TRY(rtamd::upload_async(&ws.up, ws.paper_aux.p, pp.aux.data(), pp.aux.size() * sizeof(int32_t), st));
        const size_t npx = (size_t)pp.n_ext * W;
        HIP_TRY(ws.paper_i.ensure(npx * sizeof(int)));
        HIP_TRY(ws.paper_d.ensure(npx * 4 * sizeof(double)));
    }
    HIP_TRY(hipEventRecord(ws.ev[1], st));
    drain.armed = false;
    *out = f.release();
    rtamd::note_setup_ms(rtamd::kLastBegin, ms_since(t_start));
    {
        std::lock_guard<std::mutex> lk(g_setup.mu);
        g_setup.extra[rtamd::kLastTrace] = 0.0;   // (this frame's trace calls add to it)
    }
    return RT_OK;
}

// fb: FP64 rows; codes (paper mode, FP64 kernels only): one paper_code byte
// per pixel instead (rtamd::frame_trace_paper_codes).
int frame_trace(rt_frame* f, int ri0, int ri1, double* fb, hipStream_t hs, uint8_t* codes = nullptr) {
    if (!f) { rtamd::set_last_error("rt_frame_trace: frame is NULL"); return RT_ERR_INVALID_ARG; }
    if (ri0 < 0 || ri1 < ri0 || ri1 > f->n_rows) { rtamd::set_last_error("rt_frame_trace: bad row range"); return RT_ERR_INVALID_ARG; }
    if (ri1 == ri0) return RT_OK;
    if (!fb && !codes) { rtamd::set_last_error("rt_frame_trace: fb is NULL"); return RT_ERR_INVALID_ARG; }
    if (codes && (f->mode != RT_MODE_PAPER || f->fp32)) {
        rtamd::set_last_error("rt_frame_trace: paper codes need a paper-mode FP64 frame");
        return RT_ERR_INVALID_ARG;
    }
    Workspace& ws = *f->ws;
    const hipStream_t st = hs ? hs : f->st;
    const int W = f->W, n = ri1 - ri0;
    unsigned long long* ctr = ws.counters.as<unsigned long long>();
    // another stream first waits for the scene upload and jitter (begin).  In
    // paper mode a chunk whose finish pass reads primary hits that an earlier
    // call computed on another stream waits for that call's PRIMARY pass
    // (PaperCalls::next_call: one GPU's chunked frame, or adjacent strips of
    // one rank), and only its finish waits: its primary computes new entries
    // only, so it overlaps the earlier call's finish (latency-bound) on the
    // other stream.
    const auto t_launch = SClock::now();
    if (st != f->st) HIP_TRY(hipStreamWaitEvent(st, ws.ev[1], 0));
    const int call = (int)f->call_st.size();   // this call's index (ws.pev / ws.tev)
    // paper mode: a call that fails before its events are recorded is taken
    // back, so that a later call never waits on an event that was not recorded
    struct Rollback {
        rtamd::PaperCalls* calls;
        ~Rollback() {
            if (calls) calls->rollback();
        }
    } undo{nullptr};
    if (f->mode == RT_MODE_STANDARD) {
        StdParams P;
        P.W = W;
        P.H = f->H;
        P.n_rows = n;
        P.rows = f->rows + ri0;
        P.jrow = f->rows + f->n_rows + ri0;
        P.jit = f->jit;
        P.fb = fb;
        P.counters = ctr;
        HIP_TRY(rtamd::launch_std(f->kv, st, f->S, P));
    } else {
        // RT_PAPER_ORDER (measurement A/B): 0 = row order, untimed; 1 = row
        // order, every frame timed; 2 (default) = costliest blocks first,
        // from the wave times of the first frame of the scene and row set
        // (later frames untimed: a timed launch reads the clock ahead of
        // the scene loads, which costs it its scalar loads, k_paper_primary_lean)
        static const int order_mode = [] { const char* e = std::getenv("RT_PAPER_ORDER"); return e && *e ? std::atoi(e) : 2; }();
        const rtamd::PaperPlan& pp = f->paper;
        const auto cost_it = ws.paper_cost.find(pp.key);
        const bool have_cost = cost_it != ws.paper_cost.end();
        // primary hits of the ext rows this chunk reads that no earlier chunk computed
        const rtamd::PaperCalls::Call c = f->paper_calls.next_call(
            ri0, ri1, reinterpret_cast<uintptr_t>(st), order_mode >= 2 && have_cost ? &cost_it->second : nullptr);
        if (!c.ok) {
            rtamd::set_last_error("rt_frame_trace: paper-mode list overflow");
            return RT_ERR_PROCESSING;
        }
        undo.calls = &f->paper_calls;
        int32_t* aux = ws.paper_aux.as<int32_t>();
        PaperParams P;
        P.W = W;
        P.H = f->H;
        P.n_ext = pp.n_ext;
        P.ext_rows = aux + pp.off_ext_rows();
        P.ext_shade = aux + pp.off_ext_shade();
        P.nbr = aux + pp.off_nbr() + 3 * (size_t)ri0;
        P.rows = aux + pp.off_rows() + ri0;
        int32_t* d_list = aux + pp.off_lists() + c.list_off;
        P.ext_list = d_list;
        P.n_list = (int)c.list->size();
        P.n_rows = n;
        const size_t npx = (size_t)pp.n_ext * W;
        P.mat = ws.paper_i.as<int>();
        double* dd = ws.paper_d.as<double>();
        P.t = dd;
        P.nx = dd + npx;
        P.ny = dd + 2 * npx;
        P.nz = dd + 3 * npx;
        P.fb = fb;
        P.code = codes;
        P.gtime = nullptr;
        P.counters = ctr;
        if (!c.list->empty()) {
            rtamd::KernelVariant kv = f->kv;
            if (!kv.count_ops && (order_mode == 1 || (order_mode >= 2 && !have_cost))) {
                P.gtime = ws.gtime.as<unsigned>() + (size_t)(c.list_off / 8) * rtamd::paper_waves_per_group(W) * 2;
                kv.timed = f->timed = true;
            }
            HIP_TRY(rtamd::upload_async(&ws.up, d_list, c.list->data(), c.list->size() * sizeof(int32_t), st));
            dim3 g1((W + 15) / 16, (P.n_list + 15) / 16);
            HIP_TRY(rtamd::launch_paper(kv, g1, st, f->S, P));
        }
        if ((int)ws.pev.size() <= call) {
            hipEvent_t e = nullptr;
            HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            ws.pev.push_back(e);
        }
        HIP_TRY(hipEventRecord(ws.pev[call], st));
        for (int w : c.wait) HIP_TRY(hipStreamWaitEvent(st, ws.pev[w], 0));
        dim3 g2((W + 63) / 64, (n + 3) / 4);
        HIP_TRY(rtamd::launch_paper_finish(f->kv, g2, st, f->S, P));
    }
    {
        std::lock_guard<std::mutex> lk(g_setup.mu);
        if (!g_setup.trace_launched) g_setup.trace_launch_ms = ms_since(t_launch);
        g_setup.trace_launched = true;
    }
    if ((int)ws.tev.size() <= call) {
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ws.tev.push_back(e);
    }
    HIP_TRY(hipEventRecord(ws.tev[call], st));
    rtamd::note_setup_ms(rtamd::kLastTrace, ms_since(t_launch));
    HIP_TRY(rtamd::warm_copy_engine(st));   // (once per process, while the trace runs)
    undo.calls = nullptr;
    f->call_st.push_back(st);
    return RT_OK;
}

int frame_end_body(rt_frame* f, rt_stats* stats);

int frame_end(rt_frame* f, rt_stats* stats) {
    if (!f) { rtamd::set_last_error("rt_frame_end: frame is NULL"); return RT_ERR_INVALID_ARG; }
    std::unique_ptr<rt_frame> own(f);   // (holds the workspace lock)
    const auto t_end = SClock::now();
    const int rc = frame_end_body(f, stats);
    rtamd::note_setup_ms(rtamd::kLastEnd, ms_since(t_end));
    if (rc != RT_OK) {
        // an early return left this frame's work queued: drain every stream it
        // used before the lock goes (the next frame_begin resets the
        // page-locked staging its copies read, and reuses its buffers)
        (void)hipStreamSynchronize(f->st);
        for (hipStream_t s : f->call_st) (void)hipStreamSynchronize(s);
    }
    return rc;
}

int frame_end_body(rt_frame* f, rt_stats* stats) {
    Workspace& ws = *f->ws;
    const hipStream_t st = f->st;
    // join the other trace streams: one wait on each one's last call (stream
    // order covers its earlier ones; every wait is a barrier packet on st)
    for (size_t i = 0; i < f->call_st.size(); ++i) {
        if (f->call_st[i] == st) continue;
        bool last = true;
        for (size_t j = i + 1; j < f->call_st.size(); ++j) last = last && f->call_st[j] != f->call_st[i];
        if (last) HIP_TRY(hipStreamWaitEvent(st, ws.tev[i], 0));
    }
    HIP_TRY(hipEventRecord(ws.ev[2], st));
    const int n_groups = f->paper_calls.list_used() / 8;
    const size_t host_words = kCounterWords + ((size_t)n_groups + 1) / 2;
    {
        const int rv = ensure_ctr_host(ws, host_words);
        if (rv != RT_OK) return rv;
    }
    unsigned long long* ctr = ws.counters.as<unsigned long long>();
    const bool timed = f->timed;   // (some launch of this frame stored its waves' ticks)
    hipLaunchKernelGGL(k_reduce_counters, dim3(kCounterWords + (timed ? n_groups : 0)), dim3(64), 0, st, ctr, ws.ctr_host,
                       ws.gtime.as<unsigned>(), rtamd::paper_waves_per_group(f->W));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ws.ev[3], st));
    HIP_TRY(rtamd::spin_wait(ws.ev[3]));
    ws.counters_zero = true;
    // every stream of the frame has run to its end: the draws and the rows
    // list this frame wrote are complete, and later frames of its key may
    // read them (a frame that fails before this point leaves no valid entry)
    ws.jcache.complete(f->jent);
    unsigned long long hc[kCounterWords];
    for (int k = 0; k < kCounterWords; ++k) hc[k] = ((volatile unsigned long long*)ws.ctr_host)[k];
    if (timed) {
        // this frame's group costs, by each group's first ext index
        const uint64_t key = f->paper.key;
        if (ws.paper_cost.size() >= 64 && !ws.paper_cost.count(key)) ws.paper_cost.clear();
        const volatile unsigned int* gcv = reinterpret_cast<const volatile unsigned int*>(ws.ctr_host + kCounterWords);
        const std::vector<uint32_t> gc(gcv, gcv + n_groups);
        f->paper_calls.group_costs(gc.data(), ws.paper_cost[key]);
    }
    if (f->bvh_trial >= 0) {
        // the BVH trial frames: their trace kernels' time decides later frames
        SceneCache& sc = ws.sc;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ws.ev[1], ws.ev[2]) == hipSuccess && sc.bvh_trial == f->bvh_trial) {
            sc.bvh_ms[f->bvh_trial] = ms;
            if (++sc.bvh_trial == 2) sc.bvh_off = sc.bvh_ms[1] < sc.bvh_ms[0];
        }
    }
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->rays_intersect = f->mode == RT_MODE_PAPER ? f->paper.logical_isect : hc[0];
        stats->rays_occluded = hc[1];
        stats->rays_traced = hc[0] + hc[1];
        stats->pixels = (uint64_t)f->n_rows * f->W;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ws.ev[0], ws.ev[1]) == hipSuccess) stats->ms_rng = ms;
        if (hipEventElapsedTime(&ms, ws.ev[1], ws.ev[2]) == hipSuccess) stats->ms_kernel = ms;
        for (int k = 0; k < 16; ++k) stats->ops[k] = hc[2 + k];
        stats->ms_total =
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - f->t_start).count();
        stats->n_gpus = 1;
    }
    return RT_OK;
}

int render_rows_impl(const rt_scene* s, int W, int H, int mode, int flags, const int32_t* rows_host, int n_rows,
                     double* fb_dev, hipStream_t st, rt_stats* stats) {
    if (n_rows > 0 && !fb_dev) { rtamd::set_last_error("rt_render: bad rows/fb"); return RT_ERR_INVALID_ARG; }
    rt_frame* f = nullptr;
    int rc = frame_begin(s, W, H, mode, flags, rows_host, n_rows, st, &f);
    if (rc != RT_OK) return rc;
    // paper mode: row chunks alternating between a second stream and the
    // frame's (rtamd::row_chunks), so that each chunk's finish overlaps the
    // next chunk's primary; the last chunk runs on the frame stream
    std::vector<std::pair<int, int>> bounds{{0, n_rows}};
    if (mode == RT_MODE_PAPER && rtamd::paper_chunks_1gpu() > 1) {
        Workspace& ws = *f->ws;
        if (!ws.aux_st && hipStreamCreateWithFlags(&ws.aux_st, hipStreamNonBlocking) != hipSuccess) ws.aux_st = nullptr;
        if (ws.aux_st) bounds = rtamd::row_chunks(n_rows, rtamd::paper_chunks_1gpu(), RT_PAPER_STRIP_ROWS);
    }
    for (size_t k = 0; k < bounds.size() && rc == RT_OK; ++k) {
        const hipStream_t cst = ((bounds.size() - 1 - k) & 1) ? f->ws->aux_st : nullptr;
        rc = frame_trace(f, bounds[k].first, bounds[k].second, fb_dev + (size_t)bounds[k].first * W * 3, cst);
    }
    const int rc2 = frame_end(f, stats);
    return rc != RT_OK ? rc : rc2;
}

// ------------------------------------------------------ batched-call driver
// What every batched entry point (the ray, radiance and shading queries, the
// camera rays, the paper resolve) shares.  An entry point is its argument
// checks, a BatchCall, its buffers and parameter block, and one run() whose
// callbacks stage a chunk in, launch, and stage it out.
//
// Items (rays, hits, list rows) of one launch: 2^30 (the grid's x extent holds
// 2^31 - 1 one-wave workgroups).  Items of one chunk of a call from host
// memory: g_chunk_items, 2^20 unless rt_test_camera_chunk_rays sets another
// size - for rays 64 MiB of rays + 64 MiB of hits + 1 MiB of flags in the
// workspace, large enough that a chunk's launch and copy overheads vanish in
// its transfers.  (The camera rays count it in rays and take whole rows.)
constexpr size_t kLaunchItems = (size_t)1 << 30;
constexpr size_t kChunkItems = (size_t)1 << 20;
std::atomic<size_t> g_chunk_items{kChunkItems};
constexpr int kKnownFlags =
    RT_FLAG_COUNT_OPS | RT_FLAG_NO_CULL | RT_FLAG_FP32 | RT_FLAG_NO_BVH | RT_FLAG_FORCE_BVH | RT_FLAG_RAY_BVH;

// One batched call on stream st.  Made first (it takes the call's start time);
// zero_stats() once the arguments that are checked before the stats are fine;
// open() before the first use of the device.  From open() on the call holds
// the workspace lock like a frame, and whatever happens nothing of it is left
// queued on st when the lock goes (the next frame resets the staging arena the
// uploads read, and reuses the chunk buffers): the destructor drains st, and
// runs before the members - the lock - are destroyed.
struct BatchCall {
    const char* what;
    hipStream_t st;
    rt_stats* stats = nullptr;
    const SClock::time_point t_start = SClock::now();
    Workspace* ws = nullptr;
    std::unique_lock<std::mutex> lock;
    bool counting = false;     // counters(): finish() reduces the slots
    double ms_kernel = 0.0;    // run(): the chunks' launches, by the workspace's events

    BatchCall(const char* what_, hipStream_t st_) : what(what_), st(st_) {}
    BatchCall(const BatchCall&) = delete;
    ~BatchCall() {
        if (ws) (void)hipStreamSynchronize(st);
    }
    int fail(const char* msg, int rc) const {
        rtamd::set_last_error(std::string(what) + ": " + msg);
        return rc;
    }
    void zero_stats(rt_stats* stats_) {
        stats = stats_;
        if (!stats) return;
        std::memset(stats, 0, sizeof(*stats));
        stats->n_gpus = 1;
    }
    // the device, its workspace and lock, the staging arena reset (the previous
    // frame's or call's uploads completed), the workspace's events
    int open() {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail("no HIP device available", RT_ERR_NO_DEVICE);
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        ws = &workspace(dev);
        lock = std::unique_lock<std::mutex>(ws->mu);   // (waits for an open frame of this device)
        ws->up.reset();
        if (!ws->ev[0]) {
            rtamd::SetupTimer tm(rtamd::kSetupStreams);
            for (int i = 0; i < 4; ++i) HIP_TRY(hipEventCreate(&ws->ev[i]));
        }
        return RT_OK;
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
        if (rv == RT_OK) rv = pick(ws->sc.cs, pick_desc ? *pick_desc : d, flags, &kv);
        if (rv != RT_OK) return rv;
        scene_view(*ws, d, flags, false, S);
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
        for (size_t c0 = 0; c0 < n; c0 += chunk) {
            const size_t cn = std::min(chunk, n - c0);
            int rv = in(c0, cn);
            if (rv != RT_OK) return rv;
            HIP_TRY(hipEventRecord(ws->ev[1], st));
            for (size_t l0 = 0; l0 < cn && rv == RT_OK; l0 += launch_max) rv = launch(c0, l0, std::min(launch_max, cn - l0));
            if (rv != RT_OK) return rv;
            HIP_TRY(hipEventRecord(ws->ev[2], st));
            rv = out(c0, cn);
            if (rv != RT_OK) return rv;
            HIP_TRY(hipStreamSynchronize(st));
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ws->ev[1], ws->ev[2]) == hipSuccess) ms_kernel += ms;
        }
        return RT_OK;
    }
    static int no_staging(size_t, size_t) { return RT_OK; }
    // The call's good end: a counting call's slots summed as a frame's end reads
    // them (ctr(0), ctr(1): the Scene::intersect / Scene::occluded calls; the
    // slots are left zero), and the times.
    int finish() {
        if (counting) {
            hipLaunchKernelGGL(k_reduce_counters, dim3(kCounterWords), dim3(64), 0, st,
                               ws->counters.as<unsigned long long>(), ws->ctr_host, nullptr, 0);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(st));
            ws->counters_zero = true;
        }
        if (stats) {
            stats->ms_kernel = ms_kernel;
            stats->ms_total = ms_since(t_start);
        }
        return RT_OK;
    }
    uint64_t ctr(int word) const { return ((volatile unsigned long long*)ws->ctr_host)[word]; }
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
    if (!s) return call.fail("scene is NULL", RT_ERR_INVALID_ARG);
    if (flags & ~kKnownFlags) return call.fail("unknown flag bits", RT_ERR_INVALID_ARG);
    int rv = rtamd::check_query_flags(flags);
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
    // RT_FLAG_RAY_BVH: the ray-BVH row of the variant where the scene has the tree (frame_plan.hpp use_ray_bvh)
    const bool ray_bvh = !radiance && rtamd::use_ray_bvh(ws.sc.cs, kv, flags);
    if (ray_bvh) {
        rv = ray_bvh_resident(ws, st);
        if (rv != RT_OK) return rv;
    }
    const size_t chunk = host ? std::min(n, g_chunk_items.load()) : n;
    if (host) {
        HIP_TRY(ws.q_rays.ensure(chunk * sizeof(rt_ray)));
        if (isect) HIP_TRY(ws.q_hits.ensure(chunk * sizeof(rt_hit)));
        if (mask) HIP_TRY(ws.q_mask.ensure(chunk));
        if (radiance) HIP_TRY(ws.q_rgb.ensure(chunk * 3 * sizeof(double)));
    }
    // a chunk on the device: the staging buffers, or the caller's (one chunk)
    const rt_ray* d_rays = host ? ws.q_rays.as<rt_ray>() : rays;
    rt_hit* d_hits = !isect ? nullptr : host ? ws.q_hits.as<rt_hit>() : hits;
    uint8_t* d_mask = !mask ? nullptr : host ? ws.q_mask.as<uint8_t>() : mask;
    double* d_rgb = !radiance ? nullptr : host ? ws.q_rgb.as<double>() : rgb;
    rv = call.run(
        n, chunk, kLaunchItems,
        [&](size_t c0, size_t cn) -> int {
            if (host) HIP_TRY(hipMemcpyAsync(ws.q_rays.p, rays + c0, cn * sizeof(rt_ray), hipMemcpyHostToDevice, st));
            return RT_OK;
        },
        [&](size_t, size_t l0, size_t ln) -> int {
            if (radiance) {
                RadianceParams P;
                P.n = ln;
                P.rays = d_rays + l0;
                P.rgb = d_rgb + 3 * l0;
                P.counters = ws.counters.as<unsigned long long>();
                HIP_TRY(rtamd::launch_radiance(kv, st, S, P));
            } else if (ray_bvh) {
                rtamd::RayBvhParams P{};
                P.n = ln;
                P.rays = d_rays + l0;
                P.hits = d_hits ? d_hits + l0 : nullptr;
                P.mask = d_mask ? d_mask + l0 : nullptr;
                P.nodes = ws.rnodes.as<rtamd::RayBvhNode>();
                P.n_nodes = (int)ws.sc.cs.rnodes.size();
                P.n_lead = ws.sc.cs.rlead;
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
// only this call's SceneView points there, so the resident scene (ws.lights,
// the scene cache) is what it was.  The Scene::occluded calls are counted.
int shade_impl(const char* what, const rt_scene* s, const rt_hit* hits, const double* wo, const uint8_t* mask, size_t n,
               const rt_light* lights, int n_lights, const double* miss_rgb, int flags, double* rgb, bool host,
               hipStream_t st, rt_stats* stats) {
    BatchCall call(what, st);
    if (!s) return call.fail("scene is NULL", RT_ERR_INVALID_ARG);
    if (flags & ~kKnownFlags) return call.fail("unknown flag bits", RT_ERR_INVALID_ARG);
    int rv = rtamd::check_query_flags(flags);
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
    if (n_lights >= 0) {
        // this call's point lights: k_shade (WV = 0) reads nothing else by light number
        HIP_TRY(ws.q_lights.ensure(n_lights ? (size_t)n_lights * sizeof(rt_light) : 16));
        HIP_TRY(rtamd::upload_async(&ws.up, ws.q_lights.p, lights, (size_t)n_lights * sizeof(rt_light), st));
        S.lights = ws.q_lights.p;
        S.n_lights = n_lights;
    }
    rv = call.counters();
    if (rv != RT_OK) return rv;
    const size_t chunk = host ? std::min(n, g_chunk_items.load()) : n;
    if (host) {
        HIP_TRY(ws.q_hits.ensure(chunk * sizeof(rt_hit)));
        HIP_TRY(ws.q_wo.ensure(chunk * 3 * sizeof(double)));
        if (mask) HIP_TRY(ws.q_mask.ensure(chunk));
        HIP_TRY(ws.q_rgb.ensure(chunk * 3 * sizeof(double)));
    }
    // a chunk on the device: the staging buffers, or the caller's (one chunk)
    ShadeParams P0;
    P0.hits = host ? ws.q_hits.as<rt_hit>() : hits;
    P0.wo = host ? ws.q_wo.as<double>() : wo;
    P0.mask = !mask ? nullptr : host ? ws.q_mask.as<uint8_t>() : mask;
    P0.rgb = host ? ws.q_rgb.as<double>() : rgb;
    for (int c = 0; c < 3; ++c) P0.miss[c] = miss_rgb ? miss_rgb[c] : rt_scene_get_desc(s)->background[c];
    P0.counters = ws.counters.as<unsigned long long>();
    rv = call.run(
        n, chunk, kLaunchItems,
        [&](size_t c0, size_t cn) -> int {
            if (!host) return RT_OK;
            HIP_TRY(hipMemcpyAsync(ws.q_hits.p, hits + c0, cn * sizeof(rt_hit), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(ws.q_wo.p, wo + 3 * c0, cn * 3 * sizeof(double), hipMemcpyHostToDevice, st));
            if (mask) HIP_TRY(hipMemcpyAsync(ws.q_mask.p, mask + c0, cn, hipMemcpyHostToDevice, st));
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
// The program of (node, kind) of the resident scene d, resident too: compiled
// (this node's subtree only, so a deep chain's nodes cost their own sizes, not
// the quadratic sum) and uploaded on st by the first query of it, which counts
// in rt_setup_times[0] like the scene's own compile; later queries find it.
// A program deeper than the big stacks is refused here, on the host
// (pick_node_variant), and leaves no entry.  The caller holds the workspace
// lock, has reset the staging arena and made the scene resident.
int node_program_resident(Workspace& ws, const rt_scene_desc& d, int node, int kind, int flags, hipStream_t st,
                          const NodeProg** out) {
    const auto key = std::make_pair(node, kind);
    auto it = ws.node_progs.find(key);
    if (it != ws.node_progs.end()) {
        *out = &it->second;
        return RT_OK;
    }
    const auto t_np = SClock::now();
    struct AddTime {
        SClock::time_point t;
        ~AddTime() {
            std::lock_guard<std::mutex> lk(g_setup.mu);
            g_setup.scene_ms += ms_since(t);
        }
    } add_time{t_np};
    NodeProg np;
    try {
        rtamd::NodeProgram p = rtamd::compile_node_program(d, node, kind);
        const int rv = rtamd::pick_node_variant(d, node, p, flags, &np.kv);
        if (rv != RT_OK) return rv;
        if (np.kv.eager) np.host = std::move(p.ops);
    } catch (const std::exception& e) {
        rtamd::set_last_error(std::string("node compile: ") + e.what());
        return RT_ERR_INVALID_ARG;
    }
    it = ws.node_progs.emplace(key, std::move(np)).first;
    if (!it->second.host.empty()) {
        const hipError_t e = upload(it->second.ops, it->second.host, st, &ws.up);
        if (e != hipSuccess) {
            it->second.ops.release();
            ws.node_progs.erase(it);
            rtamd::set_last_error(std::string("node program upload failed: ") + hipGetErrorString(e));
            return RT_ERR_HIP;
        }
    }
    *out = &it->second;
    return RT_OK;
}

// rt_query_node_{intersect,interval}[_device]: kind rtamd::kNodeIsect (enter:
// the hits; ex unused) / kNodeIvl (enter / ex: the enterHit / exitHit records).
// host: rays and results are host memory, moved through the workspace's chunk
// buffers (the ray queries' q_rays / q_hits / q_mask, and q_exit); else device
// memory, evaluated in place on st.
int node_impl(const char* what, const rt_scene* s, int node, int kind, const rt_ray* rays, size_t n, int flags,
              rt_hit* enter, rt_hit* ex, uint8_t* mask, bool host, hipStream_t st, rt_stats* stats) {
    BatchCall call(what, st);
    const bool isect = kind == rtamd::kNodeIsect;
    if (!s) return call.fail("scene is NULL", RT_ERR_INVALID_ARG);
    if (flags & ~kKnownFlags) return call.fail("unknown flag bits", RT_ERR_INVALID_ARG);
    int rv = rtamd::check_query_flags(flags);
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
    rv = scene_resident(ws, s, d, false, st);
    const NodeProg* np = nullptr;
    if (rv == RT_OK) rv = node_program_resident(ws, d, node, kind, flags, st, &np);
    if (rv != RT_OK) return rv;
    SceneView S;
    scene_view(ws, d, flags, false, S);
    S.n_chunks = 0;
    const size_t chunk = host ? std::min(n, g_chunk_items.load()) : n;
    if (host) {
        HIP_TRY(ws.q_rays.ensure(chunk * sizeof(rt_ray)));
        if (enter) HIP_TRY(ws.q_hits.ensure(chunk * sizeof(rt_hit)));
        if (ex) HIP_TRY(ws.q_exit.ensure(chunk * sizeof(rt_hit)));
        if (mask) HIP_TRY(ws.q_mask.ensure(chunk));
    }
    // a chunk on the device: the staging buffers, or the caller's (one chunk)
    const rt_ray* d_rays = host ? ws.q_rays.as<rt_ray>() : rays;
    rt_hit* d_enter = !enter ? nullptr : host ? ws.q_hits.as<rt_hit>() : enter;
    rt_hit* d_exit = !ex ? nullptr : host ? ws.q_exit.as<rt_hit>() : ex;
    uint8_t* d_mask = !mask ? nullptr : host ? ws.q_mask.as<uint8_t>() : mask;
    rv = call.run(
        n, chunk, kLaunchItems,
        [&](size_t c0, size_t cn) -> int {
            if (host) HIP_TRY(hipMemcpyAsync(ws.q_rays.p, rays + c0, cn * sizeof(rt_ray), hipMemcpyHostToDevice, st));
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
// host memory, filled through the workspace's ray staging buffer (q_rays, the
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
    if (!rows_host) {
        all_rows.resize(n_rows);
        for (int r = 0; r < n_rows; ++r) all_rows[r] = r;
        rows_host = all_rows.data();
    } else {
        std::vector<char> seen(H, 0);
        for (int i = 0; i < n_rows; ++i) {
            if (rows_host[i] < 0 || rows_host[i] >= H) return call.fail("row out of range", RT_ERR_INVALID_ARG);
            if (seen[rows_host[i]]++) return call.fail("duplicate row", RT_ERR_INVALID_ARG);
            in_order = in_order && rows_host[i] == i;
        }
    }
    call.zero_stats(stats);
    if (n_rows == 0) return RT_OK;
    if (!rays) return call.fail("the ray buffer is NULL", RT_ERR_INVALID_ARG);
    int rv = call.open();
    if (rv != RT_OK) return rv;
    Workspace& ws = *call.ws;
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
        HIP_TRY(hipEventRecord(ws.ev[0], st));
        bool filled = false;
        rv = jitter_draws(ws, what, W, H, n_rows, plan, st, &jent, &filled);
        if (rv != RT_OK) return rv;
        HIP_TRY(hipEventRecord(ws.ev[1], st));
        // (the plan's vectors must outlive the upload: wait here, once per call)
        HIP_TRY(hipStreamSynchronize(st));
        if (filled) rtamd::note_launch("rtamd", "k_mt_fill_w");
        (void)hipEventElapsedTime(&ms_rng, ws.ev[0], ws.ev[1]);
        P.rows = jent->rows();
        P.jrow = jent->rows() + n_rows;
        P.jit = jent->jit();
    } else if (!in_order) {
        HIP_TRY(ws.cam_rows.ensure((size_t)n_rows * sizeof(int32_t)));
        HIP_TRY(rtamd::upload_async(&ws.up, ws.cam_rows.p, rows_host, (size_t)n_rows * sizeof(int32_t), st));
        P.rows = ws.cam_rows.as<int32_t>();
    }
    const size_t per_row = (size_t)W * (jittered ? RT_SPP : 1);
    // list entries of one launch: the grid's y extent; of one host chunk: its rays
    const size_t launch_rows = 65535;
    const size_t chunk_rows = host ? std::min<size_t>(n_rows, std::max<size_t>(1, g_chunk_items.load() / per_row)) : n_rows;
    if (host) HIP_TRY(ws.q_rays.ensure(chunk_rows * per_row * sizeof(rt_ray)));
    rt_ray* d_rays = host ? ws.q_rays.as<rt_ray>() : rays;
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
    ws.jcache.complete(jent);
    rv = call.finish();
    if (rv != RT_OK || !stats) return rv;
    stats->pixels = (uint64_t)n_rows * W;
    stats->ms_rng = ms_rng;
    return RT_OK;
}

// ------------------------------------------------------------- bounce loop
// Parents of one launch group of rt_scatter_rays_device: kLaunchItems unless
// rt_test_scatter_launch_items sets another size.
std::atomic<size_t> g_scatter_items{kLaunchItems};

// rt_scatter_rays_device: the children of n parents (rays[i], hits[i]) at
// recursion depth `depth`, compacted in parent order (rt_bounce_f64.hip: count,
// scan, emit per launch group; the group's child total is read back and
// carried into the next group's first index).  Every buffer is device memory
// but n_children.  Reads the resident scene's materials, medium index and
// recursion limit and leaves the resident copy as it was.
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
    const rt_scene_desc& d = *rt_scene_get_desc(s);
    rv = scene_resident(ws, s, d, false, st);
    if (rv != RT_OK) return rv;
    const size_t group = std::min(std::max<size_t>(g_scatter_items.load(), 1), kLaunchItems);
    // [0, 8): the group's child total; behind it the scan's words
    HIP_TRY(ws.scatter_tmp.ensure(8 + rtamd::scatter_count_words(std::min(n, group)) * sizeof(uint32_t)));
    rtamd::ScatterParams P0{};
    P0.mats = ws.mats.p;
    P0.n_mats = d.n_materials;
    P0.can = rtamd::bounce_can_spawn(depth, d.recursion_limit) ? 1 : 0;
    P0.medium_index = d.medium_index;
    P0.child_rays = child_rays;
    P0.child_w = child_w;
    P0.child_cap = child_cap;
    P0.total = ws.scatter_tmp.as<uint64_t>();
    P0.counts = ws.scatter_tmp.as<uint32_t>() + 2;
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

extern "C" int rt_test_camera_chunk_rays(size_t n) {
    g_chunk_items.store(n ? n : kChunkItems);
    return RT_OK;
}

extern "C" int rt_test_scatter_launch_items(size_t n) {
    g_scatter_items.store(n ? std::min(n, kLaunchItems) : kLaunchItems);
    return RT_OK;
}

void rtamd::set_workspace_slot(int slot) { t_ws_slot = slot; }

namespace {
// dst <- page-locked host src, 16-byte words (+ a byte tail), read by the GPU over PCIe
__global__ void k_host_copy(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n16, int tail) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x)
        dst[i] = src[i];
    if (blockIdx.x == 0 && (int)threadIdx.x < tail)
        reinterpret_cast<unsigned char*>(dst + n16)[threadIdx.x] = reinterpret_cast<const unsigned char*>(src + n16)[threadIdx.x];
}
}  // namespace

hipError_t rtamd::host_copy_async(void* dst, const void* src, size_t n, hipStream_t st) {
    if (!n) return hipSuccess;
    if ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15)
        return hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, st);
    const size_t n16 = n / 16;
    const int tail = (int)(n - n16 * 16);
    const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>(1024, (n16 + 255) / 256));
    hipLaunchKernelGGL(k_host_copy, dim3(blocks), dim3(256), 0, st, static_cast<const uint4*>(src),
                       static_cast<uint4*>(dst), n16, tail);
    return hipGetLastError();
}

extern "C" int rt_warmup(int what) {
    if (what & ~(RT_WARM_HOST | RT_WARM_DEVICE)) {
        rtamd::set_last_error("rt_warmup: unknown bits");
        return RT_ERR_INVALID_ARG;
    }
    if (what & RT_WARM_HOST) {
        try {
            rtamd::mt_prefetch_host_taps();
        } catch (const std::exception& e) {
            rtamd::set_last_error(std::string("rt_warmup: ") + e.what());
            return RT_ERR_PROCESSING;
        }
    }
    if (what & RT_WARM_DEVICE) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
            rtamd::set_last_error("rt_warmup: no HIP device available");
            return RT_ERR_NO_DEVICE;
        }
        // the FP64 render kernels' code object (one per fat binary and
        // device, loaded at its first use; hipFuncGetAttributes loads it)
        hipFuncAttributes a{};
        rtamd::KernelVariant lean;   // (k_std_lean<false, 1, false>)
        lean.wv = 1;
        HIP_TRY(hipFuncGetAttributes(&a, rtamd::trace_kernel(lean, false).fn));
    }
    return RT_OK;
}

hipError_t rtamd::warm_copy_engine(hipStream_t st) {
    static std::mutex mu;
    static bool done = false;
    static void* dev = nullptr;
    static std::vector<char> host;
    std::lock_guard<std::mutex> lk(mu);
    if (done) return hipSuccess;
    done = true;   // (one attempt: the copy is an optimisation only)
    // a 1 MiB read-back into pageable memory takes the same runtime path as
    // a frame's read-back (its staging set-up is the ~8 ms first-copy cost);
    // issued behind the first trace launch, the host spends that time while
    // the trace runs (the call returns when the copy has run)
    constexpr size_t kBytes = (size_t)1 << 20;
    rtamd::SetupTimer tm(rtamd::kSetupCopyEngine);
    if (hipMalloc(&dev, kBytes) != hipSuccess) return hipSuccess;
    host.resize(kBytes);
    return hipMemcpyAsync(host.data(), dev, kBytes, hipMemcpyDeviceToHost, st);
}

void rtamd::note_setup_ms(int slot, double ms) {
    if (slot < 4 || slot >= kSetupSlots) return;
    std::lock_guard<std::mutex> lk(g_setup.mu);
    if (slot < kLastBegin || slot == kLastTrace || slot == kSetupCopyEngine) g_setup.extra[slot] += ms;
    else g_setup.extra[slot] = ms;
}

int rtamd::release_device_workspaces(int min_slot) {
    int prev = 0;
    if (hipGetDevice(&prev) != hipSuccess) return RT_ERR_NO_DEVICE;
    if (min_slot <= 0) {
        std::lock_guard<std::mutex> lk(g_fb_mu);
        if (g_fb.p) {
            (void)hipSetDevice(g_fb_dev);
            g_fb.release();
        }
    }
    std::lock_guard<std::mutex> lk(g_ws_mu);
    for (auto& kv : g_ws) {
        Workspace* w = kv.second;
        const int dev = kv.first.first;
        if (!w || kv.first.second < min_slot) continue;
        std::lock_guard<std::mutex> wl(w->mu);   // waits for an open frame of this device
        (void)hipSetDevice(dev);
        (void)hipDeviceSynchronize();
        for (DBuf* b : {&w->nodes, &w->mats, &w->lights, &w->dlights, &w->objs, &w->ops, &w->gb, &w->ctab, &w->lrec,
                        &w->lwrec, &w->lgb, &w->fold,
                        &w->wobjs, &w->wctab, &w->worig, &w->wchunk,
                        &w->nodes_f, &w->mats_f, &w->lights_f, &w->dlights_f, &w->fold_f, &w->ckpt,
                        &w->jscratch, &w->counters, &w->paper_i, &w->paper_d, &w->paper_aux, &w->fb, &w->gtime,
                        &w->q_rays, &w->q_hits, &w->q_mask, &w->q_rgb, &w->q_wo, &w->q_exit, &w->q_lights, &w->cam_rows,
                        &w->scatter_tmp})
            b->release();
        release_node_programs(*w);
        release_ray_bvh(*w);
        w->jtab.release();
        w->jcache.release();   // every cached entry and the uncached buffer (the hit / miss counts stay)
        w->counters_zero = false;
        w->up.release();
        if (w->ctr_host) (void)hipHostFree(w->ctr_host);
        w->ctr_host = nullptr;
        w->ctr_host_words = 0;
        w->paper_cost.clear();
        for (auto& e : w->ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
        for (auto& e : w->tev)
            if (e) (void)hipEventDestroy(e);
        w->tev.clear();
        for (auto& e : w->pev)
            if (e) (void)hipEventDestroy(e);
        w->pev.clear();
        if (w->aux_st) (void)hipStreamDestroy(w->aux_st);
        w->aux_st = nullptr;
        w->sc = SceneCache();
    }
    (void)hipSetDevice(prev);
    return RT_OK;
}

// ------------------------------------------------- test hooks (rt_test.h)
// The jitter cache of workspace (current device, slot).  Takes the workspace
// lock: not for a thread that holds an open frame of that workspace.
extern "C" int rt_test_jitter_cache_stats_slot(int slot, uint64_t* hits, uint64_t* misses, uint64_t* entries,
                                               uint64_t* bytes) {
    if (!hits || !misses || !entries || !bytes) return RT_ERR_INVALID_ARG;
    *hits = *misses = *entries = *bytes = 0;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    Workspace* w = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_ws_mu);
        const auto it = g_ws.find({dev, slot});
        if (it != g_ws.end()) w = it->second;
    }
    if (!w) return RT_OK;   // (no frame of that slot yet)
    std::lock_guard<std::mutex> wl(w->mu);
    *hits = w->jcache.hits();
    *misses = w->jcache.misses();
    *entries = w->jcache.entries();
    *bytes = w->jcache.bytes();
    return RT_OK;
}

extern "C" int rt_test_jitter_cache_stats(uint64_t* hits, uint64_t* misses, uint64_t* entries, uint64_t* bytes) {
    return rt_test_jitter_cache_stats_slot(t_ws_slot, hits, misses, entries, bytes);
}

extern "C" int rt_test_jitter_cache_budget(int64_t bytes) {
    int prev = 0;
    HIP_TRY(hipGetDevice(&prev));
    rtamd::set_jitter_cache_budget(bytes);
    std::lock_guard<std::mutex> lk(g_ws_mu);
    for (auto& kv : g_ws) {
        Workspace* w = kv.second;
        if (!w) continue;
        std::lock_guard<std::mutex> wl(w->mu);   // waits for an open frame of this workspace
        (void)hipSetDevice(kv.first.first);
        w->jcache.clear();
        w->jcache.reset_counts();
    }
    (void)hipSetDevice(prev);
    return RT_OK;
}

// ------------------------------------------------------------------ C-ABI
extern "C" int rt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int rt_setup_times(double* out, int n) {
    if (!out || n < 0) return RT_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_setup.mu);
    const double v[4] = {g_setup.scene_ms, g_setup.jtable_ms, g_setup.trace_launch_ms, g_setup.jitter_launch_ms};
    for (int i = 0; i < n && i < rtamd::kSetupSlots; ++i) out[i] = i < 4 ? v[i] : g_setup.extra[i];
    return RT_OK;
}

extern "C" int rt_set_device(int device) {
    HIP_TRY(hipSetDevice(device));
    return RT_OK;
}

extern "C" int rt_device_alloc(size_t bytes, void** dev_out) {
    if (!dev_out) { rtamd::set_last_error("rt_device_alloc: NULL"); return RT_ERR_INVALID_ARG; }
    *dev_out = nullptr;
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, bytes ? bytes : 1));
    const hipError_t e = hipMemset(p, 0, bytes ? bytes : 1);
    if (e != hipSuccess) {
        (void)hipFree(p);
        rtamd::set_last_error(std::string("rt_device_alloc: hipMemset failed: ") + hipGetErrorString(e));
        return RT_ERR_HIP;
    }
    *dev_out = p;
    return RT_OK;
}

extern "C" int rt_device_free(void* dev) {
    if (dev) HIP_TRY(hipFree(dev));
    return RT_OK;
}

extern "C" int rt_memcpy_h2d(void* dev, const void* host, size_t bytes) {
    if (!bytes) return RT_OK;
    if (!dev || !host) { rtamd::set_last_error("rt_memcpy_h2d: NULL"); return RT_ERR_INVALID_ARG; }
    HIP_TRY(hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice));
    return RT_OK;
}

extern "C" int rt_memcpy_d2h(void* host, const void* dev, size_t bytes) {
    if (!bytes) return RT_OK;
    if (!dev || !host) { rtamd::set_last_error("rt_memcpy_d2h: NULL"); return RT_ERR_INVALID_ARG; }
    HIP_TRY(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

extern "C" int rt_device_synchronize(void) {
    HIP_TRY(hipDeviceSynchronize());
    return RT_OK;
}

extern "C" int rt_stream_create(void** stream_out) {
    if (!stream_out) { rtamd::set_last_error("rt_stream_create: NULL"); return RT_ERR_INVALID_ARG; }
    hipStream_t st = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    *stream_out = st;
    return RT_OK;
}

extern "C" int rt_stream_destroy(void* stream) {
    if (stream) HIP_TRY(hipStreamDestroy((hipStream_t)stream));
    return RT_OK;
}

extern "C" int rt_host_register(void* host, size_t bytes) {
    if (!host || !bytes) { rtamd::set_last_error("rt_host_register: NULL or empty"); return RT_ERR_INVALID_ARG; }
    HIP_TRY(hipHostRegister(host, bytes, hipHostRegisterDefault));
    return RT_OK;
}

extern "C" int rt_host_unregister(void* host) {
    if (!host) { rtamd::set_last_error("rt_host_unregister: NULL"); return RT_ERR_INVALID_ARG; }
    HIP_TRY(hipHostUnregister(host));
    return RT_OK;
}

extern "C" int rt_render_rows_device(const rt_scene* s, int W, int H, int mode, int flags, const int32_t* rows_host,
                                     int n_rows, double* fb_rows_dev, void* hip_stream, rt_stats* stats) {
    return render_rows_impl(s, W, H, mode, flags, rows_host, n_rows, fb_rows_dev, (hipStream_t)hip_stream, stats);
}

extern "C" int rt_frame_begin(const rt_scene* s, int W, int H, int mode, int flags, const int32_t* rows_host,
                              int n_rows, void* hip_stream, rt_frame** out) {
    return frame_begin(s, W, H, mode, flags, rows_host, n_rows, (hipStream_t)hip_stream, out);
}

extern "C" int rt_frame_trace(rt_frame* f, int ri0, int ri1, double* fb_rows_dev, void* hip_stream) {
    return frame_trace(f, ri0, ri1, fb_rows_dev, (hipStream_t)hip_stream);
}

extern "C" int rt_frame_end(rt_frame* f, rt_stats* stats) { return frame_end(f, stats); }

int rtamd::frame_trace_paper_codes(rt_frame* f, int ri0, int ri1, uint8_t* codes_rows_dev, void* hip_stream) {
    return frame_trace(f, ri0, ri1, nullptr, (hipStream_t)hip_stream, codes_rows_dev);
}

extern "C" int rt_render(const rt_scene* s, int W, int H, int mode, int flags, double* fb_host, rt_stats* stats) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!fb_host) { rtamd::set_last_error("rt_render: fb is NULL"); return RT_ERR_INVALID_ARG; }
    if (W <= 0 || H <= 0) { rtamd::set_last_error("rt_render: W and H must be > 0"); return RT_ERR_INVALID_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        rtamd::set_last_error("rt_render: no HIP device available");
        return RT_ERR_NO_DEVICE;
    }
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::vector<int32_t> rows(H);
    for (int r = 0; r < H; ++r) rows[r] = r;
    std::lock_guard<std::mutex> lk(g_fb_mu);
    DBuf& fb = g_fb;
    const size_t bytes = (size_t)W * H * 3 * sizeof(double);
    if (fb.p && g_fb_dev != dev) fb.release();   // (a staging frame lives on one device)
    HIP_TRY(fb.ensure(bytes));
    g_fb_dev = dev;
    int rc = render_rows_impl(s, W, H, mode, flags, rows.data(), H, fb.as<double>(), nullptr, stats);
    if (rc != RT_OK) return rc;
    const auto t1 = std::chrono::steady_clock::now();
    HIP_TRY(hipMemcpy(fb_host, fb.p, bytes, hipMemcpyDeviceToHost));
    if (stats) {
        const auto t2 = std::chrono::steady_clock::now();
        stats->ms_d2h = std::chrono::duration<double, std::milli>(t2 - t1).count();
        stats->ms_total = std::chrono::duration<double, std::milli>(t2 - t0).count();
    }
    return RT_OK;
}

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

extern "C" int rt_scatter_rows_device(const double* src_dev, const int32_t* rows_dev, int n_rows, int W,
                                      double* fb_dev, void* hip_stream) {
    if (n_rows <= 0) return RT_OK;
    if (!src_dev || !rows_dev || !fb_dev || W <= 0) { rtamd::set_last_error("rt_scatter_rows_device: bad args"); return RT_ERR_INVALID_ARG; }
    const size_t total = (size_t)W * 3 * n_rows;
    const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(k_scatter_rows, dim3(blocks), dim3(256), 0, (hipStream_t)hip_stream, src_dev, rows_dev, n_rows,
                       W, fb_dev);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

extern "C" int rt_framebuffer_to_rgb8_device(const double* fb_dev, size_t n_pixels, uint8_t* rgb8_dev,
                                             void* hip_stream) {
    if (!n_pixels) return RT_OK;
    if (!fb_dev || !rgb8_dev) { rtamd::set_last_error("rt_framebuffer_to_rgb8_device: NULL"); return RT_ERR_INVALID_ARG; }
    const size_t n = n_pixels * 3;
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(k_to_rgb8, dim3(blocks), dim3(256), 0, (hipStream_t)hip_stream, fb_dev, n, rgb8_dev);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}
