// rt_workspace.hpp — what the host files of librtamd's renderer share: the
// per-device workspace and the scene resident in it (rt_workspace.hip), held by
// a frame (rt_frame.hip) or a batched call (rt_batch.hip) through one
// WorkspaceSession.  The workspace is four groups of device resources, each
// with its release() next to its members: a buffer added to a group is named
// in that group only.  Nothing frees itself at exit (a hipFree after the
// runtime has gone is a crash): rt_shutdown releases the groups.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstdint>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "jitter_cache.hpp"
#include "mt_jump.hpp"
#include "pinned.hpp"
#include "rt.h"
#include "rt_devbuf.hpp"
#include "rt_internal.hpp"
#include "rt_launch.hpp"
#include "scene_compile.hpp"

// (hidden: internal to librtamd, like the unnamed namespaces these came from)
namespace rtw __attribute__((visibility("hidden"))) {

using DBuf = rtamd::DevBufT<8>;   // (growth slack 1/8)
using SClock = std::chrono::steady_clock;
inline double ms_since(SClock::time_point t) { return std::chrono::duration<double, std::milli>(SClock::now() - t).count(); }

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
extern SetupTimes g_setup;
// Adds its lifetime to rt_setup_times[0]: a scene's, a ray BVH's or a node
// program's compile + upload enqueue, however the function leaves.
struct SceneSetupTime {
    const SClock::time_point t = SClock::now();
    ~SceneSetupTime() {
        std::lock_guard<std::mutex> lk(g_setup.mu);
        g_setup.scene_ms += ms_since(t);
    }
};

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

// One node's compiled program (compile_node_program) next to the resident
// scene: built and uploaded by the first query of (node, kind), found there by
// every later one.  A leaf has no ops (its row reads the node itself).
struct NodeProg {
    rtamd::KernelVariant kv;          // pick_node_variant: the row and its namespace
    std::vector<rtamd::DevOp> host;   // source of the upload (kept alive)
    DBuf ops;
};

// ---- group 1: the resident scene.  scene_resident uploads it, scene_view
// hands it to a launch, release() frees it (all in rt_workspace.hip, together).
struct ResidentScene {
    SceneCache sc;
    DBuf nodes, mats, lights, dlights, fold;      // records: FP64, or the float copies (sc.fp32)
    DBuf objs, ops, gb, ctab, lrec, lwrec, lgb;   // compiled object table (CompiledScene::objs ...)
    DBuf wobjs, wctab, worig, wchunk;             // wave BVH (CompiledScene::wobjs ...)
    // node queries: the programs of the scene's nodes queried so far, by (node,
    // kind) (node_program_resident)
    std::map<std::pair<int, int>, NodeProg> node_progs;
    // ray queries with RT_FLAG_RAY_BVH: the scene's ray BVH
    // (CompiledScene::rnodes), uploaded by the first such query (ray_bvh_resident)
    DBuf rnodes;
    bool rnodes_resident = false;

    // The node programs and the ray BVH belong to the scene they were made for:
    // they go when it goes.  (No launch reads them then: a call that used one
    // has drained its stream.)
    void release_derived() {
        for (auto& kv : node_progs) kv.second.ops.release();
        node_progs.clear();
        rnodes.release();
        rnodes_resident = false;
    }
    void release() {
        for (DBuf* b : {&nodes, &mats, &lights, &dlights, &fold, &objs, &ops, &gb, &ctab, &lrec, &lwrec, &lgb, &wobjs,
                        &wctab, &worig, &wchunk})
            b->release();
        release_derived();
        sc = SceneCache();
    }
};

// Device memory of the jitter cache's buffers (jitter_cache.hpp), on the
// current device.
void* jitter_alloc(size_t bytes);
void jitter_free(void* p);

// ---- group 2: what frames are made of beside the scene (the batched calls
// use the same draws and counters).
struct FrameBuffers {
    // standard mode: the frames' jitter draws and rows lists, resident by
    // (W, H, rows) so that only the first frame of a key generates them
    rtamd::JitterCache jcache{jitter_alloc, jitter_free};
    rtamd::JitterTable jtab;                  // mt19937(12345) checkpoint table (resident)
    rtamd::JitterJob jjob;
    DBuf jscratch;
    DBuf counters;                            // the ray / op counter slots (counters_ready)
    bool counters_zero = false;               // the last k_reduce_counters left `counters` zero (no memset)
    unsigned long long* ctr_host = nullptr;   // page-locked: the frame's reduced counters (k_reduce_counters)
    size_t ctr_host_words = 0;                //   + the paper-mode list-group costs behind them
    DBuf paper_i, paper_d, paper_aux;         // paper mode: the primary hits and the frame's lists
    DBuf gtime;                               // paper mode: primary waves' (start, end) ticks (paper_wave_slot)
    // paper mode: measured primary-pass cost of each 8-entry list group of a
    // frame, by the group's first ext index, per frame key (scene, size,
    // mode, flags, rows): the next frame of that key launches its groups
    // costliest first (frame_plan.hpp order_paper_groups)
    std::map<uint64_t, std::vector<uint32_t>> paper_cost;

    void release() {
        for (DBuf* b : {&jscratch, &counters, &paper_i, &paper_d, &paper_aux, &gtime}) b->release();
        jtab.release();
        jcache.release();   // every cached entry and the uncached buffer (the hit / miss counts stay)
        counters_zero = false;
        if (ctr_host) (void)hipHostFree(ctr_host);
        ctr_host = nullptr;
        ctr_host_words = 0;
        paper_cost.clear();
    }
};

// ---- group 3: one chunk of a batched call from host memory, and the calls'
// own small buffers.
struct QueryBuffers {
    DBuf rays, hits, mask, rgb;   // ray queries: one chunk's rays / hits / flags / colours
    DBuf wo;                      // shading queries: one chunk's view directions
    DBuf exit;                    // node interval queries: one chunk's exit records
    DBuf lights;                  // a shading query's own point lights (never the resident scene's `lights`)
    DBuf cam_rows;                // rt_camera_rays, centre rays: a rows list that is not 0, 1, 2, ...
    DBuf scatter_tmp;             // rt_scatter_rays_device: a launch group's child total + its scan's words

    void release() {
        for (DBuf* b : {&rays, &hits, &mask, &rgb, &wo, &exit, &lights, &cam_rows, &scatter_tmp}) b->release();
    }
};

// ---- group 4: the events and the second stream.
struct WorkspaceSync {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // a frame's begin, jitter done, traces done, counters reduced
    std::vector<hipEvent_t> tev;   // one per rt_frame_trace call of the open frame (pool)
    std::vector<hipEvent_t> pev;   // paper mode: the end of each call's primary pass (pool)
    hipStream_t aux_st = nullptr;  // render_rows_impl: a paper frame's odd chunks

    int ensure_events() {
        if (ev[0]) return RT_OK;
        rtamd::SetupTimer tm(rtamd::kSetupStreams);
        for (int i = 0; i < 4; ++i) HIP_TRY(hipEventCreate(&ev[i]));
        return RT_OK;
    }
    // pool[i], made on its first use
    static int pooled(std::vector<hipEvent_t>& pool, int i, hipEvent_t* out) {
        if ((int)pool.size() <= i) {
            hipEvent_t e = nullptr;
            HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            pool.push_back(e);
        }
        *out = pool[i];
        return RT_OK;
    }
    void release() {
        for (auto& e : ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
        for (std::vector<hipEvent_t>* pool : {&tev, &pev}) {
            for (hipEvent_t e : *pool)
                if (e) (void)hipEventDestroy(e);
            pool->clear();
        }
        if (aux_st) (void)hipStreamDestroy(aux_st);
        aux_st = nullptr;
    }
};

// Per-device workspace (one frame or batched call at a time per device;
// guarded by a mutex).
struct Workspace {
    std::mutex mu;
    ResidentScene scene;
    FrameBuffers frame;
    QueryBuffers q;
    WorkspaceSync sync;
    rtamd::PinnedArena up;   // page-locked staging of a frame's or call's uploads (pinned.hpp)

    void release() {
        scene.release();
        frame.release();
        q.release();
        sync.release();
        up.release();
    }
};

// Workspaces by (device, slot).  Slot 0 is the process's own; the simulated
// ranks of rt_test_dist_threads run on one device concurrently, each on its
// own host thread with its own slot (rtamd::set_workspace_slot), as separate
// processes would hold separate workspaces.  Never deleted (frames hold
// pointers); emptied by rt_shutdown.
Workspace& workspace(int dev);            // of the calling thread's slot; made on its first use
Workspace* find_workspace(int dev, int slot);   // (null: none yet)
int workspace_slot();                     // the calling thread's
// fn(w) on every workspace of slot >= min_slot, under its lock (waits for an
// open frame of it) with its device current.  The caller restores the device.
void each_workspace(int min_slot, const std::function<void(Workspace&)>& fn);
// rt_render's staging frame (rt_frame.hip; one per process, not a workspace's)
void release_staging_frame();

// One holder of a device workspace at a time: a frame for its lifetime, a
// batched call until its end.  open() checks that there is a device, takes the
// current device's workspace and its lock, resets the staging arena (the
// previous holder's uploads completed) and makes sure of the events.  Nothing
// of the holder may stay queued on st when the lock goes (the next holder
// resets the arena its uploads read, and reuses its buffers): the destructor
// drains st, and runs before the lock is destroyed - unless disarm() said that
// the holder's own end sees to it (rt_frame_end).  A holder that owns host
// sources of uploads declares its session after them, so that it drains first.
struct WorkspaceSession {
    Workspace* ws = nullptr;
    std::unique_lock<std::mutex> lock;
    hipStream_t st = nullptr;
    bool drain = false;

    ~WorkspaceSession() {
        if (drain) (void)hipStreamSynchronize(st);
    }
    int open(const char* what, hipStream_t st_);   // failures are reported under `what`
    void disarm() { drain = false; }
};

// ---- residency (rt_workspace.hip); the caller holds a session
int scene_resident(Workspace& ws, const rt_scene* s, const rt_scene_desc& d, bool fp32, hipStream_t st);
void scene_view(const Workspace& ws, const rt_scene_desc& d, int flags, rtamd::SceneView& S);
int ray_bvh_resident(Workspace& ws, hipStream_t st);
int node_program_resident(Workspace& ws, const rt_scene_desc& d, int node, int kind, int flags, hipStream_t st,
                          const NodeProg** out);
int ensure_ctr_host(Workspace& ws, size_t host_words);
int counters_ready(Workspace& ws, hipStream_t st);
int jitter_plan_ready(Workspace& ws, int W, int H, const int32_t* rows_host, int n_rows, hipStream_t st,
                      rtamd::StdPlan& plan);
int jitter_draws(Workspace& ws, const char* what, int W, int H, int n_rows, const rtamd::StdPlan& sp, hipStream_t st,
                 rtamd::JitterCache::Entry** ent, bool* filled = nullptr);

// The rows list of an H-row frame: every entry in [0, H), none twice; else
// RT_ERR_INVALID_ARG and "<what>: row out of range" / "<what>: duplicate row"
// (what == nullptr: no message, rt_last_error() is left as it was).
// *in_order (may be null): whether entry i is row i.
int check_rows(const char* what, int H, const int32_t* rows, int n_rows, bool* in_order = nullptr);

// k_reduce_counters (rt_render.hip) on st: the counter slots summed into
// `out` (page-locked) and left zero; n_groups > 0: also the wave times of that
// many paper-mode list groups of wpg waves each, from gtime.
hipError_t launch_reduce_counters(hipStream_t st, unsigned long long* slots, unsigned long long* out,
                                  const unsigned int* gtime, int wpg, int n_groups);

// Items (rays, hits, list rows) of one launch of a batched call: 2^30 (the
// grid's x extent holds 2^31 - 1 one-wave workgroups).  Items of one chunk of a
// call from host memory: g_chunk_items, 2^20 unless rt_test_camera_chunk_rays
// sets another size - for rays 64 MiB of rays + 64 MiB of hits + 1 MiB of flags
// in the workspace, large enough that a chunk's launch and copy overheads
// vanish in its transfers.  (The camera rays count it in rays and take whole
// rows.)  Parents of one launch group of rt_scatter_rays_device:
// g_scatter_items, kLaunchItems unless rt_test_scatter_launch_items sets
// another size.
constexpr size_t kLaunchItems = (size_t)1 << 30;
constexpr size_t kChunkItems = (size_t)1 << 20;
extern std::atomic<size_t> g_chunk_items, g_scatter_items;

}  // namespace rtw
