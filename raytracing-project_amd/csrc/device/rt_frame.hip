// rt_frame.hip — the frame path of librtamd: rt_frame_begin / trace / end on
// the device workspace (rt_workspace.hpp), and rt_render and
// rt_render_rows_device built from them.
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
// PaperCalls); rt_frame_begin / trace / end here execute that plan.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <memory>

#include "rt_test.h"
#include "rt_workspace.hpp"

using namespace rtw;
using rtamd::kCounterWords;
using rtamd::PaperParams;
using rtamd::SceneView;
using rtamd::StdParams;

// One frame in flight on one device (rt_frame_begin .. rt_frame_end).  Holds
// the device workspace (its session, so its lock) for its lifetime; every
// launch is stream-ordered on `st`, and every host buffer an async upload
// reads stays alive here until the stream has been synchronised: by
// rt_frame_end, or, for a frame whose begin fails, by the session, which is the
// LAST member so that it is destroyed - and drains st - before the plans are.
struct rt_frame {
    hipStream_t st = nullptr;
    SceneView S;
    int W = 0, H = 0, mode = 0, n_rows = 0;
    rtamd::KernelVariant kv;                   // the frame's trace kernel (frame_plan.hpp pick_variant)
    bool fp32 = false;
    bool timed = false;                        // paper mode: a launch stored its waves' ticks (PaperParams::gtime)
    int bvh_trial = -1;                        // SceneCache::bvh_trial this frame measures (-1: none)
    SClock::time_point t_start;
    rtamd::StdPlan std_plan;                   // standard mode (host source of the rows upload)
    rtamd::JitterCache::Entry* jent = nullptr; //   its buffer in the workspace's jcache (valid once this frame has ended well)
    const double* jit = nullptr;               //   the draws, 16 per pixel by jitter row
    const int32_t* rows = nullptr;             //   rows | jitter row of each, on the device
    rtamd::PaperPlan paper;                    // paper mode (host source of the aux upload)
    rtamd::PaperCalls paper_calls;             //   its trace calls' lists (host sources of their uploads)
    std::vector<hipStream_t> call_st;          // stream of each trace call (sync.tev[i] its end)
    WorkspaceSession ses;                      // ses.ws: the workspace (last: see above)
};

namespace {

// RT_BVH_AB (measurement A/B; default 1): 0 = a scene with a wave BVH always
// uses it (no trial frames, SceneCache::bvh_trial).
bool bvh_ab() {
    static const bool on = [] { const char* e = std::getenv("RT_BVH_AB"); return !(e && *e == '0'); }();
    return on;
}

// rt_render's staging frame (host-output path), one per process
std::mutex g_fb_mu;
DBuf g_fb;
int g_fb_dev = 0;

int frame_begin(const rt_scene* s, int W, int H, int mode, int flags, const int32_t* rows_host, int n_rows,
                hipStream_t st, rt_frame** out) {
    const auto t_start = SClock::now();
    if (!out) { rtamd::set_last_error("rt_frame_begin: out is NULL"); return RT_ERR_INVALID_ARG; }
    *out = nullptr;
    if (!s) { rtamd::set_last_error("rt_render: scene is NULL"); return RT_ERR_INVALID_ARG; }
    if (W <= 0 || H <= 0) { rtamd::set_last_error("rt_render: W and H must be > 0"); return RT_ERR_INVALID_ARG; }
    if (mode != RT_MODE_STANDARD && mode != RT_MODE_PAPER) { rtamd::set_last_error("rt_render: bad mode"); return RT_ERR_INVALID_ARG; }
    if (n_rows < 0 || (n_rows > 0 && !rows_host)) { rtamd::set_last_error("rt_render: bad rows"); return RT_ERR_INVALID_ARG; }
    int rv = check_rows("rt_render", H, rows_host, n_rows);
    if (rv != RT_OK) return rv;
    // a failure below may leave uploads of this frame queued on st: f's
    // destruction begins with the session's, which drains st before the host
    // sources of those uploads (f's plans) and the workspace lock go; a frame
    // that has begun well drains its streams itself (frame_end)
    std::unique_ptr<rt_frame> f(new rt_frame);
    rv = f->ses.open("rt_render", st);
    if (rv != RT_OK) return rv;
    const rt_scene_desc& d = *rt_scene_get_desc(s);
    Workspace& ws = *f->ses.ws;
    const bool fp32 = (flags & RT_FLAG_FP32) != 0;
    SceneCache& sc = ws.scene.sc;
    rv = scene_resident(ws, s, d, fp32, st);
    if (rv != RT_OK) return rv;
    const rtamd::CompiledScene& cs = sc.cs;
    f->st = st;
    f->W = W;
    f->H = H;
    f->mode = mode;
    f->n_rows = n_rows;
    f->fp32 = fp32;
    f->t_start = t_start;
    rv = counters_ready(ws, st);
    if (rv != RT_OK) return rv;

    SceneView& S = f->S;
    scene_view(ws, d, flags, S);
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
    rv = rtamd::pick_variant(cs, d, mode, flags, S.n_chunks > 0, &f->kv);
    if (rv != RT_OK) return rv;

    if (n_rows > 0 && mode == RT_MODE_STANDARD) {
        rv = jitter_plan_ready(ws, W, H, rows_host, n_rows, st, f->std_plan);
        if (rv != RT_OK) return rv;
    }
    HIP_TRY(hipEventRecord(ws.sync.ev[0], st));
    if (n_rows > 0 && mode == RT_MODE_STANDARD) {
        rv = jitter_draws(ws, "rt_render", W, H, n_rows, f->std_plan, st, &f->jent);
        if (rv != RT_OK) return rv;
        f->jit = f->jent->jit();
        f->rows = f->jent->rows();
    } else if (n_rows > 0) {
        f->paper = rtamd::plan_paper_frame(rtamd::scene_uid(s), W, H, mode, flags, rows_host, n_rows);
        f->paper_calls.reset(&f->paper);
        const rtamd::PaperPlan& pp = f->paper;
        FrameBuffers& fr = ws.frame;
        HIP_TRY(fr.paper_aux.ensure(pp.aux_ints() * sizeof(int32_t)));
        HIP_TRY(fr.gtime.ensure(pp.gtime_words() * sizeof(unsigned)));
        HIP_TRY(rtamd::upload_async(&ws.up, fr.paper_aux.p, pp.aux.data(), pp.aux.size() * sizeof(int32_t), st));
        const size_t npx = (size_t)pp.n_ext * W;
        HIP_TRY(fr.paper_i.ensure(npx * sizeof(int)));
        HIP_TRY(fr.paper_d.ensure(npx * 4 * sizeof(double)));
    }
    HIP_TRY(hipEventRecord(ws.sync.ev[1], st));
    f->ses.disarm();
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
    Workspace& ws = *f->ses.ws;
    FrameBuffers& fr = ws.frame;
    WorkspaceSync& sy = ws.sync;
    const hipStream_t st = hs ? hs : f->st;
    const int W = f->W, n = ri1 - ri0;
    unsigned long long* ctr = fr.counters.as<unsigned long long>();
    // another stream first waits for the scene upload and jitter (begin).  In
    // paper mode a chunk whose finish pass reads primary hits that an earlier
    // call computed on another stream waits for that call's PRIMARY pass
    // (PaperCalls::next_call: one GPU's chunked frame, or adjacent strips of
    // one rank), and only its finish waits: its primary computes new entries
    // only, so it overlaps the earlier call's finish (latency-bound) on the
    // other stream.
    const auto t_launch = SClock::now();
    if (st != f->st) HIP_TRY(hipStreamWaitEvent(st, sy.ev[1], 0));
    const int call = (int)f->call_st.size();   // this call's index (sync.pev / sync.tev)
    hipEvent_t call_ev = nullptr;
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
        const auto cost_it = fr.paper_cost.find(pp.key);
        const bool have_cost = cost_it != fr.paper_cost.end();
        // primary hits of the ext rows this chunk reads that no earlier chunk computed
        const rtamd::PaperCalls::Call c = f->paper_calls.next_call(
            ri0, ri1, reinterpret_cast<uintptr_t>(st), order_mode >= 2 && have_cost ? &cost_it->second : nullptr);
        if (!c.ok) {
            rtamd::set_last_error("rt_frame_trace: paper-mode list overflow");
            return RT_ERR_PROCESSING;
        }
        undo.calls = &f->paper_calls;
        int32_t* aux = fr.paper_aux.as<int32_t>();
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
        P.mat = fr.paper_i.as<int>();
        double* dd = fr.paper_d.as<double>();
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
                P.gtime = fr.gtime.as<unsigned>() + (size_t)(c.list_off / 8) * rtamd::paper_waves_per_group(W) * 2;
                kv.timed = f->timed = true;
            }
            HIP_TRY(rtamd::upload_async(&ws.up, d_list, c.list->data(), c.list->size() * sizeof(int32_t), st));
            dim3 g1((W + 15) / 16, (P.n_list + 15) / 16);
            HIP_TRY(rtamd::launch_paper(kv, g1, st, f->S, P));
        }
        int rv = WorkspaceSync::pooled(sy.pev, call, &call_ev);
        if (rv != RT_OK) return rv;
        HIP_TRY(hipEventRecord(call_ev, st));
        for (int w : c.wait) HIP_TRY(hipStreamWaitEvent(st, sy.pev[w], 0));
        dim3 g2((W + 63) / 64, (n + 3) / 4);
        HIP_TRY(rtamd::launch_paper_finish(f->kv, g2, st, f->S, P));
    }
    {
        std::lock_guard<std::mutex> lk(g_setup.mu);
        if (!g_setup.trace_launched) g_setup.trace_launch_ms = ms_since(t_launch);
        g_setup.trace_launched = true;
    }
    const int rv = WorkspaceSync::pooled(sy.tev, call, &call_ev);
    if (rv != RT_OK) return rv;
    HIP_TRY(hipEventRecord(call_ev, st));
    rtamd::note_setup_ms(rtamd::kLastTrace, ms_since(t_launch));
    HIP_TRY(rtamd::warm_copy_engine(st));   // (once per process, while the trace runs)
    undo.calls = nullptr;
    f->call_st.push_back(st);
    return RT_OK;
}

int frame_end_body(rt_frame* f, rt_stats* stats) {
    Workspace& ws = *f->ses.ws;
    FrameBuffers& fr = ws.frame;
    WorkspaceSync& sy = ws.sync;
    const hipStream_t st = f->st;
    // join the other trace streams: one wait on each one's last call (stream
    // order covers its earlier ones; every wait is a barrier packet on st)
    for (size_t i = 0; i < f->call_st.size(); ++i) {
        if (f->call_st[i] == st) continue;
        bool last = true;
        for (size_t j = i + 1; j < f->call_st.size(); ++j) last = last && f->call_st[j] != f->call_st[i];
        if (last) HIP_TRY(hipStreamWaitEvent(st, sy.tev[i], 0));
    }
    HIP_TRY(hipEventRecord(sy.ev[2], st));
    const int n_groups = f->paper_calls.list_used() / 8;
    const size_t host_words = kCounterWords + ((size_t)n_groups + 1) / 2;
    {
        const int rv = ensure_ctr_host(ws, host_words);
        if (rv != RT_OK) return rv;
    }
    const bool timed = f->timed;   // (some launch of this frame stored its waves' ticks)
    HIP_TRY(launch_reduce_counters(st, fr.counters.as<unsigned long long>(), fr.ctr_host, fr.gtime.as<unsigned>(),
                                   rtamd::paper_waves_per_group(f->W), timed ? n_groups : 0));
    HIP_TRY(hipEventRecord(sy.ev[3], st));
    HIP_TRY(rtamd::spin_wait(sy.ev[3]));
    fr.counters_zero = true;
    // every stream of the frame has run to its end: the draws and the rows
    // list this frame wrote are complete, and later frames of its key may
    // read them (a frame that fails before this point leaves no valid entry)
    fr.jcache.complete(f->jent);
    unsigned long long hc[kCounterWords];
    for (int k = 0; k < kCounterWords; ++k) hc[k] = ((volatile unsigned long long*)fr.ctr_host)[k];
    if (timed) {
        // this frame's group costs, by each group's first ext index
        const uint64_t key = f->paper.key;
        if (fr.paper_cost.size() >= 64 && !fr.paper_cost.count(key)) fr.paper_cost.clear();
        const volatile unsigned int* gcv = reinterpret_cast<const volatile unsigned int*>(fr.ctr_host + kCounterWords);
        const std::vector<uint32_t> gc(gcv, gcv + n_groups);
        f->paper_calls.group_costs(gc.data(), fr.paper_cost[key]);
    }
    if (f->bvh_trial >= 0) {
        // the BVH trial frames: their trace kernels' time decides later frames
        SceneCache& sc = ws.scene.sc;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, sy.ev[1], sy.ev[2]) == hipSuccess && sc.bvh_trial == f->bvh_trial) {
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
        if (hipEventElapsedTime(&ms, sy.ev[0], sy.ev[1]) == hipSuccess) stats->ms_rng = ms;
        if (hipEventElapsedTime(&ms, sy.ev[1], sy.ev[2]) == hipSuccess) stats->ms_kernel = ms;
        for (int k = 0; k < 16; ++k) stats->ops[k] = hc[2 + k];
        stats->ms_total = ms_since(f->t_start);
        stats->n_gpus = 1;
    }
    return RT_OK;
}

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
    hipStream_t& aux_st = f->ses.ws->sync.aux_st;
    if (mode == RT_MODE_PAPER && rtamd::paper_chunks_1gpu() > 1) {
        if (!aux_st && hipStreamCreateWithFlags(&aux_st, hipStreamNonBlocking) != hipSuccess) aux_st = nullptr;
        if (aux_st) bounds = rtamd::row_chunks(n_rows, rtamd::paper_chunks_1gpu(), RT_PAPER_STRIP_ROWS);
    }
    for (size_t k = 0; k < bounds.size() && rc == RT_OK; ++k) {
        const hipStream_t cst = ((bounds.size() - 1 - k) & 1) ? aux_st : nullptr;
        rc = frame_trace(f, bounds[k].first, bounds[k].second, fb_dev + (size_t)bounds[k].first * W * 3, cst);
    }
    const int rc2 = frame_end(f, stats);
    return rc != RT_OK ? rc : rc2;
}

}  // namespace

void rtw::release_staging_frame() {
    std::lock_guard<std::mutex> lk(g_fb_mu);
    if (!g_fb.p) return;
    (void)hipSetDevice(g_fb_dev);
    g_fb.release();
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

// ------------------------------------------------------------------ C-ABI
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
    const auto t0 = SClock::now();
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
    const auto t1 = SClock::now();
    HIP_TRY(hipMemcpy(fb_host, fb.p, bytes, hipMemcpyDeviceToHost));
    if (stats) {
        const auto t2 = SClock::now();
        stats->ms_d2h = std::chrono::duration<double, std::milli>(t2 - t1).count();
        stats->ms_total = std::chrono::duration<double, std::milli>(t2 - t0).count();
    }
    return RT_OK;
}
