// rt_workspace.hip — the per-device workspaces of rt_workspace.hpp: the scene
// resident in one (compile + upload once, then found there by every frame and
// batched call), the frames' counters and jitter draws, the session that holds
// a workspace, and the release of everything at rt_shutdown.
#include "rt_workspace.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "mt_poly.hpp"

namespace rtw __attribute__((visibility("hidden"))) {

SetupTimes g_setup;
std::atomic<size_t> g_chunk_items{kChunkItems}, g_scatter_items{kLaunchItems};

namespace {
std::mutex g_ws_mu;
std::map<std::pair<int, int>, Workspace*> g_ws;
thread_local int t_ws_slot = 0;

template <class T>
hipError_t upload(DBuf& b, const std::vector<T>& v, hipStream_t st, rtamd::PinnedArena* up = nullptr) {
    size_t bytes = v.size() * sizeof(T);
    hipError_t e = b.ensure(bytes ? bytes : 16);
    if (e != hipSuccess || !bytes) return e;
    return rtamd::upload_async(up, b.p, v.data(), bytes, st);
}

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
}  // namespace

// ------------------------------------------------- workspaces and sessions
Workspace& workspace(int dev) {
    std::lock_guard<std::mutex> lk(g_ws_mu);
    Workspace*& w = g_ws[{dev, t_ws_slot}];
    if (!w) w = new Workspace;
    return *w;
}

Workspace* find_workspace(int dev, int slot) {
    std::lock_guard<std::mutex> lk(g_ws_mu);
    const auto it = g_ws.find({dev, slot});
    return it != g_ws.end() ? it->second : nullptr;
}

int workspace_slot() { return t_ws_slot; }

void each_workspace(int min_slot, const std::function<void(Workspace&)>& fn) {
    std::lock_guard<std::mutex> lk(g_ws_mu);
    for (auto& kv : g_ws) {
        Workspace* w = kv.second;
        if (!w || kv.first.second < min_slot) continue;
        std::lock_guard<std::mutex> wl(w->mu);
        (void)hipSetDevice(kv.first.first);
        fn(*w);
    }
}

int WorkspaceSession::open(const char* what, hipStream_t st_) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        rtamd::set_last_error(std::string(what) + ": no HIP device available");
        return RT_ERR_NO_DEVICE;
    }
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    ws = &workspace(dev);
    lock = std::unique_lock<std::mutex>(ws->mu);   // (waits for an open frame or call of this workspace)
    st = st_;
    drain = true;
    ws->up.reset();
    return ws->sync.ensure_events();
}

int check_rows(const char* what, int H, const int32_t* rows, int n_rows, bool* in_order) {
    const auto fail = [&](const char* msg) {
        if (what) rtamd::set_last_error(std::string(what) + ": " + msg);
        return (int)RT_ERR_INVALID_ARG;
    };
    std::vector<char> seen(H, 0);
    bool ordered = true;
    for (int i = 0; i < n_rows; ++i) {
        if (rows[i] < 0 || rows[i] >= H) return fail("row out of range");
        if (seen[rows[i]]++) return fail("duplicate row");
        ordered = ordered && rows[i] == i;
    }
    if (in_order) *in_order = ordered;
    return RT_OK;
}

// A failed allocation is the jitter cache's to handle (it frees entries or
// takes the uncached buffer), so the runtime's last-error slot is cleared: a
// later launch check must not report it.
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

// -------------------------------------------------------- the resident scene
// The scene resident in the workspace: compiled and uploaded once (on st), and
// found there by every later frame or ray query of it on the device.  The
// caller holds the workspace lock and has reset the staging arena.
int scene_resident(Workspace& ws, const rt_scene* s, const rt_scene_desc& d, bool fp32, hipStream_t st) {
    ResidentScene& r = ws.scene;
    SceneCache& sc = r.sc;
    if (sc.valid && sc.uid == rtamd::scene_uid(s) && sc.fp32 == fp32) return RT_OK;
    // compile + upload the scene once; later frames of it find it resident
    // (uploads from the page-locked arena: plain DMA, no pageable staging)
    SceneSetupTime add_time;
    sc.valid = false;
    r.release_derived();
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
    if (fp32) make_float_scene(sc);
    HIP_TRY(fp32 ? upload(r.nodes, sc.nodes_f, st, &ws.up) : upload(r.nodes, sc.nodes, st, &ws.up));
    HIP_TRY(fp32 ? upload(r.mats, sc.mats_f, st, &ws.up) : upload(r.mats, sc.mats, st, &ws.up));
    HIP_TRY(fp32 ? upload(r.lights, sc.lights_f, st, &ws.up) : upload(r.lights, sc.lights, st, &ws.up));
    HIP_TRY(fp32 ? upload(r.dlights, sc.dlights_f, st, &ws.up) : upload(r.dlights, sc.dlights, st, &ws.up));
    HIP_TRY(fp32 ? upload(r.fold, sc.fold_f, st, &ws.up) : upload(r.fold, sc.cs.fold, st, &ws.up));
    HIP_TRY(upload(r.objs, sc.cs.objs, st, &ws.up));
    HIP_TRY(upload(r.ops, sc.cs.ops, st, &ws.up));
    HIP_TRY(upload(r.gb, sc.cs.gbounds, st, &ws.up));
    HIP_TRY(upload(r.ctab, sc.cs.ctab, st, &ws.up));
    HIP_TRY(upload(r.lrec, sc.cs.lrec, st, &ws.up));
    HIP_TRY(upload(r.lwrec, sc.cs.lwrec, st, &ws.up));
    HIP_TRY(upload(r.lgb, sc.cs.lgb, st, &ws.up));
    HIP_TRY(upload(r.wobjs, sc.cs.wobjs, st, &ws.up));
    HIP_TRY(upload(r.wctab, sc.cs.wctab, st, &ws.up));
    HIP_TRY(upload(r.worig, sc.cs.worig, st, &ws.up));
    HIP_TRY(upload(r.wchunk, sc.cs.wchunk, st, &ws.up));
    sc.uid = rtamd::scene_uid(s);
    sc.fp32 = fp32;
    sc.valid = true;
    sc.bvh_trial = 0;   // (a new scene: its own BVH trial)
    sc.bvh_key = 0;
    return RT_OK;
}

// The launch interface's view of the resident scene (scene_resident), in the
// precision it is resident in, for flags; n_chunks: the wave BVH unless
// RT_FLAG_NO_BVH (a frame's BVH trial may still run without it).
void scene_view(const Workspace& ws, const rt_scene_desc& d, int flags, rtamd::SceneView& S) {
    const ResidentScene& r = ws.scene;
    const rtamd::CompiledScene& cs = r.sc.cs;
    S.nodes = r.nodes.p;
    S.mats = r.mats.p;
    S.lights = r.lights.p;
    S.dlights = r.dlights.p;
    S.fold = r.fold.p;
    S.n_dlights = d.n_dir_lights;
    S.objs = r.objs.as<rtamd::DevObj>();
    S.ops = r.ops.as<rtamd::DevOp>();
    S.gb = r.gb.as<float>();
    S.ctab = r.ctab.as<float>();
    S.lrec = r.lrec.as<float>();
    S.lwrec = r.lwrec.as<float>();
    S.lgb = r.lgb.as<float>();
    S.n_gb = (int)(cs.gbounds.size() / 4);
    S.wobjs = r.wobjs.as<rtamd::DevObj>();
    S.wctab = r.wctab.as<float>();
    S.worig = r.worig.as<int32_t>();
    S.wchunk = r.wchunk.as<float>();
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

// The resident scene's ray BVH, resident too: uploaded on st by the first
// flagged ray query of the scene, which counts in rt_setup_times[0] like the
// scene's own upload; later ones find it.  Frames and unflagged queries never
// come here.  The caller holds the workspace lock, has reset the staging arena
// and made the scene resident.
int ray_bvh_resident(Workspace& ws, hipStream_t st) {
    ResidentScene& r = ws.scene;
    if (r.rnodes_resident) return RT_OK;
    SceneSetupTime add_time;
    HIP_TRY(upload(r.rnodes, r.sc.cs.rnodes, st, &ws.up));
    r.rnodes_resident = true;
    return RT_OK;
}

// The program of (node, kind) of the resident scene d, resident too: compiled
// (this node's subtree only, so a deep chain's nodes cost their own sizes, not
// the quadratic sum) and uploaded on st by the first query of it, which counts
// in rt_setup_times[0] like the scene's own compile; later queries find it.
// A program deeper than the big stacks is refused here, on the host
// (pick_node_variant), and leaves no entry.  The caller holds the workspace
// lock, has reset the staging arena and made the scene resident.
int node_program_resident(Workspace& ws, const rt_scene_desc& d, int node, int kind, int flags, hipStream_t st,
                          const NodeProg** out) {
    auto& progs = ws.scene.node_progs;
    const auto key = std::make_pair(node, kind);
    auto it = progs.find(key);
    if (it != progs.end()) {
        *out = &it->second;
        return RT_OK;
    }
    SceneSetupTime add_time;
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
    it = progs.emplace(key, std::move(np)).first;
    if (!it->second.host.empty()) {
        const hipError_t e = upload(it->second.ops, it->second.host, st, &ws.up);
        if (e != hipSuccess) {
            it->second.ops.release();
            progs.erase(it);
            rtamd::set_last_error(std::string("node program upload failed: ") + hipGetErrorString(e));
            return RT_ERR_HIP;
        }
    }
    *out = &it->second;
    return RT_OK;
}

// ------------------------------------------------- counters and jitter draws
// The page-locked words k_reduce_counters stores into: at least host_words
// (the previous frame's or query's readback is done)
int ensure_ctr_host(Workspace& ws, size_t host_words) {
    FrameBuffers& fr = ws.frame;
    if (fr.ctr_host && fr.ctr_host_words >= host_words) return RT_OK;
    if (fr.ctr_host) (void)hipHostFree(fr.ctr_host);
    fr.ctr_host = nullptr;
    fr.ctr_host_words = 0;
    rtamd::SetupTimer tm(rtamd::kSetupPinned);
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&fr.ctr_host), host_words * sizeof(unsigned long long),
                          hipHostMallocDefault));
    fr.ctr_host_words = host_words;
    return RT_OK;
}

// The ray / op counter slots, zero on st before a frame's or a radiance
// query's first launch (the last k_reduce_counters may have left them zero)
int counters_ready(Workspace& ws, hipStream_t st) {
    FrameBuffers& fr = ws.frame;
    const size_t ctr_bytes = (size_t)rtamd::kCounterSlots * rtamd::kCounterWords * sizeof(unsigned long long);
    const void* before = fr.counters.p;
    HIP_TRY(fr.counters.ensure(ctr_bytes));
    if (!fr.counters_zero || fr.counters.p != before) HIP_TRY(hipMemsetAsync(fr.counters.p, 0, ctr_bytes, st));
    fr.counters_zero = false;   // (until the reduction has run)
    return RT_OK;
}

// The jitter draws of a standard frame's rows, for the frame (frame_begin) and
// for the frame's rays (camera_rays_impl, jittered) alike, in two steps around
// the caller's ms_rng event.  The caller holds the workspace lock, has reset
// the staging arena, and reports its successful end with jcache.complete.
//
// 1. the plan of (W, H, rows), and the checkpoint table reaching the last loop
//    row's stream words (built on the first use, extended only for a larger frame)
int jitter_plan_ready(Workspace& ws, int W, int H, const int32_t* rows_host, int n_rows, hipStream_t st,
                      rtamd::StdPlan& plan) {
    plan = rtamd::plan_std_frame(W, H, rows_host, n_rows, (int64_t)rtamd::kTableK * 624);
    try {   // (the jump polynomials: file read or GF(2) arithmetic, may throw)
        if (plan.n_ckpt > ws.frame.jtab.n_ck) {   // a build or an extension: synchronous
            const auto t_j = SClock::now();
            HIP_TRY(ws.frame.jtab.ensure(plan.n_ckpt, st));
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
                 rtamd::JitterCache::Entry** ent, bool* filled) {
    FrameBuffers& fr = ws.frame;
    if (filled) *filled = false;
    const rtamd::JitterCache::Got got = fr.jcache.acquire(W, H, sp.rows_jrow, (size_t)n_rows * 16 * W * sizeof(double),
                                                          rtamd::jitter_cache_budget());
    if (!got.e) {
        rtamd::set_last_error(std::string(what) + ": out of device memory for the frame's jitter draws");
        return RT_ERR_HIP;
    }
    *ent = got.e;
    if (got.upload_rows)
        HIP_TRY(rtamd::upload_async(&ws.up, got.e->rows(), sp.rows_jrow.data(), sp.rows_jrow.size() * sizeof(int32_t), st));
    if (got.fill) {
        HIP_TRY(fr.jscratch.ensure(rtamd::mt_fill_scratch_bytes(sp.jranges)));
        fr.jjob.up = &ws.up;
        const auto t_l = SClock::now();
        HIP_TRY(rtamd::mt_launch_fill(fr.jtab, sp.jranges, fr.jjob, fr.jscratch.p, got.e->jit(), st));
        if (filled) *filled = true;
        {
            std::lock_guard<std::mutex> lk(g_setup.mu);
            if (!g_setup.jitter_launched) g_setup.jitter_launch_ms = ms_since(t_l);
            g_setup.jitter_launched = true;
        }
    }
    return RT_OK;
}

}  // namespace rtw

// ------------------------------------------------ rtamd:: and the C ABI
void rtamd::set_workspace_slot(int slot) { rtw::t_ws_slot = slot; }

void rtamd::note_setup_ms(int slot, double ms) {
    if (slot < 4 || slot >= kSetupSlots) return;
    std::lock_guard<std::mutex> lk(rtw::g_setup.mu);
    if (slot < kLastBegin || slot == kLastTrace || slot == kSetupCopyEngine) rtw::g_setup.extra[slot] += ms;
    else rtw::g_setup.extra[slot] = ms;
}

extern "C" int rt_setup_times(double* out, int n) {
    if (!out || n < 0) return RT_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(rtw::g_setup.mu);
    const rtw::SetupTimes& g = rtw::g_setup;
    const double v[4] = {g.scene_ms, g.jtable_ms, g.trace_launch_ms, g.jitter_launch_ms};
    for (int i = 0; i < n && i < rtamd::kSetupSlots; ++i) out[i] = i < 4 ? v[i] : g.extra[i];
    return RT_OK;
}

int rtamd::release_device_workspaces(int min_slot) {
    int prev = 0;
    if (hipGetDevice(&prev) != hipSuccess) return RT_ERR_NO_DEVICE;
    if (min_slot <= 0) rtw::release_staging_frame();
    rtw::each_workspace(min_slot, [](rtw::Workspace& w) {
        (void)hipDeviceSynchronize();
        w.release();
    });
    (void)hipSetDevice(prev);
    return RT_OK;
}
