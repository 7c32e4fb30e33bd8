// rt_test_hooks.hip — the rt_test_* hooks of include/rt_test.h that need
// nothing of a frame's state: the jitter-stream checks, the scene compiler's
// reports, the kernel a frame would launch (pick_variant + the dispatch
// tables), the tables' rows, the launch log the launchers fill
// (rtamd::note_launch), the frame planners of csrc/host/frame_plan.hpp, the
// jitter cache's logic over host memory (csrc/host/jitter_cache.hpp) and its
// counts and budget in the workspaces, and the batched calls' chunk sizes
// (rt_workspace.hpp).  (The distributed-frame hooks live with their transport
// in rt_dist.hip, rt_test_div3 and rt_test_norm3 with the FP64 kernels.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "frame_plan.hpp"
#include "jitter_cache.hpp"
#include "mt_jump.hpp"
#include "mt_poly.hpp"
#include "rt.h"
#include "rt_devbuf.hpp"
#include "rt_internal.hpp"
#include "rt_launch.hpp"
#include "rt_test.h"
#include "rt_workspace.hpp"
#include "scene_compile.hpp"

namespace {
using rtw::DBuf;

using rtamd::KernelNamespace;
using rtamd::KernelVariant;

// The variant pick(compiled scene, desc, &v) chooses for scene s
template <class Pick>
int scene_variant(const rt_scene* s, Pick pick, KernelVariant* v) {
    try {
        const rt_scene_desc& d = *rt_scene_get_desc(s);
        return pick(rtamd::compile_scene(d), d, v);
    } catch (const std::exception& e) {
        rtamd::set_last_error(std::string("scene compile: ") + e.what());
        return RT_ERR_INVALID_ARG;
    }
}
// The variant a frame of (mode, flags) launches: the frame's own pick_variant,
// its BVH trial aside; of a query family: its pick_*_variant (frame_plan.hpp).
auto frame_pick(int mode, int flags) {
    return [=](const rtamd::CompiledScene& cs, const rt_scene_desc& d, KernelVariant* v) {
        return rtamd::pick_variant(cs, d, mode, flags, true, v);
    };
}
auto query_pick(int (*pick)(const rtamd::CompiledScene&, const rt_scene_desc&, int, KernelVariant*), int flags) {
    return [=](const rtamd::CompiledScene& cs, const rt_scene_desc& d, KernelVariant* v) { return pick(cs, d, flags, v); };
}

// out <- "ns::name" of the kernel entry(v) of the variant `pick` chooses for s
// (rt_test_*_kernel_name; `what`: the hook)
template <class Pick, class Entry>
int kernel_name(const char* what, const rt_scene* s, char* out, int cap, Pick pick, Entry entry) {
    if (!s || !out || cap <= 0) return RT_ERR_INVALID_ARG;
    KernelVariant v;
    const int rc = scene_variant(s, pick, &v);
    if (rc != RT_OK) return rc;
    const rtamd::KernelEntry k = entry(v);
    if (!k.name) {
        rtamd::set_last_error(std::string(what) + ": no kernel for this variant");
        return RT_ERR_UNSUPPORTED;
    }
    std::snprintf(out, (size_t)cap, "%s::%s", rtamd::variant_ns_name(v.ns), k.name);
    return RT_OK;
}

// out <- row `index` of namespace ns's `table` as "ns::name" (rt_test_*_kernel_row)
template <class T>
int kernel_row(int ns, T KernelNamespace::*table, int index, char* out, int cap) {
    const KernelNamespace& n = rtamd::kernel_namespace(ns);
    const char* name = out && cap > 0 && index >= 0 && n.*table ? (n.*table)->row_name(index) : nullptr;
    if (!name) return RT_ERR_INVALID_ARG;
    std::snprintf(out, (size_t)cap, "%s::%s", n.name, name);
    return RT_OK;
}
}  // namespace

// ------------------------------------------------------------- launch log
// note_launch is called by every launcher (rt_kernels.hpp, rt_kernel_table.hpp launch_lanes)
// right before its hipLaunchKernelGGL; off, it is one relaxed load.
namespace {
std::atomic<int> g_log_on{0};
std::mutex g_log_mu;
std::string g_log;      // "ns::name\n" per launch
int g_log_n = 0;
}  // namespace

void rtamd::note_launch(const char* ns, const char* name) {
    if (!g_log_on.load(std::memory_order_relaxed)) return;
    std::lock_guard<std::mutex> lk(g_log_mu);
    if (!g_log_on.load(std::memory_order_relaxed)) return;   // (stopped while we waited)
    g_log.append(ns).append("::").append(name).push_back('\n');
    ++g_log_n;
}

extern "C" int rt_test_launch_log(int on) {
    std::lock_guard<std::mutex> lk(g_log_mu);
    if (on) {
        g_log.clear();
        g_log_n = 0;
    }
    g_log_on.store(on ? 1 : 0, std::memory_order_relaxed);
    return RT_OK;
}

extern "C" int rt_test_launch_log_get(char* out, int cap) {
    if (!out || cap <= 0) return RT_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_log_mu);
    if (g_log.size() + 1 > (size_t)cap) {
        rtamd::set_last_error("rt_test_launch_log_get: the log needs " + std::to_string(g_log.size() + 1) + " bytes");
        return RT_ERR_INVALID_ARG;
    }
    std::memcpy(out, g_log.c_str(), g_log.size() + 1);
    return g_log_n;
}

extern "C" int rt_test_kernel_row(int table, int index, char* out, int cap) {
    enum { kRtd = KernelVariant::kRtd, kRtf = KernelVariant::kRtf, kRtdb = KernelVariant::kRtdb };
    switch (table) {
        case 0: return kernel_row(kRtd, &KernelNamespace::std, index, out, cap);
        case 1: return kernel_row(kRtd, &KernelNamespace::paper, index, out, cap);
        case 2: return kernel_row(kRtf, &KernelNamespace::std, index, out, cap);
        case 3: return kernel_row(kRtf, &KernelNamespace::paper, index, out, cap);
        case 4: return kernel_row(kRtdb, &KernelNamespace::std, index, out, cap);
        case 5: return kernel_row(kRtdb, &KernelNamespace::paper, index, out, cap);
        case 6: return kernel_row(kRtd, &KernelNamespace::query, index, out, cap);
        case 7: return kernel_row(kRtdb, &KernelNamespace::query, index, out, cap);
        case 8: {
            // the finish tables rtamd::kernel_namespace hands out (big-stack
            // frames finish with rtd's kernels), rtd's rows first
            int n_rtd = 0;
            while (rtamd::kernel_namespace(kRtd).finish->row_name(n_rtd)) ++n_rtd;
            return index < n_rtd ? kernel_row(kRtd, &KernelNamespace::finish, index, out, cap)
                                 : kernel_row(kRtf, &KernelNamespace::finish, index - n_rtd, out, cap);
        }
        default: return RT_ERR_INVALID_ARG;
    }
}

extern "C" int rt_test_paper_order(int32_t* list, int n, const uint32_t* cost, int n_cost) {
    if (n < 0 || n % 16 || (n && !list) || n_cost < 0 || (n_cost && !cost)) return RT_ERR_INVALID_ARG;
    std::vector<int32_t> L(list, list + n);
    const std::vector<uint32_t> c(cost, cost + n_cost);
    rtamd::order_paper_groups(L, &c);
    std::copy(L.begin(), L.end(), list);
    return RT_OK;
}

extern "C" int rt_test_mt_jump_cpu(int K_blocks, int levels) {
    // Every radix-R tree polynomial x^(624*K*m*R^j) applied to the seed
    // window must equal advancing it m*R^j*K twist blocks sequentially.
    try {
        std::vector<uint32_t> polys = rtamd::mt_tree_polys(K_blocks, levels);
        uint32_t base[624];
        rtamd::mt_first_window(12345u, base);
        int bad = 0;
        for (int j = 0; j < levels; ++j) {
            uint32_t seq[624];
            std::memcpy(seq, base, sizeof(seq));
            const uint64_t step = (uint64_t)K_blocks << (rtamd::kMTRadixBits * j);
            for (int m = 1; m < rtamd::kMTRadix; ++m) {
                rtamd::mt_advance_blocks_cpu(seq, step);
                uint32_t jumped[624];
                rtamd::mt_apply_jump_cpu(polys.data() + ((size_t)j * (rtamd::kMTRadix - 1) + (m - 1)) * 624, base,
                                         jumped);
                // bit 31..0 of words 1..623 and the top bit of word 0 define the state
                bool ok = (jumped[0] & 0x80000000u) == (seq[0] & 0x80000000u);
                for (int k = 1; k < 624; ++k) ok = ok && jumped[k] == seq[k];
                if (!ok) ++bad;
            }
        }
        return bad;
    } catch (...) {
        return -1;
    }
}

extern "C" int rt_test_mt_poly_file(const char* path, int levels) {
    if (!path || levels <= 0) return RT_ERR_INVALID_ARG;
    try {
        std::vector<uint32_t> from_file;
        if (!rtamd::mt_load_tree_polys(path, rtamd::kTableK, levels, from_file)) return 2;
        return from_file == rtamd::mt_tree_polys_computed(rtamd::kTableK, levels) ? 0 : 1;
    } catch (...) {
        return -1;
    }
}

extern "C" int rt_test_jitter_device(int K, int64_t q0, int64_t q1, int64_t first, int64_t count,
                                     double* out_host) {
    if (K < 0 || q0 < 0 || q1 <= q0 || (q0 & 1) || (q1 & 1) || !out_host || first * 2 < q0 || (first + count) * 2 > q1)
        return RT_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return RT_ERR_NO_DEVICE;
    if (K == 0) {   // the frame path: checkpoint table + one-wave fill
        rtamd::JitterTable T;
        HIP_TRY(T.ensure((q1 - 1) / ((int64_t)rtamd::kTableK * 624) + 1, nullptr));
        DBuf dj, ds;
        const std::vector<rtamd::JRange> ranges{rtamd::JRange{q0, q1, 0}};
        rtamd::JitterJob job;
        HIP_TRY(dj.ensure((size_t)(q1 - q0) / 2 * sizeof(double)));
        HIP_TRY(ds.ensure(rtamd::mt_fill_scratch_bytes(ranges)));
        HIP_TRY(rtamd::mt_launch_fill(T, ranges, job, ds.p, dj.as<double>(), nullptr));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(out_host, dj.as<double>() + (first - q0 / 2), (size_t)count * sizeof(double),
                          hipMemcpyDeviceToHost));
        T.release();
        (void)hipFree(dj.p);
        (void)hipFree(ds.p);
        return RT_OK;
    }
    rtamd::JitterPlan plan;
    HIP_TRY(plan.build(K, rtamd::mt_levels_needed(K, q1), nullptr));
    DBuf dc, dj, ds;
    const std::vector<rtamd::JRange> ranges{rtamd::JRange{q0, q1, 0}};
    rtamd::JitterJob job;
    HIP_TRY(dc.ensure(rtamd::mt_ckpt_words(K, q1) * 4));
    HIP_TRY(dj.ensure((size_t)(q1 - q0) / 2 * sizeof(double)));
    HIP_TRY(ds.ensure(rtamd::mt_scratch_bytes(K, ranges)));
    HIP_TRY(rtamd::mt_launch_jitter(plan, ranges, job, ds.p, dc.as<uint32_t>(), dj.as<double>(), nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out_host, dj.as<double>() + (first - q0 / 2), (size_t)count * sizeof(double),
                      hipMemcpyDeviceToHost));
    plan.release();
    (void)hipFree(dc.p);
    (void)hipFree(dj.p);
    (void)hipFree(ds.p);
    return RT_OK;
}

extern "C" int rt_test_kernel_name(const rt_scene* s, int mode, int flags, char* out, int cap) {
    if (mode != RT_MODE_STANDARD && mode != RT_MODE_PAPER) return RT_ERR_INVALID_ARG;
    return kernel_name("rt_test_kernel_name", s, out, cap, frame_pick(mode, flags),
                       [=](const KernelVariant& v) { return rtamd::trace_kernel(v, mode == RT_MODE_PAPER); });
}

extern "C" int rt_test_query_kernel_name(const rt_scene* s, int kind, int flags, char* out, int cap) {
    if (kind != rtamd::kQueryIsect && kind != rtamd::kQueryOccl) return RT_ERR_INVALID_ARG;
    return kernel_name("rt_test_query_kernel_name", s, out, cap, query_pick(rtamd::pick_query_variant, flags),
                       [=](const KernelVariant& v) { return kernel_in(rtamd::kernel_namespace(v.ns).query, v, kind); });
}

// ------------------------------------------------------------------ ray BVH
extern "C" int rt_test_ray_bvh_kernel_name(const rt_scene* s, int kind, int flags, char* out, int cap) {
    if (!s || !out || cap <= 0 || (kind != rtamd::kQueryIsect && kind != rtamd::kQueryOccl)) return RT_ERR_INVALID_ARG;
    try {
        const rt_scene_desc& d = *rt_scene_get_desc(s);
        const rtamd::CompiledScene cs = rtamd::compile_scene(d);
        KernelVariant v;
        const int rc = rtamd::pick_query_variant(cs, d, flags, &v);
        if (rc != RT_OK) return rc;
        const rtamd::KernelEntry k = rtamd::use_ray_bvh(cs, v, flags)
                                         ? kernel_in(&rtd::ray_bvh_table(), v, kind)
                                         : kernel_in(rtamd::kernel_namespace(v.ns).query, v, kind);
        if (!k.name) {
            rtamd::set_last_error("rt_test_ray_bvh_kernel_name: no kernel for this variant");
            return RT_ERR_UNSUPPORTED;
        }
        std::snprintf(out, (size_t)cap, "%s::%s", rtamd::variant_ns_name(v.ns), k.name);
        return RT_OK;
    } catch (const std::exception& e) {
        rtamd::set_last_error(std::string("scene compile: ") + e.what());
        return RT_ERR_INVALID_ARG;
    }
}

extern "C" int rt_test_ray_bvh_row(int index, char* out, int cap) {
    const char* name = out && cap > 0 && index >= 0 ? rtd::ray_bvh_table().row_name(index) : nullptr;
    if (!name) return RT_ERR_INVALID_ARG;
    std::snprintf(out, (size_t)cap, "rtd::%s", name);
    return RT_OK;
}

extern "C" int rt_test_ray_bvh(const rt_scene* s, int32_t* counts, void* nodes_out, int cap) {
    if (!s || !counts || cap < 0 || (cap > 0 && !nodes_out)) return RT_ERR_INVALID_ARG;
    try {
        const rtamd::CompiledScene cs = rtamd::compile_scene(*rt_scene_get_desc(s));
        const int n = (int)cs.rnodes.size();
        counts[0] = n;
        counts[1] = cs.rlead;
        counts[2] = (int32_t)cs.wobjs.size();
        if (n && cap) std::memcpy(nodes_out, cs.rnodes.data(), (size_t)std::min(n, cap) * sizeof(rtamd::RayBvhNode));
        return RT_OK;
    } catch (const std::exception& e) {
        rtamd::set_last_error(std::string("scene compile: ") + e.what());
        return RT_ERR_INVALID_ARG;
    }
}

extern "C" int rt_test_ray_bvh_walk(const rt_scene* s, const rt_ray* rays, size_t n, uint8_t* cand_out,
                                    int32_t* tests_out) {
    if (!s || (n && !rays)) return RT_ERR_INVALID_ARG;
    try {
        const rt_scene_desc& d = *rt_scene_get_desc(s);
        const rtamd::CompiledScene cs = rtamd::compile_scene(d);
        if (cand_out) std::memset(cand_out, 0, n * (size_t)d.n_objects);
        if (!rtamd::ray_bvh_walk(cs, rays, n, d.n_objects, cand_out, tests_out)) {
            rtamd::set_last_error("rt_test_ray_bvh_walk: the scene has no ray BVH");
            return RT_ERR_UNSUPPORTED;
        }
        return RT_OK;
    } catch (const std::exception& e) {
        rtamd::set_last_error(std::string("scene compile: ") + e.what());
        return RT_ERR_INVALID_ARG;
    }
}

extern "C" int rt_test_radiance_kernel_name(const rt_scene* s, int flags, char* out, int cap) {
    return kernel_name("rt_test_radiance_kernel_name", s, out, cap, query_pick(rtamd::pick_radiance_variant, flags),
                       [](const KernelVariant& v) { return kernel_in(rtamd::kernel_namespace(v.ns).radiance, v); });
}

extern "C" int rt_test_shade_kernel_name(const rt_scene* s, int flags, char* out, int cap) {
    return kernel_name("rt_test_shade_kernel_name", s, out, cap, query_pick(rtamd::pick_shade_variant, flags),
                       [](const KernelVariant& v) { return kernel_in(rtamd::kernel_namespace(v.ns).shade, v); });
}

// (table 0: rtd's, 1: rtdb's)
extern "C" int rt_test_radiance_kernel_row(int table, int index, char* out, int cap) {
    if (table != 0 && table != 1) return RT_ERR_INVALID_ARG;
    return kernel_row(table ? KernelVariant::kRtdb : KernelVariant::kRtd, &KernelNamespace::radiance, index, out, cap);
}

extern "C" int rt_test_shade_kernel_row(int table, int index, char* out, int cap) {
    if (table != 0 && table != 1) return RT_ERR_INVALID_ARG;
    return kernel_row(table ? KernelVariant::kRtdb : KernelVariant::kRtd, &KernelNamespace::shade, index, out, cap);
}

extern "C" int rt_test_node_kernel_row(int table, int index, char* out, int cap) {
    if (table != 0 && table != 1) return RT_ERR_INVALID_ARG;
    return kernel_row(table ? KernelVariant::kRtdb : KernelVariant::kRtd, &KernelNamespace::node, index, out, cap);
}

extern "C" int rt_test_node_program(const rt_scene* s, int node, int kind, int32_t* ops_out, int cap,
                                    int32_t* depths_out2) {
    if (!s || cap < 0 || (cap > 0 && !ops_out)) return RT_ERR_INVALID_ARG;
    try {
        const rtamd::NodeProgram p = rtamd::compile_node_program(*rt_scene_get_desc(s), node, kind);
        for (int i = 0; i < cap && i < (int)p.ops.size(); ++i) {
            const rtamd::DevOp& o = p.ops[i];
            const int32_t v[4] = {o.op, o.node, o.top, o.csg_op};
            std::copy(v, v + 4, ops_out + 4 * (size_t)i);
        }
        if (depths_out2) {
            depths_out2[0] = p.max_ray_depth;
            depths_out2[1] = p.max_ivl_depth;
        }
        return (int)p.ops.size();
    } catch (const std::exception& e) {
        rtamd::set_last_error(std::string("node compile: ") + e.what());
        return RT_ERR_INVALID_ARG;
    }
}

extern "C" int rt_test_node_kernel_name(const rt_scene* s, int node, int kind, int flags, char* out, int cap) {
    if (!s || !out || cap <= 0 || (kind != rtamd::kNodeIsect && kind != rtamd::kNodeIvl)) return RT_ERR_INVALID_ARG;
    KernelVariant v;
    try {
        const rt_scene_desc& d = *rt_scene_get_desc(s);
        const int rc = rtamd::pick_node_variant(d, node, rtamd::compile_node_program(d, node, kind), flags, &v);
        if (rc != RT_OK) return rc;
    } catch (const std::exception& e) {
        rtamd::set_last_error(std::string("node compile: ") + e.what());
        return RT_ERR_INVALID_ARG;
    }
    const rtamd::KernelEntry k = kernel_in(rtamd::kernel_namespace(v.ns).node, v, kind);
    if (!k.name) {
        rtamd::set_last_error("rt_test_node_kernel_name: no kernel for this variant");
        return RT_ERR_UNSUPPORTED;
    }
    std::snprintf(out, (size_t)cap, "%s::%s", rtamd::variant_ns_name(v.ns), k.name);
    return RT_OK;
}

extern "C" int rt_test_kernel_info(const rt_scene* s, int mode, int flags, int32_t* out) {
    if (!s || !out) return RT_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return RT_ERR_NO_DEVICE;
    rtamd::KernelVariant v;
    // (the non-counting, untimed variant, whatever the flags say)
    if (mode != RT_MODE_STANDARD && mode != RT_MODE_PAPER) return RT_ERR_INVALID_ARG;
    const int rc = scene_variant(s, frame_pick(mode, flags & ~RT_FLAG_COUNT_OPS), &v);
    if (rc != RT_OK) return rc;
    const bool paper = mode == RT_MODE_PAPER;
    const void* fn = rtamd::trace_kernel(v, paper).fn;
    if (!fn) { rtamd::set_last_error("rt_test_kernel_info: no kernel for this variant"); return RT_ERR_UNSUPPORTED; }
    hipFuncAttributes a{};
    HIP_TRY(hipFuncGetAttributes(&a, fn));
    int blocks = 0;
    const int threads = rtamd::trace_block_threads(v, paper);
    const size_t pool = rtamd::trace_pool_bytes(v, paper);
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, fn, threads, pool));
    out[0] = a.numRegs;                      // VGPRs per lane
    out[1] = (int32_t)a.localSizeBytes;      // scratch (spill) bytes per lane
    out[2] = (int32_t)(a.sharedSizeBytes + pool);   // LDS per workgroup (static + the shading pool)
    out[3] = blocks;                                 // resident workgroups per CU
    out[4] = blocks * (threads / 64) / 4;            // waves per SIMD (4 SIMDs per CU)
    out[5] = a.maxThreadsPerBlock;
    out[6] = v.wv > 0 ? 1 : 0;
    out[7] = v.secondary ? 1 : 0;
    return RT_OK;
}

extern "C" int rt_test_wave_bvh(const rt_scene* s, int32_t* counts, int32_t* worig, float* wctab, int cap_objs,
                                float* wchunk, int cap_chunks) {
    if (!s || !counts || cap_objs < 0 || cap_chunks < 0) return RT_ERR_INVALID_ARG;
    try {
        const rtamd::CompiledScene cs = rtamd::compile_scene(*rt_scene_get_desc(s));
        const int n = (int)cs.wobjs.size(), nch = (int)(cs.wchunk.size() / 8);
        counts[0] = n;
        counts[1] = nch;
        for (int i = 0; i < std::min(n, cap_objs); ++i) {
            if (worig) worig[i] = cs.worig[i];
            if (wctab) std::memcpy(wctab + 8 * (size_t)i, &cs.wctab[8 * (size_t)i], 8 * sizeof(float));
        }
        if (wchunk) std::memcpy(wchunk, cs.wchunk.data(), (size_t)std::min(nch, cap_chunks) * 8 * sizeof(float));
        return RT_OK;
    } catch (const std::exception& e) {
        rtamd::set_last_error(std::string("scene compile: ") + e.what());
        return RT_ERR_INVALID_ARG;
    }
}

extern "C" int rt_test_compile_info(const rt_scene* s, int32_t* out) {
    if (!s || !out) return RT_ERR_INVALID_ARG;
    try {
        const rtamd::CompiledScene cs = rtamd::compile_scene(*rt_scene_get_desc(s));
        int groups = 0, members = 0, ivl_groups = 0, ivl_members = 0;
        for (const auto& o : cs.objs)
            if (o.kind == rtamd::OBJ_GROUP) { ++groups; members += o.m; }
        for (const auto& op : cs.ops)
            if (op.op == rtamd::OP_IVL_GROUP) { ++ivl_groups; ivl_members += op.top / 2; }
        out[0] = (int32_t)cs.objs.size();
        out[1] = groups;
        out[2] = members;
        out[3] = (int32_t)cs.ops.size();
        out[4] = ivl_groups;
        out[5] = ivl_members;
        out[6] = cs.has_eager ? 1 : 0;
        out[7] = cs.max_ivl_depth;
        return RT_OK;
    } catch (const std::exception& e) {
        rtamd::set_last_error(std::string("scene compile: ") + e.what());
        return RT_ERR_INVALID_ARG;
    }
}

extern "C" int rt_test_compile_forms(const rt_scene* s, int32_t* out, int cap) {
    if (!s || !out || cap < RT_TEST_FORMS_LEN) return RT_ERR_INVALID_ARG;
    try {
        const rtamd::CompiledScene cs = rtamd::compile_scene(*rt_scene_get_desc(s));
        std::fill(out, out + RT_TEST_FORMS_LEN, 0);
        auto bin3 = [](int v) { return v < 0 ? 0 : v > 2 ? 2 : v; };
        for (const auto& o : cs.objs) {
            if (o.kind >= 0 && o.kind <= rtamd::OBJ_GROUP) ++out[RT_TEST_FORMS_OBJ + o.kind];
            if (o.kind != rtamd::OBJ_GROUP && o.has_bound) ++out[RT_TEST_FORMS_BOUNDED];
            if (o.kind != rtamd::OBJ_CHAIN) continue;
            if (o.npb > 0) ++out[RT_TEST_FORMS_PREFILTER];
            ++out[RT_TEST_FORMS_CHAIN_CORE + (o.core ? 1 : 0)];
            ++out[RT_TEST_FORMS_CHAIN_M + std::min(o.m, 3)];
            if (o.m >= 3) ++out[RT_TEST_FORMS_CHAIN_M3_CORE + (o.core ? 1 : 0)];
            if (o.nfold > 0) ++out[RT_TEST_FORMS_FOLD + bin3(o.fold_op)];
        }
        for (const auto& op : cs.ops) {
            if (op.op >= 0 && op.op <= rtamd::OP_IVL_GROUP) ++out[RT_TEST_FORMS_OP + op.op];
            if (op.op == rtamd::OP_NEVER) ++out[RT_TEST_FORMS_NEVER_TOP + bin3(op.top)];
            if (op.op == rtamd::OP_IVL_GROUP) ++out[RT_TEST_FORMS_IVL_GROUP + bin3(op.csg_op)];
        }
        out[RT_TEST_FORMS_RAY_DEPTH] = cs.max_ray_depth;
        out[RT_TEST_FORMS_IVL_DEPTH] = cs.max_ivl_depth;
        return RT_OK;
    } catch (const std::exception& e) {
        rtamd::set_last_error(std::string("scene compile: ") + e.what());
        return RT_ERR_INVALID_ARG;
    }
}

// ------------------------------------------------------ frame planners (CPU)
extern "C" int rt_test_plan_dist(int H, int world, int rank, int mode, int kind, int chunks, int32_t* counts,
                                 int32_t* rows_out, int32_t* bounds_out, int32_t* rowtab_out, int cap_table) {
    if (H <= 0 || world <= 0 || rank < 0 || rank >= world || chunks < 1 || chunks > rtamd::kChunks || !counts ||
        !rows_out || !bounds_out)
        return RT_ERR_INVALID_ARG;
    const rtamd::DistPlan p =
        rtamd::plan_dist_frame(H, world, rank, mode, kind ? 0 : rtamd::root_shed(mode), chunks, rowtab_out != nullptr);
    if (rowtab_out && (size_t)cap_table < p.rowtab.size()) return RT_ERR_INVALID_ARG;
    counts[0] = (int32_t)p.rows.size();
    counts[1] = p.m;
    counts[2] = (int32_t)p.bounds.size();
    std::copy(p.rows.begin(), p.rows.end(), rows_out);
    for (size_t k = 0; k < p.bounds.size(); ++k) {
        bounds_out[2 * k] = p.bounds[k].first;
        bounds_out[2 * k + 1] = p.bounds[k].second;
    }
    if (rowtab_out) std::copy(p.rowtab.begin(), p.rowtab.end(), rowtab_out);
    return RT_OK;
}

// ------------------------------------------------------ jitter cache (CPU)
extern "C" int rt_test_jitter_cache_sim(const int64_t* ops, int n_ops, int64_t budget, int64_t* out) {
    if (n_ops < 0 || (n_ops && (!ops || !out)) || budget < 0) return RT_ERR_INVALID_ARG;
    for (int k = 0; k < n_ops; ++k) {
        const int64_t* o = ops + 5 * (size_t)k;
        if (o[0] < 0 || o[0] > 5) return RT_ERR_INVALID_ARG;
        if (o[0] <= 1 && (o[1] <= 0 || o[1] > 4096 || o[2] < 0 || o[3] <= 0 || o[3] > 4096 || o[2] + o[3] > (1 << 20) ||
                          o[4] < 0 || o[4] > (1 << 20)))
            return RT_ERR_INVALID_ARG;
        if (o[0] >= 3 && o[0] <= 4 && o[4] < 0) return RT_ERR_INVALID_ARG;
    }
    return rtamd::jitter_cache_sim(ops, n_ops, budget, out);
}

namespace {
bool rows_ok(int H, const int32_t* rows, int n_rows) {
    return H > 0 && n_rows > 0 && n_rows <= H && rows && rtw::check_rows(nullptr, H, rows, n_rows) == RT_OK;
}
}  // namespace

extern "C" int rt_test_plan_std(int W, int H, const int32_t* rows, int n_rows, int32_t* jrow_out, int64_t* ranges_out,
                                int64_t* out3) {
    if (W <= 0 || !rows_ok(H, rows, n_rows) || !jrow_out || !ranges_out || !out3) return RT_ERR_INVALID_ARG;
    const rtamd::StdPlan p = rtamd::plan_std_frame(W, H, rows, n_rows, (int64_t)rtamd::kTableK * 624);
    std::copy(p.rows_jrow.begin() + n_rows, p.rows_jrow.end(), jrow_out);
    for (size_t i = 0; i < p.jranges.size(); ++i) {
        ranges_out[3 * i] = p.jranges[i].qa;
        ranges_out[3 * i + 1] = p.jranges[i].qb;
        ranges_out[3 * i + 2] = p.jranges[i].dst;
    }
    out3[0] = (int64_t)p.jranges.size();
    out3[1] = p.q_end;
    out3[2] = p.n_ckpt;
    return RT_OK;
}

extern "C" int rt_test_plan_paper(int W, int H, const int32_t* rows, int n_rows, int32_t* ext_out,
                                  int32_t* ext_shade_out, int32_t* ext_pos_out, int32_t* nbr_out, int64_t* out6) {
    if (W <= 0 || !rows_ok(H, rows, n_rows) || !ext_out || !ext_shade_out || !ext_pos_out || !nbr_out || !out6)
        return RT_ERR_INVALID_ARG;
    const rtamd::PaperPlan p = rtamd::plan_paper_frame(0, W, H, RT_MODE_PAPER, 0, rows, n_rows);
    std::copy_n(p.aux.begin() + p.off_ext_rows(), p.n_ext, ext_out);
    std::copy_n(p.aux.begin() + p.off_ext_shade(), p.n_ext, ext_shade_out);
    std::copy(p.ext_pos.begin(), p.ext_pos.end(), ext_pos_out);
    std::copy_n(p.aux.begin() + p.off_nbr(), 3 * (size_t)n_rows, nbr_out);
    out6[0] = p.n_ext;
    out6[1] = (int64_t)p.logical_isect;
    out6[2] = (int64_t)p.aux_ints();
    out6[3] = (int64_t)p.list_cap();
    out6[4] = (int64_t)p.gtime_words();
    out6[5] = rtamd::paper_waves_per_group(W);
    return RT_OK;
}

extern "C" int rt_test_plan_paper_calls(int W, int H, const int32_t* rows, int n_rows, const int32_t* calls,
                                        int n_calls, int rollback_after, int32_t* call_out, int32_t* lists_out,
                                        int cap_lists, int32_t* ext_done_out) {
    if (W <= 0 || !rows_ok(H, rows, n_rows) || n_calls < 0 || n_calls > 30 || (n_calls && !calls) || !call_out ||
        !lists_out || cap_lists < 0 || !ext_done_out)
        return RT_ERR_INVALID_ARG;
    for (int k = 0; k < n_calls; ++k)
        if (calls[3 * k] < 0 || calls[3 * k + 1] < calls[3 * k] || calls[3 * k + 1] > n_rows) return RT_ERR_INVALID_ARG;
    const rtamd::PaperPlan p = rtamd::plan_paper_frame(0, W, H, RT_MODE_PAPER, 0, rows, n_rows);
    rtamd::PaperCalls pc;
    pc.reset(&p);
    int used = 0;
    for (int k = 0; k < n_calls; ++k) {
        const rtamd::PaperCalls::Call c = pc.next_call(calls[3 * k], calls[3 * k + 1], (uintptr_t)calls[3 * k + 2]);
        const int len = c.ok ? (int)c.list->size() : 0;
        if (used + len > cap_lists) return RT_ERR_INVALID_ARG;
        if (len) std::copy(c.list->begin(), c.list->end(), lists_out + used);
        used += len;
        int32_t mask = 0;
        for (int w : c.wait) mask |= 1 << w;
        call_out[4 * k] = c.ok ? 1 : 0;
        call_out[4 * k + 1] = c.list_off;
        call_out[4 * k + 2] = len;
        call_out[4 * k + 3] = mask;
        if (c.ok && k == rollback_after) pc.rollback();
    }
    std::copy(pc.ext_done().begin(), pc.ext_done().end(), ext_done_out);
    return RT_OK;
}

// ------------------------------------------- workspaces (rt_workspace.hpp)
// The jitter cache of workspace (current device, slot).  Takes the workspace
// lock: not for a thread that holds an open frame of that workspace.
extern "C" int rt_test_jitter_cache_stats_slot(int slot, uint64_t* hits, uint64_t* misses, uint64_t* entries,
                                               uint64_t* bytes) {
    if (!hits || !misses || !entries || !bytes) return RT_ERR_INVALID_ARG;
    *hits = *misses = *entries = *bytes = 0;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    rtw::Workspace* w = rtw::find_workspace(dev, slot);
    if (!w) return RT_OK;   // (no frame of that slot yet)
    std::lock_guard<std::mutex> wl(w->mu);
    const rtamd::JitterCache& jc = w->frame.jcache;
    *hits = jc.hits();
    *misses = jc.misses();
    *entries = jc.entries();
    *bytes = jc.bytes();
    return RT_OK;
}

extern "C" int rt_test_jitter_cache_stats(uint64_t* hits, uint64_t* misses, uint64_t* entries, uint64_t* bytes) {
    return rt_test_jitter_cache_stats_slot(rtw::workspace_slot(), hits, misses, entries, bytes);
}

extern "C" int rt_test_jitter_cache_budget(int64_t bytes) {
    int prev = 0;
    HIP_TRY(hipGetDevice(&prev));
    rtamd::set_jitter_cache_budget(bytes);
    rtw::each_workspace(INT32_MIN, [](rtw::Workspace& w) {
        w.frame.jcache.clear();
        w.frame.jcache.reset_counts();
    });
    (void)hipSetDevice(prev);
    return RT_OK;
}

extern "C" int rt_test_camera_chunk_rays(size_t n) {
    rtw::g_chunk_items.store(n ? n : rtw::kChunkItems);
    return RT_OK;
}

extern "C" int rt_test_scatter_launch_items(size_t n) {
    rtw::g_scatter_items.store(n ? std::min(n, rtw::kLaunchItems) : rtw::kLaunchItems);
    return RT_OK;
}
