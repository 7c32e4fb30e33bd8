// rt_query_kernels.hpp — the batched ray-query kernels, built right after
// rt_device.hpp in translation units of their own (rt_query_f64.hip: RT_NS =
// rtd; rt_query_big.hip: RT_NS = rtdb, the big-stack build), so that the frame
// kernels of rt_kernels.hpp compile exactly as they did without them.  There
// is no FP32 build.
//
//   k_query_isect: Scene::intersect (scene.cpp:10-24) for a batch of rays
//   k_query_occl:  Scene::occluded  (scene.cpp:33-42)
//
// One ray per lane, one-wave workgroups (the frame kernels' shape,
// rt_kernels.hpp RT_STD_WPB).  A wave's rays are whatever the caller put next
// to each other: scene_intersect / scene_occluded skip an object only when no
// lane's own ray can touch its bound (__any over per-lane tests), which stays
// exact for incoherent rays and merely culls less.  The wave-level culls and
// the wave BVH (scene_intersect_wave ...) bound a pixel tile's rays and are
// not used here; scenes of more than 256 objects walk the flat object list,
// whose results are the BVH's (RT_FLAG_NO_BVH).
//
// Those queries run wave-wide tests between per-lane work, so every lane of a
// wave walks the object loop: lanes past the batch's end take the last ray
// again and only their stores are masked.  Every store comes after the last
// scene read (see paper_primary_body, rt_kernels.hpp: a store ahead of a scene
// load turns the scene's wave-uniform reads into vector loads).  No LDS (only
// shade and the counter flush use the pool) and no counters: a batch of n rays
// is n queries.

#include "rt_kernel_table.hpp"

namespace RT_NS {

using rtamd::QueryParams;
using rtamd::SceneView;

namespace {

// ray i of the batch (lanes past its end: the last ray), as Ray(o, d) (core.h:278)
__device__ __forceinline__ DRay query_ray(const QueryParams& P, size_t i, real& tmin, real& tmax) {
    const rt_ray R = P.rays[i];
    tmin = (real)R.tmin;
    tmax = (real)R.tmax;
    return make_ray(v3((real)R.o[0], (real)R.o[1], (real)R.o[2]), v3((real)R.d[0], (real)R.d[1], (real)R.d[2]));
}

template <bool E, bool D, bool PL>
__global__ __launch_bounds__(kQueryThreads) void k_query_isect(DevScene S, QueryParams P) {
    const size_t i0 = (size_t)blockIdx.x * kQueryThreads + threadIdx.x;
    const bool active = i0 < P.n;
    const size_t i = active ? i0 : P.n - 1;
    std::conditional_t<PL, CntPlain, Cnt<false>> cnt;
    cnt.init();
    real tmin, tmax;
    const DRay r = query_ray(P, i, tmin, tmax);
    real ht = RV(0.0);
    DHit h;
    h.mat = -1;
    h.p = h.n = v3(RV(0.0), RV(0.0), RV(0.0));
    h.ff = 0;
    const bool hit = scene_intersect<E, D>(S, r, tmin, tmax, ht, h, cnt);
    if (active) {
        rt_hit o;   // (a miss: mat -1, every other field 0)
        o.t = hit ? (double)ht : 0.0;
        o.p[0] = hit ? (double)h.p.x : 0.0;
        o.p[1] = hit ? (double)h.p.y : 0.0;
        o.p[2] = hit ? (double)h.p.z : 0.0;
        o.n[0] = hit ? (double)h.n.x : 0.0;
        o.n[1] = hit ? (double)h.n.y : 0.0;
        o.n[2] = hit ? (double)h.n.z : 0.0;
        o.mat = hit ? h.mat : -1;
        o.front_face = hit ? h.ff : 0;
        P.hits[i] = o;
        if (P.mask) P.mask[i] = hit ? 1 : 0;
    }
}

template <bool E, bool D, bool PL>
__global__ __launch_bounds__(kQueryThreads) void k_query_occl(DevScene S, QueryParams P) {
    const size_t i0 = (size_t)blockIdx.x * kQueryThreads + threadIdx.x;
    const bool active = i0 < P.n;
    const size_t i = active ? i0 : P.n - 1;
    std::conditional_t<PL, CntPlain, Cnt<false>> cnt;
    cnt.init();
    real tmin, tmax;
    const DRay r = query_ray(P, i, tmin, tmax);
    const bool occ = scene_occluded<E, D>(S, r, tmin, tmax, cnt);
    if (active) P.mask[i] = occ ? 1 : 0;
}

// The query kernels by variant, in the tables' one form (rt_kernel_table.hpp).
// Columns: kind (rtamd::kQueryIsect / kQueryOccl) E D PL.  RT_GENERAL_ONLY (the
// big-stack build) keeps the general rows.
constexpr unsigned qkey(int kind, bool e, bool d, bool pl) {
    return (unsigned)kind | (unsigned)e << 1 | (unsigned)d << 2 | (unsigned)pl << 3;
}
#define RT_QRY(kind, e, d, pl, ...) RT_KERNEL_ROW(qkey(kind, e, d, pl), __VA_ARGS__)
const KernelRow<DevScene, QueryParams> kQueryKernels[] = {
    RT_QRY(0, 1, 1, 0, k_query_isect<true, true, false>),
    RT_QRY(1, 1, 1, 0, k_query_occl<true, true, false>),
#ifndef RT_GENERAL_ONLY
    RT_QRY(0, 0, 1, 0, k_query_isect<false, true, false>),
    RT_QRY(1, 0, 1, 0, k_query_occl<false, true, false>),
    RT_QRY(0, 0, 0, 0, k_query_isect<false, false, false>),
    RT_QRY(1, 0, 0, 0, k_query_occl<false, false, false>),
    RT_QRY(0, 0, 0, 1, k_query_isect<false, false, true>),
    RT_QRY(1, 0, 0, 1, k_query_occl<false, false, true>),
#endif
};
#undef RT_QRY

const KernelRow<DevScene, QueryParams>* query_row(const rtamd::KernelVariant& v, int kind) {
    if (kind != rtamd::kQueryIsect && kind != rtamd::kQueryOccl) return nullptr;
    return find_kernel(kQueryKernels, qkey(kind, v.eager, v.deep, v.plain));
}

hipError_t launch_query(const rtamd::KernelVariant& v, int kind, dim3, hipStream_t st, const SceneView& V,
                        const QueryParams& P) {
    return launch_lanes(query_row(v, kind), 0, false, st, V, P);
}
rtamd::KernelEntry query_kernel(const rtamd::KernelVariant& v, int kind) { return kernel_entry(query_row(v, kind)); }
const char* query_row_name(int i) { return row_name(kQueryKernels, i); }

}  // namespace

const rtamd::KernelTable<QueryParams>& query_table() {
    static const rtamd::KernelTable<QueryParams> t = {launch_query, query_kernel, query_row_name, kQueryThreads, 0};
    return t;
}

}  // namespace RT_NS
