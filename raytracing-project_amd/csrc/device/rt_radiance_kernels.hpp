// rt_radiance_kernels.hpp — the batched radiance-query kernel, built right
// after rt_device.hpp in translation units of its own (rt_radiance_f64.hip:
// RT_NS = rtd; rt_radiance_big.hip: RT_NS = rtdb, the big-stack build), so
// that the frame kernels of rt_kernels.hpp and the ray-query kernels of
// rt_query_kernels.hpp compile exactly as they did without it.  There is no
// FP32 build.
//
//   k_radiance: Tracer::trace (tracer.cpp:12-73) for a batch of rays: the
//   closest hit, Phong shading with a shadow ray to every light, and the
//   reflection / refraction recursion: trace<E, D, SEC, DL = D, WV = 0> of
//   rt_device.hpp, the frames' own Tracer::trace_recursive.
//
// One ray per lane, one-wave workgroups (the query kernels' shape).  A wave's
// rays are whatever the caller put next to each other, so the trace runs with
// per-lane culls (WV = 0: an object is skipped only when no lane's own ray can
// touch its bound), which stay exact for incoherent rays; the wave-level culls
// and the wave BVH bound a pixel tile's rays and are not used here.  tmin and
// tmax of an rt_ray are not read: Tracer::trace queries [1e-4, inf).
//
// The query kernels' rules hold: lanes past the batch's end take the last ray
// again, so that the wave-wide tests of the first closest hit see a full wave;
// their stores are masked, and so are their ray counts.  Every store comes
// after the last scene read.  Dynamic LDS: pool_bytes(64), shade()'s light
// cache (wave_pool).

#include "rt_kernel_table.hpp"

namespace RT_NS {

using rtamd::kCounterSlots;
using rtamd::kCounterWords;
using rtamd::RadianceParams;
using rtamd::SceneView;

namespace {

constexpr size_t kRadiancePool = pool_bytes(kQueryThreads);

// The wave's Scene::intersect / Scene::occluded call counts: reduced by
// shuffles, then one 64-bit atomic per counter into the frames' hashed slots
// (rt_kernels.hpp flush_counters, for one-wave workgroups without op
// counters; the host sums the slots as it does for a frame).
__device__ __forceinline__ void flush_ray_counts(unsigned long long* ctr, uint32_t ni, uint32_t no) {
    unsigned long long vi = ni, vo = no;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        vi += __shfl_xor(vi, off);
        vo += __shfl_xor(vo, off);
    }
    if (threadIdx.x == 0) {
        unsigned long long* slot = ctr + (size_t)(blockIdx.x % kCounterSlots) * kCounterWords;
        if (vi) atomicAdd(slot, vi);
        if (vo) atomicAdd(slot + 1, vo);
    }
}

template <bool E, bool D, bool SEC, bool PL>
__global__ __launch_bounds__(kQueryThreads) void k_radiance(DevScene S, RadianceParams P) {
    const size_t i0 = (size_t)blockIdx.x * kQueryThreads + threadIdx.x;
    const bool active = i0 < P.n;
    const size_t i = active ? i0 : P.n - 1;
    std::conditional_t<PL, CntPlain, Cnt<false>> cnt;
    cnt.init();
    // ray i of the batch as Ray(o, d) (core.h:278)
    const rt_ray R = P.rays[i];
    const DRay r = make_ray(v3((real)R.o[0], (real)R.o[1], (real)R.o[2]), v3((real)R.d[0], (real)R.d[1], (real)R.d[2]));
    uint32_t ni = 0, no = 0;
    const V3 c = trace<E, D, SEC, /*DL=*/D, /*WV=*/0>(S, r, ni, no, cnt);
    if (active) {
        double* o = P.rgb + 3 * i;
        o[0] = (double)c.x;
        o[1] = (double)c.y;
        o[2] = (double)c.z;
    }
    // (a tail lane's replay of the last ray is not the caller's ray: not counted)
    flush_ray_counts(P.counters, active ? ni : 0u, active ? no : 0u);
}

// The radiance kernels by variant, in the tables' one form
// (rt_kernel_table.hpp).  Columns: E D SEC PL.  The general row traces every
// scene (with no reflecting or refracting material, or recursion < 2, its loop
// never descends), so eager scenes have no SEC = false row (frame_plan.hpp
// pick_radiance_variant never asks for one); RT_GENERAL_ONLY (the big-stack
// build) keeps that row alone.
constexpr unsigned rkey(bool e, bool d, bool sec, bool pl) {
    return (unsigned)e | (unsigned)d << 1 | (unsigned)sec << 2 | (unsigned)pl << 3;
}
#define RT_RAD(e, d, sec, pl, ...) RT_KERNEL_ROW(rkey(e, d, sec, pl), __VA_ARGS__)
const KernelRow<DevScene, RadianceParams> kRadianceKernels[] = {
    RT_RAD(1, 1, 1, 0, k_radiance<true, true, true, false>),
#ifndef RT_GENERAL_ONLY
    RT_RAD(0, 1, 1, 0, k_radiance<false, true, true, false>),
    RT_RAD(0, 1, 0, 0, k_radiance<false, true, false, false>),
    RT_RAD(0, 0, 1, 0, k_radiance<false, false, true, false>),
    RT_RAD(0, 0, 0, 0, k_radiance<false, false, false, false>),
    RT_RAD(0, 0, 1, 1, k_radiance<false, false, true, true>),
    RT_RAD(0, 0, 0, 1, k_radiance<false, false, false, true>),
#endif
};
#undef RT_RAD

const KernelRow<DevScene, RadianceParams>* radiance_row(const rtamd::KernelVariant& v) {
    return find_kernel(kRadianceKernels, rkey(v.eager, v.deep, v.secondary, v.plain));
}

hipError_t launch_radiance(const rtamd::KernelVariant& v, int, dim3, hipStream_t st, const SceneView& V,
                           const RadianceParams& P) {
    return launch_lanes(radiance_row(v), kRadiancePool, false, st, V, P);
}
rtamd::KernelEntry radiance_kernel(const rtamd::KernelVariant& v, int) { return kernel_entry(radiance_row(v)); }
const char* radiance_row_name(int i) { return row_name(kRadianceKernels, i); }

}  // namespace

const rtamd::KernelTable<RadianceParams>& radiance_table() {
    static const rtamd::KernelTable<RadianceParams> t = {launch_radiance, radiance_kernel, radiance_row_name,
                                                         kQueryThreads, kRadiancePool};
    return t;
}

}  // namespace RT_NS
