// rt_shade_kernels.hpp — the batched shading-query kernel, built right after
// rt_device.hpp in translation units of its own (rt_shade_f64.hip: RT_NS =
// rtd; rt_shade_big.hip: RT_NS = rtdb, the big-stack build), so that the
// frame kernels of rt_kernels.hpp and the query kernels of
// rt_query_kernels.hpp / rt_radiance_kernels.hpp compile exactly as they did
// without it.  There is no FP32 build.
//
//   k_shade: shade_lambert_phong(scene, hit, wo) (shading.cpp:31-138) for a
//   batch of caller-given hits: shade<E, D, DL = D, WV = 0> of rt_device.hpp,
//   the function every frame and radiance kernel calls after its closest hit.
//
// One hit per lane, one-wave workgroups (the query kernels' shape).  A wave's
// hits are whatever the caller put next to each other, so the shadow queries
// run with per-lane culls (WV = 0: scene_occluded, which reads nothing indexed
// by a light's number); the wave-level shadow hull and the light-relative cull
// records (DevScene::lrec / lgb) belong to the WV kernels and are not reached:
// the launcher hands the kernel null pointers for them, because the call's
// point lights (DevScene::lights / n_lights) may not be the scene's.
//
// Lanes with nothing to shade - past the batch's end, masked out
// (ShadeParams::mask), or with a material index outside [0, n_materials) -
// ride along with valid = false: they hold a zero hit, make no occlusion
// query and count nothing.  A wave without a valid lane never calls shade():
// it touches no material and no light.  Every store comes after the last
// scene read; the stores of lanes past the end are masked.  Dynamic LDS:
// pool_bytes(64), shade()'s light cache (wave_pool).

#include "rt_kernel_table.hpp"

namespace RT_NS {

using rtamd::kCounterSlots;
using rtamd::kCounterWords;
using rtamd::SceneView;
using rtamd::ShadeParams;

namespace {

constexpr size_t kShadePool = pool_bytes(kQueryThreads);

// The wave's Scene::occluded call count: reduced by shuffles, then one 64-bit
// atomic into word 1 of the frames' hashed counter slots (as the radiance
// kernel's flush_ray_counts; the host sums the slots as it does for a frame).
__device__ __forceinline__ void flush_occl_count(unsigned long long* ctr, uint32_t no) {
    unsigned long long vo = no;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) vo += __shfl_xor(vo, off);
    if (threadIdx.x == 0 && vo) atomicAdd(ctr + (size_t)(blockIdx.x % kCounterSlots) * kCounterWords + 1, vo);
}

template <bool E, bool D, bool PL>
__global__ __launch_bounds__(kQueryThreads) void k_shade(DevScene S, ShadeParams P) {
    const size_t i = (size_t)blockIdx.x * kQueryThreads + threadIdx.x;
    const bool active = i < P.n;
    std::conditional_t<PL, CntPlain, Cnt<false>> cnt;
    cnt.init();
    // entry i of the batch as Hit{t, p, n, mat} and wo; a masked-out entry is
    // not read, a material index outside the table is a null material
    // (S.bg_mat = n_materials)
    bool valid = active && (!P.mask || P.mask[i] != 0);
    bool null_mat = false;
    real ht = RV(0.0);
    DHit h;
    h.p = h.n = v3(RV(0.0), RV(0.0), RV(0.0));
    h.mat = -1;
    h.ff = 1;
    V3 wo = v3(RV(0.0), RV(0.0), RV(0.0));
    if (valid) {
        const rt_hit* H = P.hits + i;
        const int mat = H->mat;
        if (mat >= 0 && mat < S.bg_mat) {
            ht = (real)H->t;
            h.p = v3((real)H->p[0], (real)H->p[1], (real)H->p[2]);
            h.n = v3((real)H->n[0], (real)H->n[1], (real)H->n[2]);
            h.mat = mat;
            const double* w = P.wo + 3 * i;
            wo = v3((real)w[0], (real)w[1], (real)w[2]);
        } else {
            null_mat = true;
            valid = false;
        }
    }
    uint32_t no = 0;
    V3 c = v3(RV(0.0), RV(0.0), RV(0.0));
    // (wave-uniform: every lane of a wave with a valid one calls shade())
    if (__any(valid)) c = shade<E, D, /*DL=*/D, /*WV=*/0>(S, ht, h, wo, no, cnt, valid);
    if (active) {
        double* o = P.rgb + 3 * i;
        // magenta for a null material (shading.cpp:33), the miss colour for a masked-out entry
        o[0] = valid ? (double)c.x : null_mat ? 1.0 : P.miss[0];
        o[1] = valid ? (double)c.y : null_mat ? 0.0 : P.miss[1];
        o[2] = valid ? (double)c.z : null_mat ? 1.0 : P.miss[2];
    }
    flush_occl_count(P.counters, valid ? no : 0u);
}

// The shade kernels by variant, in the tables' one form (rt_kernel_table.hpp;
// the occluded query's columns).  Columns: E D PL.  RT_GENERAL_ONLY (the
// big-stack build) keeps the general row alone.
constexpr unsigned skey(bool e, bool d, bool pl) { return (unsigned)e | (unsigned)d << 1 | (unsigned)pl << 2; }
#define RT_SHD(e, d, pl, ...) RT_KERNEL_ROW(skey(e, d, pl), __VA_ARGS__)
const KernelRow<DevScene, ShadeParams> kShadeKernels[] = {
    RT_SHD(1, 1, 0, k_shade<true, true, false>),
#ifndef RT_GENERAL_ONLY
    RT_SHD(0, 1, 0, k_shade<false, true, false>),
    RT_SHD(0, 0, 0, k_shade<false, false, false>),
    RT_SHD(0, 0, 1, k_shade<false, false, true>),
#endif
};
#undef RT_SHD

const KernelRow<DevScene, ShadeParams>* shade_row(const rtamd::KernelVariant& v) {
    return find_kernel(kShadeKernels, skey(v.eager, v.deep, v.plain));
}

// (V.lights / V.n_lights are the call's point lights: launch_lanes' own_lights)
hipError_t launch_shade(const rtamd::KernelVariant& v, int, dim3, hipStream_t st, const SceneView& V,
                        const ShadeParams& P) {
    return launch_lanes(shade_row(v), kShadePool, true, st, V, P);
}
rtamd::KernelEntry shade_kernel(const rtamd::KernelVariant& v, int) { return kernel_entry(shade_row(v)); }
const char* shade_row_name(int i) { return row_name(kShadeKernels, i); }

}  // namespace

const rtamd::KernelTable<ShadeParams>& shade_table() {
    static const rtamd::KernelTable<ShadeParams> t = {launch_shade, shade_kernel, shade_row_name, kQueryThreads, kShadePool};
    return t;
}

}  // namespace RT_NS
