// rt_bounce_f64.hip — the bounce-loop kernels (namespace rtd): the recursion
// of Tracer::trace_recursive (tracer.cpp:22-73) as two links over device
// buffers,
//   children = rt_scatter_rays(rays, hits, mask, depth)         the spawn half
//   total    = rt_combine_bounce(direct, spawn, first, child colours, weights)   the unwind half
// so that radiance = the loop intersect -> shade -> scatter per level, then
// combine from the last level up (rt.h, "bounce-by-bounce tracing").
//
// Scatter: an ordered compaction without atomics on the output position and
// without any workgroup waiting on another (no decoupled look-back, no flag
// spins: a scan of more than one level is more launches).
//   k_scatter_count: one lane per parent decides its spawn bits with
//   reflect_dir / incident_cos / refract_sin_t2 of rt_device.hpp - the functions
//   trace() and trace_wave() call, compiled with the frames' flags (no FP
//   contraction, IEEE div / sqrt) - writes spawn[i], and the workgroup's child
//   count from the popcounts of the two ballots.
//   k_scan_tile / k_scan_add: the exclusive scan of the workgroup counts,
//   kScatterTile counts per workgroup and level.
//   k_scatter_emit: the lane's offset is the popcount of the two ballots below
//   the lane; it writes first[i], and the wave's children (origins,
//   directions, weights) leave through LDS as contiguous 16-byte stores
//   (rt_camera_f64.hip measured 1.5-1.7x for that on the same 64 B records).
// The emit pass rereads spawn[i] (1 B of the ~130 B a parent costs it) instead
// of taking its own decision for the truth: the offsets were scanned from those
// bytes, so positions and records agree by construction whatever the two
// kernels' code looks like; the terms the decision needs (incident, eta,
// sin_t2) are recomputed anyway, because the children's directions are made of
// them.
//
// Neither link has variants chosen by scene: they are not rows of the launch
// tables.
#include <algorithm>

#include "rt_device.hpp"
#include "rt_bounce.hpp"

namespace RT_NS {

using rtamd::CombineParams;
using rtamd::kScatterThreads;
using rtamd::kScatterTile;
using rtamd::ScatterParams;

namespace {

constexpr int kWaves = kScatterThreads / 64;
static_assert(kScatterTile == kScatterThreads, "k_scan_tile scans one count per thread");

// Parent i as a lane holds it.  A lane past n, a miss and a null material hold
// values every expression below accepts (every lane of a wave runs the same
// statements: normalized() votes across the wave) and spawn nothing.
struct Parent {
    V3 d;
    DHit h;
    real kr, kt, ri;
    bool on;
};

__device__ __forceinline__ Parent load_parent(const ScatterParams& P, size_t i) {
    Parent pa;
    pa.d = v3(RV(0.0), RV(0.0), -RV(1.0));
    pa.h.p = pa.h.n = v3(RV(0.0), RV(0.0), RV(0.0));
    pa.h.mat = -1;
    pa.h.ff = 1;
    pa.kr = pa.kt = RV(0.0);
    pa.ri = RV(1.0);
    pa.on = false;
    if (i < P.n && (!P.mask || P.mask[i] != 0)) {
        const rt_hit& h = P.hits[i];
        const int mat = h.mat;
        if (mat >= 0 && mat < P.n_mats) {   // (-1, or a garbage index: a null material, no table is read)
            const rt_ray& r = P.rays[i];
            pa.d = v3(RV(r.d[0]), RV(r.d[1]), RV(r.d[2]));
            pa.h.p = v3(RV(h.p[0]), RV(h.p[1]), RV(h.p[2]));
            pa.h.n = v3(RV(h.n[0]), RV(h.n[1]), RV(h.n[2]));
            pa.h.mat = mat;
            pa.h.ff = h.front_face;
            const MatT& m = static_cast<const MatT*>(P.mats)[mat];
            pa.kr = m.kr;
            pa.kt = m.kt;
            pa.ri = m.refractive_index;
            pa.on = true;
        }
    }
    return pa;
}

// tracer.cpp:38-59 up to the two decisions
struct Terms {
    V3 inc;
    real eta, cos_i, st2;
    unsigned bits;
};
__device__ __forceinline__ Terms spawn_terms(const ScatterParams& P, const Parent& pa) {
    Terms t;
    // r = Ray(o, d) (core.h:278), incident = r.d.normalized() (tracer.cpp:40, 57)
    t.inc = normalized(make_ray(v3(RV(0.0), RV(0.0), RV(0.0)), pa.d).d);
    t.eta = pa.h.ff ? (RV(P.medium_index) / pa.ri) : (pa.ri / RV(P.medium_index));   // tracer.cpp:53-55
    t.cos_i = incident_cos(t.inc, pa.h.n);
    t.st2 = refract_sin_t2(t.eta, t.cos_i);
    const bool can = pa.on && P.can;
    const bool refl = pa.kr > RV(0.0) && can;
    const bool refr = pa.kt > RV(0.0) && can && !(t.st2 >= RV(1.0));
    t.bits = (refl ? RT_SPAWN_REFLECT : 0u) | (refr ? RT_SPAWN_REFRACT : 0u);
    return t;
}

// The wave's children of the two kinds, and the workgroup's over its waves
__device__ __forceinline__ unsigned wave_children(unsigned bits, unsigned long long& b1, unsigned long long& b2) {
    b1 = __ballot((bits & RT_SPAWN_REFLECT) != 0);
    b2 = __ballot((bits & RT_SPAWN_REFRACT) != 0);
    return (unsigned)__popcll(b1) + (unsigned)__popcll(b2);
}

__global__ __launch_bounds__(kScatterThreads) void k_scatter_count(ScatterParams P) {
    const size_t i = (size_t)blockIdx.x * kScatterThreads + threadIdx.x;
    const Terms t = spawn_terms(P, load_parent(P, i));
    if (i < P.n) P.spawn[i] = (uint8_t)t.bits;
    __shared__ unsigned s_wc[kWaves];
    unsigned long long b1, b2;
    const unsigned wc = wave_children(t.bits, b1, b2);
    if ((threadIdx.x & 63) == 0) s_wc[threadIdx.x >> 6] = wc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned c = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) c += s_wc[w];
        P.counts[blockIdx.x] = c;
    }
}

// v[0, m) in tiles of kScatterTile: each tile's exclusive scan in place, its
// total to sums[tile] (TOP: one tile, its total to *total instead).
template <bool TOP>
__global__ __launch_bounds__(kScatterTile) void k_scan_tile(uint32_t* v, size_t m, uint32_t* sums, uint64_t* total) {
    const size_t e = (size_t)blockIdx.x * kScatterTile + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t x = e < m ? v[e] : 0u;
    uint32_t inc = x;   // the wave's inclusive scan
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(inc, o, 64);
        if (lane >= o) inc += y;
    }
    __shared__ uint32_t s_w[kScatterTile / 64];
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kScatterTile / 64; ++w) {
        if (w < wave) before += s_w[w];
        all += s_w[w];
    }
    if (e < m) v[e] = before + inc - x;
    if (threadIdx.x == 0) {
        if constexpr (TOP) *total = all;
        else sums[blockIdx.x] = all;
    }
}

__global__ __launch_bounds__(kScatterTile) void k_scan_add(uint32_t* v, size_t m, const uint32_t* sums) {
    const size_t e = (size_t)blockIdx.x * kScatterTile + threadIdx.x;
    if (e < m) v[e] += sums[blockIdx.x];
}

// The interval Tracer::trace_recursive queries (tracer.cpp:29)
constexpr double kRayTmin = 1e-4;

// A16: child_rays is 16-byte aligned (every record is then).
template <bool A16>
__global__ __launch_bounds__(kScatterThreads) void k_scatter_emit(ScatterParams P) {
    const size_t i = (size_t)blockIdx.x * kScatterThreads + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Parent pa = load_parent(P, i);
    const Terms t = spawn_terms(P, pa);
    // the decision the offsets were scanned from
    const unsigned bits = i < P.n ? (unsigned)P.spawn[i] & (RT_SPAWN_REFLECT | RT_SPAWN_REFRACT) : 0u;
    unsigned long long b1, b2;
    const unsigned wc = wave_children(bits, b1, b2);   // <= 128
    __shared__ unsigned s_wc[kWaves];
    // wave w's children, transposed: part q of child c at [q*128 + c]; 16-byte
    // unit m of the wave's records is part m % 4 of child m / 4
    __shared__ double2 s_rec[kWaves][4 * 128];
    __shared__ double s_w[kWaves][128];
    if (lane == 0) s_wc[wave] = wc;
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned off = (unsigned)__popcll(b1 & below) + (unsigned)__popcll(b2 & below);   // the lane's first child in the wave
    // both children of every lane (the statements are the wave's; a lane
    // stages only what it spawns)
    const V3 rd1 = reflect_dir(t.inc, pa.h.n);
    const V3 ro1 = pa.h.ff ? origin_above(pa.h) : origin_below(pa.h);
    const V3 rd2 = refract_dir(t.inc, pa.h.n, t.eta, t.cos_i, t.st2);
    const V3 ro2 = pa.h.ff ? origin_below(pa.h) : origin_above(pa.h);
    double2* rec = s_rec[wave];
    if (bits & RT_SPAWN_REFLECT) {
        const unsigned c = off;
        rec[c] = make_double2((double)ro1.x, (double)ro1.y);
        rec[128 + c] = make_double2((double)ro1.z, (double)rd1.x);
        rec[256 + c] = make_double2((double)rd1.y, (double)rd1.z);
        rec[384 + c] = make_double2(kRayTmin, __builtin_inf());
        s_w[wave][c] = (double)pa.kr;
    }
    if (bits & RT_SPAWN_REFRACT) {
        const unsigned c = off + (bits & RT_SPAWN_REFLECT);
        rec[c] = make_double2((double)ro2.x, (double)ro2.y);
        rec[128 + c] = make_double2((double)ro2.z, (double)rd2.x);
        rec[256 + c] = make_double2((double)rd2.y, (double)rd2.z);
        rec[384 + c] = make_double2(kRayTmin, __builtin_inf());
        s_w[wave][c] = (double)pa.kt;
    }
    __syncthreads();
    unsigned wave_off = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w)
        if (w < wave) wave_off += s_wc[w];
    const uint64_t j0 = P.base + (uint64_t)P.counts[blockIdx.x] + wave_off;   // the wave's first child of the call
    if (i < P.n) P.first[i] = j0 + off;
    // children of the wave that the call's buffers hold
    const unsigned nw = j0 >= P.child_cap ? 0u : (P.child_cap - j0 < (uint64_t)wc ? (unsigned)(P.child_cap - j0) : wc);
    for (unsigned c = lane; c < nw; c += 64) P.child_w[j0 + c] = s_w[wave][c];
    double* out = reinterpret_cast<double*>(P.child_rays + j0);
    for (unsigned m = lane; m < 4 * nw; m += 64) {
        const double2 u = rec[(m & 3) * 128 + (m >> 2)];
        if constexpr (A16) {
            *reinterpret_cast<double2*>(out + 2 * m) = u;
        } else {
            out[2 * m] = u.x;
            out[2 * m + 1] = u.y;
        }
    }
}

constexpr int kCombineThreads = 256;

__global__ __launch_bounds__(kCombineThreads) void k_combine_bounce(CombineParams P) {
    const size_t i = (size_t)blockIdx.x * kCombineThreads + threadIdx.x;
    if (i >= P.n) return;
    const unsigned bits = P.spawn[i];
    if (!(bits & (RT_SPAWN_REFLECT | RT_SPAWN_REFRACT))) return;
    double* c = P.rgb + 3 * i;
    V3 total = v3(RV(c[0]), RV(c[1]), RV(c[2]));
    const uint64_t f = P.first[i];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        if (!(bits & (1u << b))) continue;
        const uint64_t j = f + (b ? (uint64_t)(bits & 1u) : 0ull);
        if (j >= P.n_children) continue;   // (a garbage index reads nothing)
        const double* I = P.child_rgb + 3 * j;
        const real k = RV(P.child_w[j]);
        total = combine(total, v3(RV(I[0]) * k, RV(I[1]) * k, RV(I[2]) * k));   // tracer.cpp:47, 66
    }
    c[0] = (double)total.x;
    c[1] = (double)total.y;
    c[2] = (double)total.z;
}

size_t tiles(size_t m) { return (m + kScatterTile - 1) / kScatterTile; }

// The exclusive scan of v[0, m) in place, its total to *total: one tile on top,
// and below it per level the tiles' scans, the scan of their totals (in the
// words behind v's) and the add.
hipError_t scan(hipStream_t st, uint32_t* v, size_t m, uint64_t* total) {
    if (m <= (size_t)kScatterTile) {
        rtamd::note_launch(kNsName, "k_scan_tile<true>");
        hipLaunchKernelGGL(k_scan_tile<true>, dim3(1), dim3(kScatterTile), 0, st, v, m, nullptr, total);
        return hipGetLastError();
    }
    const size_t nt = tiles(m);
    uint32_t* sums = v + m;
    rtamd::note_launch(kNsName, "k_scan_tile<false>");
    hipLaunchKernelGGL(k_scan_tile<false>, dim3((unsigned)nt), dim3(kScatterTile), 0, st, v, m, sums, nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = scan(st, sums, nt, total);
    if (e != hipSuccess) return e;
    rtamd::note_launch(kNsName, "k_scan_add");
    hipLaunchKernelGGL(k_scan_add, dim3((unsigned)nt), dim3(kScatterTile), 0, st, v, m, sums);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_scatter(hipStream_t st, const ScatterParams& P) {
    if (!P.n || P.n > ((size_t)1 << 30) || !P.rays || !P.hits || !P.spawn || !P.first || !P.counts || !P.total ||
        (P.child_cap && (!P.child_rays || !P.child_w)) || (P.n_mats > 0 && !P.mats))
        return hipErrorInvalidValue;
    const size_t wgs = (P.n + kScatterThreads - 1) / kScatterThreads;   // <= 2^22
    rtamd::note_launch(kNsName, "k_scatter_count");
    hipLaunchKernelGGL(k_scatter_count, dim3((unsigned)wgs), dim3(kScatterThreads), 0, st, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = scan(st, P.counts, wgs, P.total);
    if (e != hipSuccess) return e;
    if ((reinterpret_cast<uintptr_t>(P.child_rays) & 15) == 0) {
        rtamd::note_launch(kNsName, "k_scatter_emit<true>");
        hipLaunchKernelGGL(k_scatter_emit<true>, dim3((unsigned)wgs), dim3(kScatterThreads), 0, st, P);
    } else {
        rtamd::note_launch(kNsName, "k_scatter_emit<false>");
        hipLaunchKernelGGL(k_scatter_emit<false>, dim3((unsigned)wgs), dim3(kScatterThreads), 0, st, P);
    }
    return hipGetLastError();
}

hipError_t launch_combine_bounce(hipStream_t st, const CombineParams& P) {
    if (!P.n || !P.rgb || !P.spawn || !P.first || (P.n_children && (!P.child_rgb || !P.child_w))) return hipErrorInvalidValue;
    const size_t blocks = (P.n + kCombineThreads - 1) / kCombineThreads;
    if (blocks >= ((size_t)1 << 31)) return hipErrorInvalidValue;
    rtamd::note_launch(kNsName, "k_combine_bounce");
    hipLaunchKernelGGL(k_combine_bounce, dim3((unsigned)blocks), dim3(kCombineThreads), 0, st, P);
    return hipGetLastError();
}

}  // namespace RT_NS

// the words of a group's scan: the workgroup counts and every level's sums
size_t rtamd::scatter_count_words(size_t n) {
    size_t m = (n + kScatterThreads - 1) / kScatterThreads, words = 0;
    for (;;) {
        words += m;
        if (m <= (size_t)kScatterTile) return words;
        m = (m + kScatterTile - 1) / kScatterTile;
    }
}
