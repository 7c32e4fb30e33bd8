// rt_kernels.hpp — the render kernels, built once per precision right after
// rt_device.hpp (RT_NS = rtd: FP64 parity path, rt_kernels_f64.hip; RT_NS = rtf:
// FP32 fast path, rt_kernels_f32.hip).
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
// The framebuffer, jitter draws and paper hit records stay double in both
// precisions (the float kernels convert on load / store).
// (The batched ray-query kernels k_query_isect / k_query_occl and their table
// live in rt_query_kernels.hpp, built in translation units of their own.)

#include "paper_rules.hpp"
#include "rt_kernel_table.hpp"

namespace RT_NS {

using rtamd::kCounterSlots;
using rtamd::kCounterWords;
using rtamd::PaperParams;
using rtamd::SceneView;
using rtamd::StdParams;

namespace {

// Ray / op counters: wave reduction by shuffles, block reduction through LDS,
// then one atomic per block and counter into one of kCounterSlots slots
// (blockIdx-hashed).  A single hot address would serialize ~2M atomics at the
// L2 (~6 ns each, MI355X_MICROARCH.md fan-in row) - 12 ms per 4K frame.
// Standard-mode workgroup: RT_STD_WPB waves of 2x4 pixels x 8 samples.
// Default 1 (round 6): one-wave workgroups, each with its own 10 KiB of
// dynamic LDS (lds_pool).  A workgroup's LDS is released only when its last
// wave ends, so with 4-wave workgroups a wave that finished early left its
// SIMD slot empty until the slowest wave of its group was done; single-wave
// groups let the dispatcher refill each slot as soon as its wave exits.
// Measured: recursion row 12.77 -> 10.69 ms (waves of one group take
// different numbers of bounces), config 4 6.41 -> 6.33 ms
// (profiles/r06_ab/ab_wpb.txt).
#ifndef RT_STD_WPB
#define RT_STD_WPB 1
#endif
constexpr int kStdWPB = RT_STD_WPB;
constexpr int kStdThreads = 64 * kStdWPB;
// RT_STD_TW: a wave's pixel tile is TW x (8 / TW) pixels (default 2 x 4: the 4 x 2 tile of rounds 1-4
// measured config 4 8.45 -> 8.39 ms and the recursion row 17.55 -> 15.83 ms, profiles/r05_ab/ab_std_tile.txt)
#ifndef RT_STD_TW
#define RT_STD_TW 2
#endif
constexpr int kStdTW = RT_STD_TW, kStdTH = 8 / RT_STD_TW;
static_assert(kStdTW * kStdTH == 8, "a wave holds 8 pixels");
constexpr int kStdBlockX = kStdWPB >= 2 ? 2 * kStdTW : kStdTW;            // pixels per workgroup in x
constexpr int kStdBlockY = kStdWPB >= 4 ? 2 * kStdTH : kStdTH;            // output rows per workgroup

template <bool C, int NWAVES = 4>
__device__ __forceinline__ void flush_counters(unsigned long long* ctr, uint32_t ni, uint32_t no, Cnt<C>& cnt) {
#if defined(RT_EVENT_PROF)
    constexpr int NW = C ? 18 : 2 + EV_COUNT;
#elif defined(RT_PHASE_PROF)
    constexpr int NW = C ? 18 : 2 + PH_COUNT;
#else
    constexpr int NW = C ? 18 : 2;
#endif
    // red(w)[k] lives in wave w's own region of the LDS pool (its lanes are
    // done with shading when their wave gets here)
    static_assert(NW <= 64 && 64 <= kPoolWave, "counter slots");
    auto red = [](int w) { return reinterpret_cast<unsigned long long*>(wave_pool(w)); };
    unsigned long long v[NW];
    v[0] = ni;
    v[1] = no;
    if constexpr (C) {
#pragma unroll
        for (int k = 0; k < 16; ++k) v[2 + k] = cnt.c[k];
    }
#if defined(RT_EVENT_PROF)
    if constexpr (!C) {
#pragma unroll
        for (int k = 0; k < EV_COUNT; ++k) v[2 + k] = (threadIdx.x & 63) == 0 ? cnt.get(k) : 0ull;
    }
#elif defined(RT_PHASE_PROF)
    if constexpr (!C) {
#pragma unroll
        for (int k = 0; k < PH_COUNT; ++k) v[2 + k] = (threadIdx.x & 63) == 0 ? cnt.get(k) : 0ull;
    }
#endif
#pragma unroll
    for (int k = 0; k < NW; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < NW; ++k) red(wave)[k] = v[k];
    __syncthreads();   // (a one-wave group too: lane 0's LDS writes are fenced before the wave reads them)
    if (threadIdx.x < NW) {
        unsigned long long sum = 0;
#pragma unroll
        for (int w = 0; w < NWAVES; ++w) sum += red(w)[threadIdx.x];
        const unsigned slot = (blockIdx.x + blockIdx.y * gridDim.x) % kCounterSlots;
        if (sum) atomicAdd(&ctr[(size_t)slot * kCounterWords + threadIdx.x], sum);
    }
}

// Occupancy target of the lean variants (E = D = SEC = false): 4 waves/SIMD
// caps them at 128 VGPRs; the few values the compiler then spills are
// long-lived (stored once, reloaded once), and the extra wave per SIMD hides
// FP64 latency (measured 21.6 -> 19.2 ms on config 4; 5 and 6 are slower).
#ifndef RT_LEAN_WAVES
#define RT_LEAN_WAVES 4
#endif

// A/B switches of the lean standard kernels' argument re-reads (KA below):
// the closest-hit / shading queries and the kernel's tail
// (profiles/sgpr_relief/ab_parts.txt)
#ifndef RT_KA_SHADE
#define RT_KA_SHADE 1
#endif
#ifndef RT_KA_TAIL
#define RT_KA_TAIL 1
#endif
// The standard kernels' second argument again (scene_again, rt_device.hpp):
// it follows the DevScene in the kernarg segment.
static_assert(sizeof(DevScene) % alignof(StdParams) == 0, "StdParams follows DevScene without padding");
template <bool KA>
__device__ __forceinline__ decltype(auto) std_again(const StdParams& P, int at) {
    if constexpr (KA) {
        StdParams L = args_again<StdParams>(sizeof(DevScene), at);
        L.fb = global_table(L.fb), L.counters = global_table(L.counters);
        return L;
    } else {
        return (P);
    }
}

// PL: the plain kernels (CntPlain: no transform / CSG code)
// KA: a kernel whose arguments are (DevScene S, StdParams P) handed down as
// they are (every k_std* kernel); the lean kernels ask for the re-reads
template <bool E, bool D, bool SEC, bool C, bool DL = true, int WV = 0, bool PL = false, bool KA = false>
__device__ __forceinline__ void std_body(const DevScene& S, const StdParams& P) {
    static_assert(!(PL && C), "plain kernels do not count");
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int s = lane & 7;
    const int pix = lane >> 3;
    const int x = blockIdx.x * kStdBlockX + (wave & 1) * kStdTW + (pix % kStdTW);
    const int ri = blockIdx.y * kStdBlockY + (wave >> 1) * kStdTH + (pix / kStdTW);
    const bool active = x < P.W && ri < P.n_rows;
    uint32_t ni = 0, no = 0;
    std::conditional_t<PL, CntPlain, Cnt<C>> cnt;
    cnt.init();
    V3 c = v3(RV(0.0), RV(0.0), RV(0.0));
    if (active) {
        cnt.ev(EV_WAVES);
        cnt.pb(PH_SETUP);
        const int r = P.rows[ri];
        const int y = P.H - 1 - r;   // loop row (tracer.cpp:297 writes row ny-1-y)
        // draws 16p+2s, 16p+2s+1 of the stream: dx, dy (tracer.cpp:293)
        const double2 j = *reinterpret_cast<const double2*>(P.jit + ((size_t)P.jrow[ri] * P.W + x) * 16 + 2 * s);
        const DRay ray = gen_ray_subpixel(S, x, y, RV(j.x), RV(j.y));
        cnt.pe(PH_SETUP);
        c = trace<E, D, SEC, DL, WV, RT_KA_SHADE && KA>(S, ray, ni, no, cnt);
    }
    cnt.pb(PH_TAIL);
    // acc += trace(...) for s = 0..7 in order (tracer.cpp:290-296)
    const int base = lane & ~7;
    V3 acc = v3(RV(0.0), RV(0.0), RV(0.0));
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const real cx = __shfl(c.x, base + k);
        const real cy = __shfl(c.y, base + k);
        const real cz = __shfl(c.z, base + k);
        acc.x += cx;
        acc.y += cy;
        acc.z += cz;
    }
    // (P's fields the tail needs, from the kernarg segment: not live across
    // the trace; the first lane's ray count ties the read to the trace's end)
    const StdParams& T = std_again<RT_KA_TAIL && KA>(P, (int)__builtin_amdgcn_readfirstlane(ni));
    if (active && s == 0) {
        const real inv = RV(1.0) / (real)8;
        // the pixel's row and column again, from a thread id the compiler
        // cannot match with the one above: otherwise both stay in registers
        // across the whole trace (the lean kernels sit at their 128-VGPR cap,
        // and the row index was the value that went to scratch)
        unsigned t = threadIdx.x;
        asm volatile("" : "+v"(t));
        const int wave2 = t >> 6, pix2 = (t & 63) >> 3;
        const int x2 = blockIdx.x * kStdBlockX + (wave2 & 1) * kStdTW + (pix2 % kStdTW);
        const int ri2 = blockIdx.y * kStdBlockY + (wave2 >> 1) * kStdTH + (pix2 / kStdTW);
        double* o = T.fb + ((size_t)ri2 * T.W + x2) * 3;
        o[0] = acc.x * inv;
        o[1] = acc.y * inv;
        o[2] = acc.z * inv;
    }
    cnt.pe(PH_TAIL);
    flush_counters<C, kStdWPB>(T.counters, ni, no, cnt);
}

// WV: wave-level culling (scene_occluded_wave / scene_intersect_wave), picked
// by the host for scenes with >= 4 bounded objects and culling on.
template <bool E, bool D, bool SEC, bool C, bool WV = false>
__global__ __launch_bounds__(kStdThreads) void k_std(DevScene S, StdParams P) {
    std_body<E, D, SEC, C, true, WV>(S, P);
}

// Occupancy targets of the plain variants (PL): 4 waves/SIMD (128 VGPRs),
// as the general kernels.  (A 5-wave target caps the registers at 96 and
// spills: config 3 1.10 -> 1.22 ms once the LDS pool became dynamic and no
// longer capped the compiler's occupancy estimate itself; with a static
// 40 KiB pool the target had been inert, profiles/r06_ab/ab_wpb.txt,
// ab_light_cache.txt, ab_plain_tune.txt.)
#ifndef RT_PLAIN_LEAN_WAVES
#define RT_PLAIN_LEAN_WAVES 4
#endif
// WV: 0 = per-lane culls, 1 = wave-level culls, 2 = wave-level culls over the
// wave BVH (CompiledScene::wobjs / wchunk)
template <bool C, int WV, bool PL = false>
__global__ __launch_bounds__(kStdThreads) __attribute__((amdgpu_waves_per_eu(PL ? RT_PLAIN_LEAN_WAVES : RT_LEAN_WAVES))) void k_std_lean(DevScene S,
                                                                                                       StdParams P) {
    std_body<false, false, false, C, false, WV, PL, /*KA=*/!PL>(S, P);
}

// Reflection / refraction with wave-level culling (trace_wave): the wave
// runs every bounce in lockstep.  Occupancy target RT_SEC_WAVES waves/SIMD.
#ifndef RT_SEC_WAVES
#define RT_SEC_WAVES 4
#endif
#ifndef RT_PLAIN_SEC_WAVES
#define RT_PLAIN_SEC_WAVES RT_SEC_WAVES
#endif
template <bool C, int WV = 1, bool PL = false>
__global__ __launch_bounds__(kStdThreads) __attribute__((amdgpu_waves_per_eu(PL ? RT_PLAIN_SEC_WAVES : RT_SEC_WAVES))) void k_std_secw(DevScene S,
                                                                                                      StdParams P) {
    std_body<false, false, true, C, false, WV, PL>(S, P);   // (no directional lights: those scenes take D)
}

// apply_crosshatch (tracer.cpp:188-205) in two halves (paper_rules.hpp: the one
// copy of paper mode's pixel rules, shared with k_paper_resolve and the host
// form of rt_paper_resolve).  Its FP64 part - the luminance tests - depends
// on the pixel's own shading only, so the primary pass reduces it to a band
// (0: lum < 0.15, black; 1..6: the darkness branch taken; 7: no branch,
// white; a NaN luminance takes none, as in the reference) stored with the
// material (4 bits instead of an 8-byte luminance); the finish pass applies
// the band's (x, y) pattern.
__device__ __forceinline__ int hatch_band(real lum) { return rtamd::paper::hatch_band<real>(lum); }
__device__ __forceinline__ real crosshatch(int band, int x, int y) { return rtamd::paper::crosshatch<real>(band, x, y); }
// material slot: material (>= -3) in the low 24 bits, band in bits 24-27
__device__ __forceinline__ int paper_mat_pack(int mat, int band) { return (mat & 0xffffff) | (band << 24); }
__device__ __forceinline__ int paper_mat(int slot) {   // (sign-extends the material's 24 bits)
    return static_cast<int>(static_cast<unsigned>(slot) << 8) >> 8;
}
__device__ __forceinline__ int paper_band(int slot) { return (slot >> 24) & 15; }

// Paper-mode primary records: the material slot of a pixel whose ray hit
// nothing (a hit's material is an index >= 0, or -1 for none).
constexpr int kPaperMiss = -3;



#ifndef RT_PAPER_UO
#define RT_PAPER_UO true
#endif
// The plain paper kernel keeps the shadow bundle's wave-uniform parameters in
// VGPRs (it has the registers: config 5 3.55 -> 3.51 ms,
// profiles/r06_ab/ab_uo.txt); the general one moves them to SGPRs.
#ifndef RT_PLAIN_PAPER_UO
#define RT_PLAIN_PAPER_UO false
#endif
// Paper-mode primary workgroup: RT_PAPER_WPB waves of 8x8 pixels (4: 16x16
// pixels per 256-thread workgroup; 1, the default since round 6: one wave per
// workgroup with its own 10 KiB of dynamic LDS, as RT_STD_WPB; config 5
// 3.78 -> 3.56 ms, profiles/r06_ab/ab_wpb.txt).  The host's grid is in 16x16
// units either way (launch_paper remaps it), and wave (start, end) slots stay
// per 8x8 tile.
#ifndef RT_PAPER_WPB
#define RT_PAPER_WPB 1
#endif
constexpr int kPaperWPB = RT_PAPER_WPB;
static_assert(kPaperWPB == 1 || kPaperWPB == 4, "paper workgroups of 1 or 4 waves");
constexpr int kPaperThreads = 64 * kPaperWPB;
// a wave's 8x8 tile: (tile column, list group of 8 entries)
__device__ __forceinline__ int paper_tile_x() {
    return kPaperWPB == 4 ? (int)blockIdx.x * 2 + (int)((threadIdx.x >> 6) & 1) : (int)blockIdx.x;
}
__device__ __forceinline__ int paper_tile_y() {
    return kPaperWPB == 4 ? (int)blockIdx.y * 2 + (int)(threadIdx.x >> 7) : (int)blockIdx.y;
}
// A primary wave's (start, end) tick slot: group-major, one per 8-column tile
// (2 * ceil(W / 16) of them, frame_plan.hpp paper_waves_per_group) per 8-entry
// list group.
__device__ __forceinline__ unsigned* paper_wave_slot(const PaperParams& P) {
    const unsigned g = __builtin_amdgcn_readfirstlane(paper_tile_y()), xt = __builtin_amdgcn_readfirstlane(paper_tile_x());
    const unsigned tiles = kPaperWPB == 4 ? 2 * gridDim.x : gridDim.x;
    return P.gtime + 2 * ((size_t)g * tiles + xt);
}
#ifndef RT_PAPER_LEAD_I   // (A/B switches: lead objects in the paper closest-hit / shadow queries)
#define RT_PAPER_LEAD_I true
#endif
#ifndef RT_PAPER_LEAD_S
#define RT_PAPER_LEAD_S true
#endif
template <bool E, bool D, bool C, bool DL = true, int WV = 0, bool T = false, bool PL = false>
__device__ __forceinline__ void paper_primary_body(const DevScene& S, const PaperParams& P) {
    static_assert(!(PL && C), "plain kernels do not count");
    // wave 8x8 pixels (block 16x16 or one wave, RT_PAPER_WPB)
    const int lane = threadIdx.x & 63;
    const int x = paper_tile_x() * 8 + (lane & 7);
    const int li = paper_tile_y() * 8 + (lane >> 3);
    // (list entries < 0 pad a run of consecutive rows to a wave boundary)
    const int ei = li < P.n_list ? P.ext_list[li] : -1;
    const bool active = x < P.W && ei >= 0;
    // T (timed launches, P.gtime set): the wave's cost for later frames'
    // launch order (frame_plan.hpp order_paper_groups), its start and end
    // wall-clock ticks, stored into its own slot at the end (one-address
    // atomics per list group serialised the waves: +18 % frame time).  Every
    // store of this kernel comes after its last scene read, and only timed
    // launches read the clock at the start: a global store or the clock read
    // (an intrinsic with side effects) ahead of a load from the scene's arrays
    // takes away the compiler's proof that the load sees unmodified memory,
    // and the wave-uniform object and node reads of every shadow query then
    // become vector loads instead of scalar ones (config 5 4.61 vs 5.30 ms).
    unsigned t_start = 0u;
    if constexpr (T) t_start = (unsigned)wall_clock64();
    uint32_t ni = 0, no = 0;
    std::conditional_t<PL, CntPlain, Cnt<C>> cnt;
    cnt.init();
    DRay r{v3(RV(0.0), RV(0.0), RV(0.0)), v3(RV(0.0), RV(0.0), -RV(1.0))};
    real ht = RV(0.0);
    DHit h;
    h.mat = -1;
    h.p = h.n = v3(RV(0.0), RV(0.0), RV(0.0));
    h.ff = 1;
    bool hits = false, sh = false;
    size_t idx = 0;
    if (active) {
        const int y = P.ext_rows[ei];
        r = gen_ray(S, x, y);
        ++ni;
        if constexpr (WV)
            hits = scene_intersect_wave<E, D, (WV == 2), RT_PAPER_LEAD_I>(S, r, RV(1e-4), RT_INF, ht, h, __builtin_amdgcn_read_exec() == ~0ull,
                                              cnt);
        else
            hits = scene_intersect<E, D>(S, r, RV(1e-4), RT_INF, ht, h, cnt);
        idx = (size_t)ei * P.W + x;
        sh = P.ext_shade[ei] != 0;   // (a neighbour-only row needs the hit, not the shading)
    }
    int band = 0;   // the pixel's crosshatch band (hatch_band; neighbour-only rows: unused)
    // trace_paper (tracer.cpp:111-120) + get_luminance (:123-125).  shade()
    // runs with the whole wave (lanes with nothing to shade pass valid =
    // false) so that the wave-level shadow culls keep a full wave even when
    // it mixes shaded rows and neighbour-only rows (strip edges of a
    // multi-GPU partition) or inactive lanes.
    if (__any(sh)) {
        V3 base = shade<E, D, DL, WV, PL ? RT_PLAIN_PAPER_UO : RT_PAPER_UO, RT_PAPER_LEAD_S>(S, ht, h, normalized(vneg(r.d)), no,
                                                                                     cnt, sh && hits);
        if (sh) {
            if (!hits) base = v3(RV(1.0), RV(1.0), RV(1.0));
            band = hatch_band(rtamd::paper::luminance<real>(base.x, base.y, base.z));
        }
    }
    // the material slot: the material (kPaperMiss for no hit: the finish
    // pass's hit flag) in the low 24 bits, the crosshatch band above
    if (active) {
        P.t[idx] = ht;
        P.nx[idx] = h.n.x;
        P.ny[idx] = h.n.y;
        P.nz[idx] = h.n.z;
        P.mat[idx] = paper_mat_pack(hits ? h.mat : kPaperMiss, band);
    }
    flush_counters<C, kPaperWPB>(P.counters, ni, no, cnt);
    if constexpr (T) {
        if (__lane_id() == 0) {
            unsigned* slot = paper_wave_slot(P);
            slot[0] = t_start;
            slot[1] = (unsigned)wall_clock64();
        }
    }
}

template <bool E, bool D, bool C, bool T = false>
__global__ __launch_bounds__(kPaperThreads) void k_paper_primary(DevScene S, PaperParams P) {
    paper_primary_body<E, D, C, true, 0, T>(S, P);
}

#ifndef RT_PAPER_WAVES
#define RT_PAPER_WAVES RT_LEAN_WAVES
#endif
#ifndef RT_PLAIN_PAPER_WAVES
#define RT_PLAIN_PAPER_WAVES RT_PAPER_WAVES
#endif
template <bool C, int WV, bool T = false, bool PL = false>
__global__ __launch_bounds__(kPaperThreads) __attribute__((amdgpu_waves_per_eu(PL ? RT_PLAIN_PAPER_WAVES : RT_PAPER_WAVES))) void k_paper_primary_lean(
    DevScene S, PaperParams P) {
    paper_primary_body<false, false, C, false, WV, T, PL>(S, P);
}

// One paper pixel (tracer.cpp:258-281) from its primary record and its four
// neighbours' (-1,0) (1,0) (0,-1) (0,1), already loaded.  CODES: a
// distributed frame's rank writes a paper_code byte (P.code) instead of FP64.
template <bool CODES>
__device__ __forceinline__ void paper_pixel(const PaperParams& P, int x, int y, int ri, int cm, real ct, V3 cn,
                                            int cband, const int (&nm)[4], const real (&nt)[4], const real (&nnx)[4],
                                            const real (&nny)[4], const real (&nnz)[4]) {
    // get_edge_strength (tracer.cpp:133-178): hit / miss is the material slot
    // against kPaperMiss, a neighbour outside the frame is not counted
    const bool nv[4] = {x - 1 >= 0, x + 1 < P.W, y - 1 >= 0, y + 1 < P.H};
    const bool nh[4] = {nm[0] != kPaperMiss, nm[1] != kPaperMiss, nm[2] != kPaperMiss, nm[3] != kPaperMiss};
    int eidx, valid;   // index of the strength in {0, 0.3, 0.5, 0.6, 0.9} (rtamd::paper_code); neighbours counted
    const real edge = rtamd::paper::edge_strength<real>(cm != kPaperMiss, ct, cn.x, cn.y, cn.z, cm, nv, nh, nt, nnx, nny,
                                                        nnz, nm, eidx, valid);
    if constexpr (CODES) {
        // distributed frames: the pixel's place in the output alphabet
        // (rtamd::paper_code), decoded bit-exactly on the root after the gather
        const bool h = edge <= RV(0.5) && crosshatch(cband, x, y) != RV(0.0);
        P.code[(size_t)ri * P.W + x] = (uint8_t)(eidx | (valid < 4 ? 8 : 0) | (h ? 16 : 0));
        return;
    }
    double* dst = P.fb + ((size_t)ri * P.W + x) * 3;
    if constexpr (!std::is_same_v<real, double>) {
        // The FP32 build decides in float (edge tests, hatch band) but writes the
        // reference's own FP64 alphabet, as the root of a distributed frame
        // decodes it: pixel_value<float> gave (float)0.2, (float)0.92, (float)0.94
        // in an FP64 frame whose stable pixels are otherwise the oracle's.
        const bool hw = crosshatch(cband, x, y) != RV(0.0);
        const double v = rtamd::paper_code_value((unsigned)eidx | (valid < 4 ? 8u : 0u) | (hw ? 16u : 0u));
        dst[0] = v;
        dst[1] = v;
        dst[2] = v;
        return;
    }
    const real v = rtamd::paper::pixel_value<real>(edge, cband, x, y);
    const V3 o = v3(v, v, v);
    dst[0] = o.x;
    dst[1] = o.y;
    dst[2] = o.z;
}

// A pixel pair's record in one ext row (x even, W even: 8/16-byte loads)
struct FinRec {
    int2 m;
    double2 t, nx, ny, nz;
};
__device__ __forceinline__ FinRec fin_load(const PaperParams& P, size_t i) {
    FinRec r;
    r.m = *reinterpret_cast<const int2*>(P.mat + i);
    r.t = *reinterpret_cast<const double2*>(P.t + i);
    r.nx = *reinterpret_cast<const double2*>(P.nx + i);
    r.ny = *reinterpret_cast<const double2*>(P.ny + i);
    r.nz = *reinterpret_cast<const double2*>(P.nz + i);
    return r;
}
// Pixels x and x + 1 of output row ri (frame row y) from the pair's records
// in the centre (ext index at ci), up and down rows, and their outer
// x-neighbours (loaded here).
template <bool CODES>
__device__ __forceinline__ void paper_finish_pair(const PaperParams& P, int x, int y, int ri, size_t ci, const FinRec& c,
                                                  const FinRec& u, const FinRec& d) {
    const size_t li = ci - (x > 0 ? 1 : 0), rj = ci + 1 + (x + 2 < P.W ? 1 : 0);
    const int ml = paper_mat(P.mat[li]), mr = paper_mat(P.mat[rj]);
    const real tl = P.t[li], tr = P.t[rj];
    const real xl = P.nx[li], xr = P.nx[rj], yl = P.ny[li], yr = P.ny[rj], zl = P.nz[li], zr = P.nz[rj];
    {
        const int nm[4] = {ml, paper_mat(c.m.y), paper_mat(u.m.x), paper_mat(d.m.x)};
        const real nt[4] = {tl, RV(c.t.y), RV(u.t.x), RV(d.t.x)};
        const real nnx[4] = {xl, RV(c.nx.y), RV(u.nx.x), RV(d.nx.x)}, nny[4] = {yl, RV(c.ny.y), RV(u.ny.x), RV(d.ny.x)},
                   nnz[4] = {zl, RV(c.nz.y), RV(u.nz.x), RV(d.nz.x)};
        paper_pixel<CODES>(P, x, y, ri, paper_mat(c.m.x), RV(c.t.x), v3(RV(c.nx.x), RV(c.ny.x), RV(c.nz.x)),
                           paper_band(c.m.x), nm, nt, nnx, nny, nnz);
    }
    {
        const int nm[4] = {paper_mat(c.m.x), mr, paper_mat(u.m.y), paper_mat(d.m.y)};
        const real nt[4] = {RV(c.t.x), tr, RV(u.t.y), RV(d.t.y)};
        const real nnx[4] = {RV(c.nx.x), xr, RV(u.nx.y), RV(d.nx.y)}, nny[4] = {RV(c.ny.x), yr, RV(u.ny.y), RV(d.ny.y)},
                   nnz[4] = {RV(c.nz.x), zr, RV(u.nz.y), RV(d.nz.y)};
        paper_pixel<CODES>(P, x + 1, y, ri, paper_mat(c.m.y), RV(c.t.y), v3(RV(c.nx.y), RV(c.ny.y), RV(c.nz.y)),
                           paper_band(c.m.y), nm, nt, nnx, nny, nnz);
    }
}

// The finish pass: 64x4 threads per block.  Every operand is loaded up front
// in one round of independent loads (neighbours outside the frame clamped
// onto the centre and skipped by paper_pixel; hit/miss is the material slot
// against kPaperMiss).  PAIR (even W): a thread takes two adjacent pixels
// with 8/16-byte loads of both, and their outer x-neighbours.
template <bool CODES, bool PAIR>
__device__ __forceinline__ void paper_finish_px(const PaperParams& P, int x, int ri) {
    const int y = P.rows[ri];
    const int e_up = P.nbr[3 * ri + 0], e_c = P.nbr[3 * ri + 1], e_dn = P.nbr[3 * ri + 2];
    const size_t ci = (size_t)e_c * P.W + x;
    const size_t ui = (size_t)(e_up >= 0 ? e_up : e_c) * P.W + x, di = (size_t)(e_dn >= 0 ? e_dn : e_c) * P.W + x;
    if constexpr (!PAIR) {
        const size_t nidx[4] = {ci - (x > 0 ? 1 : 0), ci + (x + 1 < P.W ? 1 : 0), ui, di};
        int nm[4];
        real nt[4], nnx[4], nny[4], nnz[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            nm[i] = paper_mat(P.mat[nidx[i]]);
            nt[i] = P.t[nidx[i]];
            nnx[i] = P.nx[nidx[i]];
            nny[i] = P.ny[nidx[i]];
            nnz[i] = P.nz[nidx[i]];
        }
        const int mc = P.mat[ci];
        paper_pixel<CODES>(P, x, y, ri, paper_mat(mc), P.t[ci], v3(P.nx[ci], P.ny[ci], P.nz[ci]), paper_band(mc), nm, nt,
                           nnx, nny, nnz);
    } else {
        // rows: c = centre, u = up, d = down; pixels x and x + 1 (x even, W even:
        // every pair is 8/16-byte aligned)
        paper_finish_pair<CODES>(P, x, y, ri, ci, fin_load(P, ci), fin_load(P, ui), fin_load(P, di));
    }
}

// RT_FINISH_RPT row rounds per block: a 64x4-thread block finishes 4 rows per
// round, so a round's up / down neighbour records were the previous round's
// centre rows (L1 / L2-hot) and only a block's first and last rows are read
// again by another block.
#ifndef RT_FINISH_RPT
#define RT_FINISH_RPT 1
#endif
// RT_FINISH_BR rows per block (64 x BR threads): a block's rows share their
// neighbour rows, only its first and last rows' are read by another block.
// (Measured and rejected in round 6: one wave walking down a 128-pixel column
// strip, its up / centre / down records kept in registers so that every
// record row is read once: config 5 3.58 -> 3.65-3.68 ms for 8-32 rows per
// wave, profiles/r06_ab/ab_finish_walk.txt.)
#ifndef RT_FINISH_BR
#define RT_FINISH_BR 4
#endif
constexpr int kFinishRounds = RT_FINISH_RPT;
constexpr int kFinishRows = RT_FINISH_BR;
template <bool CODES, bool PAIR>
__global__ __launch_bounds__(64 * kFinishRows) void k_paper_finish(PaperParams P) {
    const int xt = blockIdx.x * 64 + (threadIdx.x & 63);
    const int x = PAIR ? 2 * xt : xt;
    if (x >= P.W) return;
    for (int k = 0; k < kFinishRounds; ++k) {
        const int ri = (blockIdx.y * kFinishRounds + k) * kFinishRows + (threadIdx.x >> 6);
        if (ri >= P.n_rows) return;
        paper_finish_px<CODES, PAIR>(P, x, ri);
    }
}

// Dynamic LDS of the kernels that shade (lds_pool): one region per wave
constexpr size_t kStdPool = pool_bytes(kStdThreads), kPaperPool = pool_bytes(kPaperThreads);
// the paper primary's grid from the host's 16x16-pixel units
inline dim3 pgrid(dim3 g) { return kPaperWPB == 4 ? g : dim3(2 * g.x, 2 * g.y); }

// The trace kernels by variant: one table per mode, in the tables' one form
// (rt_kernel_table.hpp).  (The untimed k_paper_primary entries leave T at its
// default: the name rt_test_kernel_name has always reported.)
// Columns: E D SEC C WV PL (T), the KernelVariant fields an entry answers to
// (frame_plan.hpp pick_variant produces only canonical variants).
// RT_GENERAL_ONLY (the big-stack build) keeps the general E = D = true rows,
// RT_NO_PLAIN (the FP32 diagnostic build) drops the PL rows: a variant
// without a row has no kernel in this namespace, and its launch is an error.
constexpr unsigned vkey(bool e, bool d, bool sec, bool c, int wv, bool pl, bool t) {
    return (unsigned)e | (unsigned)d << 1 | (unsigned)sec << 2 | (unsigned)c << 3 | (unsigned)pl << 4 |
           (unsigned)t << 5 | (unsigned)wv << 6;
}
#define RT_ROW(e, d, sec, c, wv, pl, t, ...) RT_KERNEL_ROW(vkey(e, d, sec, c, wv, pl, t), __VA_ARGS__)
#define RT_STD(e, d, sec, c, wv, pl, ...) RT_ROW(e, d, sec, c, wv, pl, 0, __VA_ARGS__)
#define RT_PAP(e, d, c, wv, pl, t, ...) RT_ROW(e, d, 0, c, wv, pl, t, __VA_ARGS__)
const KernelRow<DevScene, StdParams> kStdKernels[] = {
    RT_STD(1, 1, 0, 0, 0, 0, k_std<true, true, false, false, false>),
    RT_STD(1, 1, 0, 1, 0, 0, k_std<true, true, false, true, false>),
    RT_STD(1, 1, 1, 0, 0, 0, k_std<true, true, true, false, false>),
    RT_STD(1, 1, 1, 1, 0, 0, k_std<true, true, true, true, false>),
#ifndef RT_GENERAL_ONLY
    RT_STD(0, 1, 0, 0, 0, 0, k_std<false, true, false, false, false>),
    RT_STD(0, 1, 0, 1, 0, 0, k_std<false, true, false, true, false>),
    RT_STD(0, 1, 1, 0, 0, 0, k_std<false, true, true, false, false>),
    RT_STD(0, 1, 1, 1, 0, 0, k_std<false, true, true, true, false>),
    RT_STD(0, 0, 1, 0, 0, 0, k_std<false, false, true, false, false>),   // (reflection without wave culls)
    RT_STD(0, 0, 1, 1, 0, 0, k_std<false, false, true, true, false>),
    RT_STD(0, 0, 0, 0, 0, 0, k_std_lean<false, 0, false>),
    RT_STD(0, 0, 0, 0, 1, 0, k_std_lean<false, 1, false>),
    RT_STD(0, 0, 0, 0, 2, 0, k_std_lean<false, 2, false>),
    RT_STD(0, 0, 0, 1, 0, 0, k_std_lean<true, 0, false>),
    RT_STD(0, 0, 0, 1, 1, 0, k_std_lean<true, 1, false>),
    RT_STD(0, 0, 0, 1, 2, 0, k_std_lean<true, 2, false>),
    RT_STD(0, 0, 1, 0, 1, 0, k_std_secw<false, 1, false>),
    RT_STD(0, 0, 1, 0, 2, 0, k_std_secw<false, 2, false>),
    RT_STD(0, 0, 1, 1, 1, 0, k_std_secw<true, 1, false>),
    RT_STD(0, 0, 1, 1, 2, 0, k_std_secw<true, 2, false>),
#ifndef RT_NO_PLAIN
    RT_STD(0, 0, 0, 0, 0, 1, k_std_lean<false, 0, true>),
    RT_STD(0, 0, 0, 0, 1, 1, k_std_lean<false, 1, true>),
    RT_STD(0, 0, 0, 0, 2, 1, k_std_lean<false, 2, true>),
    RT_STD(0, 0, 1, 0, 1, 1, k_std_secw<false, 1, true>),
    RT_STD(0, 0, 1, 0, 2, 1, k_std_secw<false, 2, true>),
#endif
#endif
};
// (timed launches: never op-counting ones, rt_frame_trace)
const KernelRow<DevScene, PaperParams> kPaperKernels[] = {
    RT_PAP(1, 1, 0, 0, 0, 0, k_paper_primary<true, true, false>),
    RT_PAP(1, 1, 0, 0, 0, 1, k_paper_primary<true, true, false, true>),
    RT_PAP(1, 1, 1, 0, 0, 0, k_paper_primary<true, true, true>),
#ifndef RT_GENERAL_ONLY
    RT_PAP(0, 1, 0, 0, 0, 0, k_paper_primary<false, true, false>),
    RT_PAP(0, 1, 0, 0, 0, 1, k_paper_primary<false, true, false, true>),
    RT_PAP(0, 1, 1, 0, 0, 0, k_paper_primary<false, true, true>),
    RT_PAP(0, 0, 0, 0, 0, 0, k_paper_primary_lean<false, 0, false, false>),
    RT_PAP(0, 0, 0, 1, 0, 0, k_paper_primary_lean<false, 1, false, false>),
    RT_PAP(0, 0, 0, 2, 0, 0, k_paper_primary_lean<false, 2, false, false>),
    RT_PAP(0, 0, 0, 0, 0, 1, k_paper_primary_lean<false, 0, true, false>),
    RT_PAP(0, 0, 0, 1, 0, 1, k_paper_primary_lean<false, 1, true, false>),
    RT_PAP(0, 0, 0, 2, 0, 1, k_paper_primary_lean<false, 2, true, false>),
    RT_PAP(0, 0, 1, 0, 0, 0, k_paper_primary_lean<true, 0, false, false>),
    RT_PAP(0, 0, 1, 1, 0, 0, k_paper_primary_lean<true, 1, false, false>),
    RT_PAP(0, 0, 1, 2, 0, 0, k_paper_primary_lean<true, 2, false, false>),
#ifndef RT_NO_PLAIN
    RT_PAP(0, 0, 0, 0, 1, 0, k_paper_primary_lean<false, 0, false, true>),
    RT_PAP(0, 0, 0, 1, 1, 0, k_paper_primary_lean<false, 1, false, true>),
    RT_PAP(0, 0, 0, 2, 1, 0, k_paper_primary_lean<false, 2, false, true>),
    RT_PAP(0, 0, 0, 0, 1, 1, k_paper_primary_lean<false, 0, true, true>),
    RT_PAP(0, 0, 0, 1, 1, 1, k_paper_primary_lean<false, 1, true, true>),
    RT_PAP(0, 0, 0, 2, 1, 1, k_paper_primary_lean<false, 2, true, true>),
#endif
#endif
};
#undef RT_PAP
#undef RT_STD
#undef RT_ROW

// The finish kernels by (CODES, PAIR).  RT_NO_PAPER_CODES (the FP32 build)
// drops the CODES rows: paper codes need an FP64 frame (rt_frame.hip
// frame_trace refuses them with RT_FLAG_FP32, and rt_dist.hip gathers doubles
// from FP32 ranks), so no frame can ask this namespace for them.
constexpr unsigned fkey(bool codes, bool pair) { return (unsigned)codes | (unsigned)pair << 1; }
#define RT_FIN(codes, pair, ...) RT_KERNEL_ROW(fkey(codes, pair), __VA_ARGS__)
const KernelRow<PaperParams> kFinishKernels[] = {
    RT_FIN(0, 0, k_paper_finish<false, false>),
    RT_FIN(0, 1, k_paper_finish<false, true>),
#ifndef RT_NO_PAPER_CODES
    RT_FIN(1, 0, k_paper_finish<true, false>),
    RT_FIN(1, 1, k_paper_finish<true, true>),
#endif
};
#undef RT_FIN

// (the standard-mode kernels have no timed build, the paper ones no SEC)
const KernelRow<DevScene, StdParams>* std_row(const rtamd::KernelVariant& v) {
    return find_kernel(kStdKernels, vkey(v.eager, v.deep, v.secondary, v.count_ops, v.wv, v.plain, false));
}
const KernelRow<DevScene, PaperParams>* paper_row(const rtamd::KernelVariant& v) {
    return find_kernel(kPaperKernels, vkey(v.eager, v.deep, false, v.count_ops, v.wv, v.plain, v.timed));
}

// Each variant gets its own register allocation.  A variant this namespace
// has no kernel for is an error, never another kernel.
hipError_t launch_std(const rtamd::KernelVariant& v, int, dim3, hipStream_t st, const SceneView& V, const StdParams& P) {
    const KernelRow<DevScene, StdParams>* k = std_row(v);
    if (!k) return hipErrorInvalidDeviceFunction;
    const DevScene S = make_scene(V, v.wv == 2);
    const dim3 grid((P.W + kStdBlockX - 1) / kStdBlockX, (P.n_rows + kStdBlockY - 1) / kStdBlockY);
    rtamd::note_launch(kNsName, k->name);
    hipLaunchKernelGGL(k->fn, grid, dim3(kStdThreads), kStdPool, st, S, P);
    return hipGetLastError();
}

hipError_t launch_paper(const rtamd::KernelVariant& v, int, dim3 grid, hipStream_t st, const SceneView& V,
                        const PaperParams& P) {
    const KernelRow<DevScene, PaperParams>* k = paper_row(v);
    if (!k) return hipErrorInvalidDeviceFunction;
    const DevScene S = make_scene(V, v.wv == 2);
    rtamd::note_launch(kNsName, k->name);
    hipLaunchKernelGGL(k->fn, pgrid(grid), dim3(kPaperThreads), kPaperPool, st, S, P);
    return hipGetLastError();
}

hipError_t launch_paper_finish(const rtamd::KernelVariant&, int, dim3 grid, hipStream_t st, const SceneView&,
                               const PaperParams& P) {
    // (grid.x covers W pixels one per thread; even W: two per thread; grid.y
    // kFinishRows * kFinishRounds rows per block)
    const bool pair = P.W % 2 == 0;
    const KernelRow<PaperParams>* k = find_kernel(kFinishKernels, fkey(P.code != nullptr, pair));
    if (!k) return hipErrorInvalidDeviceFunction;
    grid.y = (P.n_rows + kFinishRows * kFinishRounds - 1) / (kFinishRows * kFinishRounds);
    if (pair) grid.x = (P.W / 2 + 63) / 64;
    rtamd::note_launch(kNsName, k->name);
    hipLaunchKernelGGL(k->fn, grid, dim3(64 * kFinishRows), 0, st, P);
    return hipGetLastError();
}

rtamd::KernelEntry std_kernel(const rtamd::KernelVariant& v, int) { return kernel_entry(std_row(v)); }
rtamd::KernelEntry paper_kernel(const rtamd::KernelVariant& v, int) { return kernel_entry(paper_row(v)); }
rtamd::KernelEntry finish_kernel(const rtamd::KernelVariant&, int kind) {
    return kernel_entry(find_kernel(kFinishKernels, (unsigned)kind));
}
const char* std_row_name(int i) { return row_name(kStdKernels, i); }
const char* paper_row_name(int i) { return row_name(kPaperKernels, i); }
const char* finish_row_name(int i) { return row_name(kFinishKernels, i); }

}  // namespace

// The tables as the host sees them (rt_launch.hpp): the launcher, the kernel a
// launch picks for a variant, row i as written above, and the trace kernels'
// workgroup size and dynamic LDS.  (The finish table's kernel(v, kind): kind
// is its key, CODES | PAIR << 1.)
const rtamd::KernelTable<StdParams>& std_table() {
    static const rtamd::KernelTable<StdParams> t = {launch_std, std_kernel, std_row_name, kStdThreads, kStdPool};
    return t;
}
const rtamd::KernelTable<PaperParams>& paper_table() {
    static const rtamd::KernelTable<PaperParams> t = {launch_paper, paper_kernel, paper_row_name, kPaperThreads, kPaperPool};
    return t;
}
const rtamd::KernelTable<PaperParams>& finish_table() {
    static const rtamd::KernelTable<PaperParams> t = {launch_paper_finish, finish_kernel, finish_row_name,
                                                      64 * kFinishRows, 0};
    return t;
}

}  // namespace RT_NS
