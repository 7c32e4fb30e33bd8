// rt_paper_f64.hip — the outgoing-direction and paper-resolve kernels
// (namespace rtd): the links that make a paper frame a composition of the
// queries, on device buffers,
//   paper = rt_paper_resolve(hits, mask, rt_query_shade(hits, rt_rays_wo(rays), mask, miss = (1,1,1)))
//   where (hits, mask) = rt_query_intersect(rays), rays = rt_camera_rays(cam, RT_RAYS_CENTRE).
//
//   k_rays_wo: wo = (-Ray(o, d).d).normalized() (tracer.cpp:30, :115), one ray
//   per lane, with make_ray / normalized of rt_device.hpp: the functions the
//   frame kernels call, compiled with the frames' flags, so the bits are those
//   of paper_primary_body and std_body.  The 24-byte results leave through LDS
//   as contiguous 16-byte stores (8-byte ones for a wo buffer that is not
//   16-byte aligned).
//
//   k_paper_resolve: get_edge_strength + get_luminance + apply_crosshatch
//   (tracer.cpp:123-205) and the pixel of tracer.cpp:266-279 as a stencil over
//   the caller's AoS rt_hit records.  A workgroup takes a tile of kTW columns
//   by kTR rows, reads the tile's records with one halo row above and below
//   and one halo column each side, once, in 16-byte units consecutive across
//   the lanes, and keeps what the rules read (t, n, mat, the hit flag: 37 B a
//   pixel; p is dropped on the way in) in LDS.  The pixels are then evaluated
//   from LDS by the rules of paper_rules.hpp, the frames' own.  A row's
//   colours come in and its pixels go out as consecutive 8-byte words across
//   the wave, through a per-wave LDS stage.
//
// Neither has variants chosen by scene: they are not rows of the launch tables.
#include <algorithm>

#include "rt_device.hpp"
#include "rt_paper.hpp"
#include "paper_rules.hpp"

namespace RT_NS {

using rtamd::PaperResolveParams;
using rtamd::RaysWoParams;

namespace {

constexpr int kWoThreads = 256;

template <bool A16>
__global__ __launch_bounds__(kWoThreads) void k_rays_wo(RaysWoParams P) {
    const size_t k = (size_t)blockIdx.x * kWoThreads + threadIdx.x;
    V3 d = v3(RV(0.0), RV(0.0), -RV(1.0));   // (lanes past n: normalized() votes across the whole wave)
    if (k < P.n) {
        const double* r = reinterpret_cast<const double*>(P.rays + k);
        d = v3(RV(r[3]), RV(r[4]), RV(r[5]));
    }
    const V3 wo = normalized(vneg(make_ray(v3(RV(0.0), RV(0.0), RV(0.0)), d).d));
    // wave w's 64 results, 192 doubles in ray order
    __shared__ __attribute__((aligned(16))) double stage[kWoThreads / 64][192];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* w = stage[wave];
    w[3 * lane + 0] = (double)wo.x;
    w[3 * lane + 1] = (double)wo.y;
    w[3 * lane + 2] = (double)wo.z;
    __syncthreads();
    const size_t k0 = (size_t)blockIdx.x * kWoThreads + (size_t)wave * 64;   // the wave's first ray
    const int nd = k0 < P.n ? (P.n - k0 < 64 ? 3 * (int)(P.n - k0) : 192) : 0;   // its doubles
    double* out = P.wo + k0 * 3;
    if constexpr (A16) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int m = j * 64 + lane;   // 16-byte unit of the wave's 1536 B
            if (2 * m + 1 < nd) *reinterpret_cast<double2*>(out + 2 * m) = *reinterpret_cast<const double2*>(w + 2 * m);
            else if (2 * m < nd) out[2 * m] = w[2 * m];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int m = j * 64 + lane;
            if (m < nd) out[m] = w[m];
        }
    }
}

// k_paper_resolve's tile: kTW columns (a wave's width) by kTR rows per
// 256-thread workgroup; wave w evaluates tile rows w, w + 4, ...  With the halo
// a workgroup holds (kTW + 2)*(kTR + 2) records of 37 B and a 6 KiB row stage.
// RT_PAPER_TR rows, measured on config 5's 7680x4320 G-buffer (fb only, 113 B a
// pixel; a device-to-device copy of the same bytes takes 0.76 ms;
// profiles/paper_resolve/tile_rows.txt):
//    8 rows: 30 KiB, 5 workgroups (20 waves) a CU, 1.29 records read per pixel: 0.96 ms
//   16 rows: 49 KiB, 3 workgroups (12 waves) a CU, 1.16 records per pixel:      1.32 ms
//   32 rows: 89 KiB, 1 workgroup  ( 4 waves) a CU, 1.10 records per pixel:      3.21 ms
// The waves in flight that hide the load latency are worth more than the halo
// rows saved: a workgroup loads, waits and then evaluates, so only other
// workgroups of the CU cover its loads, and the halo rows a neighbour read a
// moment ago mostly come from L2.  The halo rows and columns are the only
// records another workgroup reads too.
#ifndef RT_PAPER_TR
#define RT_PAPER_TR 8
#endif
constexpr int kTW = 64, kTR = RT_PAPER_TR;
static_assert(kTR % 4 == 0, "every wave of a workgroup takes the same number of tile rows");
constexpr int kLW = kTW + 2, kLR = kTR + 2;
constexpr int kResThreads = 256;
constexpr int kResWaves = kResThreads / 64;

template <bool A16>
__device__ __forceinline__ double2 load_unit(const double* p) {
    if constexpr (A16) return *reinterpret_cast<const double2*>(p);
    else return make_double2(p[0], p[1]);
}

// A16: the hits buffer is 16-byte aligned (every record is then).
// r0: the launch's first row within the call's n_rows.
template <bool A16>
__global__ __launch_bounds__(kResThreads) void k_paper_resolve(PaperResolveParams P, int r0) {
    __shared__ double s_t[kLR][kLW], s_nx[kLR][kLW], s_ny[kLR][kLW], s_nz[kLR][kLW];
    __shared__ int s_mat[kLR][kLW];
    __shared__ unsigned char s_hit[kLR][kLW];
    __shared__ double s_stage[kResWaves][3 * kTW];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = (int)blockIdx.x * kTW;                       // the tile's first column
    const int yb = P.row0 + r0 + (int)blockIdx.y * kTR;         // and first output row (frame coordinates)
    const int y_end = min(yb + kTR, P.row0 + P.n_rows);         // end of its output rows: the lower halo row
    const int in0 = max(0, P.row0 - 1);                         // first frame row of the inputs
    const int ncols = min(kTW, P.W - x0);

    // the records: tile row lr is frame row yb - 1 + lr, tile column lx is
    // frame column x0 - 1 + lx; 16-byte unit `part` of a record holds
    // (t, p0) (p1, p2) (n0, n1) (n2, mat | front_face)
    for (int i = tid; i < kLR * kLW * 4; i += kResThreads) {
        const int lr = i / (kLW * 4), m = i - lr * (kLW * 4);
        const int lx = m >> 2, part = m & 3;
        const int y = yb - 1 + lr, x = x0 - 1 + lx;
        if (part == 1 || x < 0 || x >= P.W || y < 0 || y >= P.H || y > y_end) continue;
        const double* rec = reinterpret_cast<const double*>(P.hits + ((size_t)(y - in0) * (size_t)P.W + (size_t)x));
        const double2 u = load_unit<A16>(rec + 2 * part);
        if (part == 0) {
            s_t[lr][lx] = u.x;
        } else if (part == 2) {
            s_nx[lr][lx] = u.x;
            s_ny[lr][lx] = u.y;
        } else {
            s_nz[lr][lx] = u.x;
            s_mat[lr][lx] = (int)(unsigned)(__double_as_longlong(u.y) & 0xffffffffll);
        }
    }
    for (int i = tid; i < kLR * kLW; i += kResThreads) {
        const int lr = i / kLW, lx = i - lr * kLW;
        const int y = yb - 1 + lr, x = x0 - 1 + lx;
        if (x < 0 || x >= P.W || y < 0 || y >= P.H || y > y_end) continue;
        s_hit[lr][lx] = P.mask ? (P.mask[(size_t)(y - in0) * (size_t)P.W + (size_t)x] != 0) : 1;
    }
    __syncthreads();

    double* stage = s_stage[wave];
    // (every thread runs every round: the barriers below are workgroup-wide)
    for (int k = 0; k < kTR / kResWaves; ++k) {
        const int ty = k * kResWaves + wave;   // tile row
        const int y = yb + ty, x = x0 + lane;
        const bool row_on = y < y_end;         // wave-uniform
        const bool on = row_on && x < P.W;
        const int ly = ty + 1, lx = lane + 1;
        double v = 0.0, edge = 0.0;
        int band = 7;
        if (P.fb) {
            // the row's colours: 3 * ncols consecutive doubles
            if (row_on) {
                const double* src = P.rgb + ((size_t)(y - in0) * (size_t)P.W + (size_t)x0) * 3;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int m = j * 64 + lane;
                    if (m < 3 * ncols) stage[m] = src[m];
                }
            }
            __syncthreads();
            if (on) band = rtamd::paper::hatch_band<double>(rtamd::paper::luminance<double>(stage[3 * lane], stage[3 * lane + 1], stage[3 * lane + 2]));
        }
        if (on) {
            // neighbours (-1,0) (1,0) (0,-1) (0,1); one outside the frame is not read
            const bool nv[4] = {x - 1 >= 0, x + 1 < P.W, y - 1 >= 0, y + 1 < P.H};
            const int ny_[4] = {ly, ly, ly - 1, ly + 1}, nx_[4] = {lx - 1, lx + 1, lx, lx};
            bool nh[4];
            double nt[4], nnx[4], nny[4], nnz[4];
            int nm[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                // (a skipped neighbour's values are not looked at: the centre's stand in)
                const int a = nv[i] ? ny_[i] : ly, b = nv[i] ? nx_[i] : lx;
                nh[i] = s_hit[a][b] != 0;
                nt[i] = s_t[a][b];
                nnx[i] = s_nx[a][b];
                nny[i] = s_ny[a][b];
                nnz[i] = s_nz[a][b];
                nm[i] = s_mat[a][b];
            }
            int eidx, valid;
            edge = rtamd::paper::edge_strength<double>(s_hit[ly][lx] != 0, s_t[ly][lx], s_nx[ly][lx], s_ny[ly][lx],
                                                       s_nz[ly][lx], s_mat[ly][lx], nv, nh, nt, nnx, nny, nnz, nm, eidx,
                                                       valid);
            v = rtamd::paper::pixel_value<double>(edge, band, x, y);
            if (P.edge) P.edge[(size_t)(y - P.row0) * (size_t)P.W + (size_t)x] = edge;
        }
        if (P.fb) {
            // (a lane rewrites the three words it alone read)
            stage[3 * lane] = v;
            stage[3 * lane + 1] = v;
            stage[3 * lane + 2] = v;
            __syncthreads();
            if (row_on) {
                double* dst = P.fb + ((size_t)(y - P.row0) * (size_t)P.W + (size_t)x0) * 3;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int m = j * 64 + lane;
                    if (m < 3 * ncols) dst[m] = stage[m];
                }
            }
            // (the next round's loads into stage[m] come from the lane that read stage[m] here)
        }
    }
}

}  // namespace

hipError_t launch_rays_wo(hipStream_t st, const RaysWoParams& P) {
    if (!P.n || !P.rays || !P.wo) return hipErrorInvalidValue;
    const size_t blocks = (P.n + kWoThreads - 1) / kWoThreads;
    if (blocks >= ((size_t)1 << 31)) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(P.wo) & 15) == 0) {
        rtamd::note_launch(kNsName, "k_rays_wo<true>");
        hipLaunchKernelGGL(k_rays_wo<true>, dim3((unsigned)blocks), dim3(kWoThreads), 0, st, P);
    } else {
        rtamd::note_launch(kNsName, "k_rays_wo<false>");
        hipLaunchKernelGGL(k_rays_wo<false>, dim3((unsigned)blocks), dim3(kWoThreads), 0, st, P);
    }
    return hipGetLastError();
}

hipError_t launch_paper_resolve(hipStream_t st, const PaperResolveParams& P) {
    if (P.W <= 0 || P.H <= 0 || P.row0 < 0 || P.n_rows <= 0 || P.n_rows > P.H - P.row0 || !P.hits || (!P.fb && !P.edge) ||
        (P.fb && !P.rgb))
        return hipErrorInvalidValue;
    const bool a16 = (reinterpret_cast<uintptr_t>(P.hits) & 15) == 0;
    const unsigned gx = (unsigned)((P.W + kTW - 1) / kTW);
    constexpr int kLaunchRows = 65535 * kTR;   // the grid's y extent
    for (int r0 = 0; r0 < P.n_rows; r0 += kLaunchRows) {
        const int rows = std::min(kLaunchRows, P.n_rows - r0);
        const dim3 grid(gx, (unsigned)((rows + kTR - 1) / kTR));
        // (a launch's last row group ends at the call's last row or at a whole tile)
        if (a16) {
            rtamd::note_launch(kNsName, "k_paper_resolve<true>");
            hipLaunchKernelGGL(k_paper_resolve<true>, grid, dim3(kResThreads), 0, st, P, r0);
        } else {
            rtamd::note_launch(kNsName, "k_paper_resolve<false>");
            hipLaunchKernelGGL(k_paper_resolve<false>, grid, dim3(kResThreads), 0, st, P, r0);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace RT_NS
