// rt_camera_f64.hip — the camera-ray and sample-resolve kernels (namespace
// rtd): the first and the last link of a frame composed from the queries,
//   frame = rt_resolve_samples(rt_query_radiance(rt_camera_rays(camera))).
//
//   k_camera_rays<JITTERED>: Camera::generate_ray (camera.h:44-58) at the pixel
//   centres, or Camera::generate_ray_subpixel (camera.h:68-78) at the frame's
//   own mt19937(12345) jitter draws (tracer.cpp:284-293), through gen_ray /
//   gen_ray_subpixel of rt_device.hpp: the functions the frame kernels call,
//   compiled with the frames' flags (no FP contraction, IEEE div / sqrt), so
//   the rays are the frames' rays bit for bit.  One lane per ray; a grid row
//   per list entry, so no lane divides by W.  The centre variant reads nothing
//   but its arguments (and the rows list when the caller gave one), the
//   jittered variant 16 B of draws per ray.  The 64 B records leave as 16-byte
//   vector stores, four per lane, staged through LDS so that each store
//   instruction of a wave writes 1 KiB of consecutive bytes (RT_CAMERA_STAGED).
//
//   k_resolve_samples: the frame's `acc += trace(...)` over the samples in
//   order, then `acc * (1.0 / spp)` (tracer.cpp:291-296), one lane per pixel
//   channel.
//
// Neither has variants chosen by scene: they are not rows of the launch tables.
#include <algorithm>

#include "rt_device.hpp"
#include "rt_camera.hpp"

// RT_CAMERA_STAGED=1 (default): a wave's 64 rays (4 KiB) go through LDS and
// leave as four contiguous 1 KiB stores, 16 B per lane each; 0: every lane
// stores its own 64 B record, four 16-byte stores at a 64 B stride between
// lanes.  Measured on config 4's 8.3 M rays (531 MB): centre 156 -> 90 us,
// jittered 181 -> 119 us (DESIGN.md §Camera rays and sample resolve,
// profiles/camera_rays/).  The rays are the same bit for bit.
#ifndef RT_CAMERA_STAGED
#define RT_CAMERA_STAGED 1
#endif

namespace RT_NS {

using rtamd::CameraParams;
using rtamd::ResolveParams;

namespace {

constexpr int kCamThreads = 256;
constexpr int kResolveThreads = 256;

// The camera fields of a DevScene: all gen_ray / gen_ray_subpixel read.
__device__ __forceinline__ DevScene camera_scene(const CameraParams& P) {
    DevScene S{};
    S.cam_nx = P.cam_nx;
    S.cam_ny = P.cam_ny;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        S.eye[i] = (real)P.eye[i];
        S.P[i] = (real)P.P[i];
    }
    S.Lx = (real)P.Lx;
    S.Ly = (real)P.Ly;
    return S;
}

// The interval Tracer::trace, trace_paper and get_edge_strength query
// (tracer.cpp:29, 114, 136-156)
constexpr double kRayTmin = 1e-4;

template <bool JITTERED>
__global__ __launch_bounds__(kCamThreads) void k_camera_rays(CameraParams P) {
    const unsigned per_row = JITTERED ? (unsigned)P.W * RT_SPP : (unsigned)P.W;
    const unsigned k = blockIdx.x * kCamThreads + threadIdx.x;   // the lane's ray within its list entry
    const bool active = k < per_row;
    const int ri = P.ri0 + (int)blockIdx.y;
    DRay ray = DRay{v3(RV(0.0), RV(0.0), RV(0.0)), v3(RV(0.0), RV(0.0), RV(0.0))};
    if (active) {
        const DevScene S = camera_scene(P);
        if constexpr (JITTERED) {
            const int x = (int)(k / RT_SPP), s = (int)(k % RT_SPP);
            const int y = P.H - 1 - P.rows[ri];   // loop row (tracer.cpp:297 writes row ny-1-y)
            // draws 16p+2s, 16p+2s+1 of the stream: dx, dy (tracer.cpp:293), as std_body reads them
            const double2 j = *reinterpret_cast<const double2*>(P.jit + ((size_t)P.jrow[ri] * P.W + x) * 16 + 2 * s);
            ray = gen_ray_subpixel(S, x, y, RV(j.x), RV(j.y));
        } else {
            ray = gen_ray(S, (int)k, P.rows ? P.rows[ri] : ri);
        }
    }
    double2* out = reinterpret_cast<double2*>(P.rays + (size_t)blockIdx.y * per_row);
    const double2 q0 = make_double2((double)ray.o.x, (double)ray.o.y);
    const double2 q1 = make_double2((double)ray.o.z, (double)ray.d.x);
    const double2 q2 = make_double2((double)ray.d.y, (double)ray.d.z);
    const double2 q3 = make_double2(kRayTmin, __builtin_inf());
#if RT_CAMERA_STAGED
    // wave w's rays, transposed: part q of lane l at [q*64 + l]; 16-byte unit m
    // of the wave's 4 KiB is part m % 4 of ray m / 4
    __shared__ double2 stage[kCamThreads / 64][4 * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double2* w = stage[wave];
    w[lane] = q0;
    w[64 + lane] = q1;
    w[128 + lane] = q2;
    w[192 + lane] = q3;
    __syncthreads();
    const unsigned k0 = blockIdx.x * kCamThreads + wave * 64;   // the wave's first ray
    const unsigned nv = k0 < per_row ? (per_row - k0 < 64u ? per_row - k0 : 64u) : 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned m = j * 64 + lane;
        if (m < 4 * nv) out[(size_t)k0 * 4 + m] = w[(m & 3) * 64 + (m >> 2)];
    }
#else
    if (active) {
        double2* o = out + (size_t)k * 4;
        o[0] = q0;
        o[1] = q1;
        o[2] = q2;
        o[3] = q3;
    }
#endif
}

__global__ __launch_bounds__(kResolveThreads) void k_resolve_samples(ResolveParams P) {
    const size_t n = P.n_pixels * 3;
    const double inv = 1.0 / (double)P.spp;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t p = i / 3, c = i - 3 * p;
        const double* src = P.rgb + p * (size_t)P.spp * 3 + c;
        double acc = 0.0;
        for (int s = 0; s < P.spp; ++s) acc += src[(size_t)s * 3];
        P.fb[i] = acc * inv;
    }
}

}  // namespace

hipError_t launch_camera_rays(bool jittered, hipStream_t st, const CameraParams& P) {
    const size_t per_row = (size_t)P.W * (jittered ? RT_SPP : 1);
    if (P.W <= 0 || P.n_rows <= 0 || P.n_rows > 65535 || per_row >= ((size_t)1 << 31) || !P.rays) return hipErrorInvalidValue;
    if (jittered && (!P.rows || !P.jrow || !P.jit)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((per_row + kCamThreads - 1) / kCamThreads), (unsigned)P.n_rows);
    if (jittered) {
        rtamd::note_launch(kNsName, "k_camera_rays<true>");
        hipLaunchKernelGGL(k_camera_rays<true>, grid, dim3(kCamThreads), 0, st, P);
    } else {
        rtamd::note_launch(kNsName, "k_camera_rays<false>");
        hipLaunchKernelGGL(k_camera_rays<false>, grid, dim3(kCamThreads), 0, st, P);
    }
    return hipGetLastError();
}

hipError_t launch_resolve_samples(hipStream_t st, const ResolveParams& P) {
    if (!P.n_pixels || P.spp < 1 || !P.rgb || !P.fb) return hipErrorInvalidValue;
    const size_t n = P.n_pixels * 3;
    const unsigned blocks = (unsigned)std::min<size_t>((n + kResolveThreads - 1) / kResolveThreads, 16384);
    rtamd::note_launch(kNsName, "k_resolve_samples");
    hipLaunchKernelGGL(k_resolve_samples, dim3(blocks), dim3(kResolveThreads), 0, st, P);
    return hipGetLastError();
}

}  // namespace RT_NS
