// rt_camera.hpp — launch interface of the camera-ray and sample-resolve
// kernels (rt_camera_f64.hip; rt_camera_rays / rt_resolve_samples of rt.h).
// They have no variants chosen by scene, so they are not rows of the
// scene-variant launch tables of rt_launch.hpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt.h"

namespace rtamd {

// Rays of list entries [ri0, ri0 + n_rows) of a frame of W x H: entry ri0 + k,
// column x (and sample s) goes to rays[k*W + x] (centre) or
// rays[(k*W + x)*RT_SPP + s] (jittered).  The camera's own nx x ny enter the
// formulas as in the frames (SceneView::cam_nx / cam_ny).
struct CameraParams {
    double eye[3], P[3], Lx, Ly;
    int cam_nx, cam_ny;
    int W, H;
    int ri0, n_rows;
    const int32_t* rows;   // output row of every list entry; centre rays: null = entry ri is row ri
    const int32_t* jrow;   // jittered: jitter row of every list entry (StdPlan::rows_jrow)
    const double* jit;     // jittered: 16 draws per pixel by jitter row (StdParams::jit)
    rt_ray* rays;
};

// fb[3p + c] = (((0 + rgb[(p*spp + 0)*3 + c]) + rgb[(p*spp + 1)*3 + c]) + ...) * (1.0 / spp)
struct ResolveParams {
    const double* rgb;
    size_t n_pixels;
    int spp;
    double* fb;
};

}  // namespace rtamd

namespace rtd {
// One launch over P.n_rows list entries (0 < n_rows <= 65535, W * RT_SPP < 2^31).
hipError_t launch_camera_rays(bool jittered, hipStream_t st, const rtamd::CameraParams& P);
hipError_t launch_resolve_samples(hipStream_t st, const rtamd::ResolveParams& P);
}  // namespace rtd
