// rt_bounce.hpp — launch interface of the bounce-loop kernels
// (rt_bounce_f64.hip; rt_scatter_rays / rt_combine_bounce of rt.h).  Like the
// camera and paper-resolve kernels they have no variants chosen by scene, so
// they are not rows of the scene-variant launch tables of rt_launch.hpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt.h"

namespace rtamd {

// Parents of one workgroup of the scatter kernels, and counts of one tile of
// the scan.  The scan's first level is one workgroup over kScatterTile
// workgroup counts, so up to kScatterTile * kScatterThreads parents need one
// level; one parent more takes the second.
constexpr int kScatterThreads = 256;
constexpr int kScatterTile = 256;

// One launch group of rt_scatter_rays_device: parents [0, n) of the group
// (n <= 2^30), whose children start at child index `base` of the call.
struct ScatterParams {
    const rt_ray* rays;
    const rt_hit* hits;
    const uint8_t* mask;   // null: every entry is a hit
    size_t n;
    const void* mats;      // MatR<double>[n_mats], the resident scene's
    int n_mats;
    int can;               // depth < recursion_limit - 1
    double medium_index;
    uint8_t* spawn;
    uint64_t* first;
    rt_ray* child_rays;
    double* child_w;
    uint64_t child_cap;    // of the call: a child index >= child_cap is not written
    uint64_t base;
    // scratch of the group: counts[0, levels' sizes back to back) and the
    // group's child total
    uint32_t* counts;
    uint64_t* total;
};
// uint32 words of ScatterParams::counts for n parents
size_t scatter_count_words(size_t n);

// rgb[3i ..] <- combine(rgb[3i ..], child_rgb[j] * child_w[j]) over parent i's children
struct CombineParams {
    double* rgb;
    const uint8_t* spawn;
    const uint64_t* first;
    size_t n;
    const double* child_rgb;
    const double* child_w;
    uint64_t n_children;
};

}  // namespace rtamd

namespace rtd {
// count + scan + emit of one group, enqueued on st; *P.total holds the group's
// children once st has run
hipError_t launch_scatter(hipStream_t st, const rtamd::ScatterParams& P);
hipError_t launch_combine_bounce(hipStream_t st, const rtamd::CombineParams& P);
}  // namespace rtd
