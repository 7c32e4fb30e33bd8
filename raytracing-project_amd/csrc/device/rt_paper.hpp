// rt_paper.hpp — launch interface of the paper-resolve and outgoing-direction
// kernels (rt_paper_f64.hip; rt_paper_resolve / rt_rays_wo of rt.h).  Like
// the camera kernels they have no variants chosen by scene, so they are not
// rows of the scene-variant launch tables of rt_launch.hpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt.h"

namespace rtamd {

// wo[3i .. 3i+2] = normalized(-normalized(rays[i].d)) for i < n
struct RaysWoParams {
    const rt_ray* rays;
    size_t n;
    double* wo;
};

// Output rows [row0, row0 + n_rows) of a W x H paper frame from the records of
// frame rows [in0, in1) = [max(0, row0 - 1), min(H, row0 + n_rows + 1)): pixel
// (x, y) at index (y - in0)*W + x of hits, mask (null: all hits) and rgb (3
// doubles; null only with a null fb).  fb and edge are indexed from row0;
// either may be null.
struct PaperResolveParams {
    const rt_hit* hits;
    const uint8_t* mask;
    const double* rgb;
    int W, H, row0, n_rows;
    double* fb;
    double* edge;
};

}  // namespace rtamd

namespace rtd {
hipError_t launch_rays_wo(hipStream_t st, const rtamd::RaysWoParams& P);
// Any n_rows > 0: split into launches where one grid cannot cover the rows.
hipError_t launch_paper_resolve(hipStream_t st, const rtamd::PaperResolveParams& P);
}  // namespace rtd
