// rt_query_bvh_f64.hip — the FP64 ray-query kernels on the per-ray BVH
// (namespace rtd): rt_query_intersect / rt_query_occluded with
// RT_FLAG_RAY_BVH, on the parity path's device code.
#include "rt_device.hpp"
#include "rt_query_bvh_kernels.hpp"
