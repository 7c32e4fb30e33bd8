// rt_query_f64.hip — the FP64 ray-query kernels (namespace rtd): Scene::intersect
// / Scene::occluded for batches of caller-given rays (rt_query_intersect /
// rt_query_occluded), on the parity path's device code.
#include "rt_device.hpp"
#include "rt_query_kernels.hpp"
