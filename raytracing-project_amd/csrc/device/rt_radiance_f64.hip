// rt_radiance_f64.hip — the FP64 radiance-query kernels (namespace rtd):
// Tracer::trace for batches of caller-given rays (rt_query_radiance), on the
// parity path's device code.
#include "rt_device.hpp"
#include "rt_radiance_kernels.hpp"
