// rt_shade_f64.hip — the FP64 shading-query kernels (namespace rtd):
// shade_lambert_phong for batches of caller-given hits (rt_query_shade), on
// the parity path's device code.
#include "rt_device.hpp"
#include "rt_shade_kernels.hpp"
