// rt_shade_f64.hip — the FP64 shading-query kernels (namespace rtd):
// shade_lambert_phong for batches of caller-given hits (rt_query_shade), on
// the parity path's device code.
#define RT_POW_ANY_X 1   // a caller-given wo need not be unit: pow_spec (rt_device.hpp)
#include "rt_device.hpp"
#include "rt_shade_kernels.hpp"
