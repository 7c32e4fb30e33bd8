// rt_shade_big.hip — the shading-query kernel's big-stack build (namespace
// rtdb, general variant only), for the scenes rt_kernels_big.hip renders.
#define RT_REAL double
#define RT_NS rtdb
#define RT_BIG_STACKS 1
#define RT_GENERAL_ONLY 1
#define RT_POW_ANY_X 1   // a caller-given wo need not be unit: pow_spec (rt_device.hpp)
#include "rt_device.hpp"
#include "rt_shade_kernels.hpp"
