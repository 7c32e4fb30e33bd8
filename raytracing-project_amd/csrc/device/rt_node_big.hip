// rt_node_big.hip — the node-query kernels' big-stack build (namespace rtdb,
// program rows only), for nodes whose own programs need more than the common
// stacks (frame_plan.hpp pick_node_variant).
#define RT_REAL double
#define RT_NS rtdb
#define RT_BIG_STACKS 1
#define RT_GENERAL_ONLY 1
#include "rt_device.hpp"
#include "rt_node_kernels.hpp"
