// rt_node_f64.hip — the FP64 node-query kernels (namespace rtd):
// Primitive::intersect / Primitive::interval of one node of the scene graph for
// batches of caller-given rays (rt_query_node_intersect / rt_query_node_interval),
// on the parity path's device code.
#include "rt_device.hpp"
#include "rt_node_kernels.hpp"
