// rt_kernels_f32.hip — the FP32 render kernels (namespace rtf), selected by
// RT_FLAG_FP32: SURVEY.md §8f row 3, the optional non-parity fast path.  The
// algorithm, op order and culling are the FP64 path's; only the arithmetic
// type of the scene records and the trace differs.
#define RT_REAL float
#define RT_NS rtf
#undef RT_FUSED_NORM
#define RT_FUSED_NORM 0   // (the fused sqrt + division is FP64 arithmetic: float keeps sqrt_r + div3)
#undef RT_SPEC_SKIP
#define RT_SPEC_SKIP 0   // (the specular skip's margin is derived for FP64: float keeps today's text)
#define RT_NO_PLAIN   // (no plain kernel variants in the FP32 diagnostic build)
#define RT_NO_PAPER_CODES   // (paper codes are FP64 frames only: no CODES finish kernels)
#include "rt_device.hpp"
#include "rt_kernels.hpp"
