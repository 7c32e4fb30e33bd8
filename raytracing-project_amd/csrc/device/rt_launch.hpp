// rt_launch.hpp — what the host side of librtamd hands to the render kernels.
//
// The kernels exist twice: namespace rtd (FP64, the parity path) and
// namespace rtf (FP32, RT_FLAG_FP32, rt_render_f32.hip).  Both are built from
// rt_device.hpp + rt_kernels.hpp; this header holds the precision-neutral
// launch interface: device pointers, the camera/medium in double, and the
// per-launch parameter blocks.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frame_plan.hpp"
#include "rt.h"
#include "scene_compile.hpp"

namespace rtamd {

// Scene records in a given precision.  The double instances are
// layout-identical to the C-ABI structs of rt.h; the float ones are the
// converted copies the FP32 kernels read.
template <class T>
struct NodeR {
    int32_t kind;
    int32_t a, b;
    int32_t op;
    int32_t mat;
    int32_t mats[5];
    T v[24];
    T aux[4];
};
template <class T>
struct MatR {
    T albedo[3];
    T ambient[3];
    T kd, ks, kr, kt;
    T shininess;
    T refractive_index;
};
template <class T>
struct LightR {
    T pos[3];
    T intensity[3];
};
template <class T>
struct DLightR {
    T dir[3];
    T radiance[3];
};
template <class T>
struct FoldLeafR {   // FoldLeaf (scene_compile.hpp) in the launching precision
    T c[3];
    T r;
    int32_t pc;
    int32_t pad;
};
static_assert(sizeof(FoldLeafR<double>) == sizeof(FoldLeaf), "FoldLeafR<double> must mirror FoldLeaf");
static_assert(sizeof(NodeR<double>) == sizeof(rt_node), "NodeR<double> must mirror rt_node");
static_assert(sizeof(MatR<double>) == sizeof(rt_material), "MatR<double> must mirror rt_material");
static_assert(sizeof(LightR<double>) == sizeof(rt_light), "LightR<double> must mirror rt_light");
static_assert(sizeof(DLightR<double>) == sizeof(rt_dir_light), "DLightR<double> must mirror rt_dir_light");

// Device-resident scene, precision-neutral (records are NodeR/MatR/... of
// the launching precision).
struct SceneView {
    const void* nodes;
    const void* mats;
    const void* lights;
    const void* dlights;
    const DevObj* objs;
    const DevOp* ops;
    const float* gb;
    const float* ctab;   // CompiledScene::ctab
    const float* lrec;   // CompiledScene::lrec / lwrec / lgb: light-relative shadow cull records
    const float* lwrec;
    const float* lgb;
    int n_gb;
    const void* fold;   // FoldLeafR of the launching precision
    // wave BVH (CompiledScene::wobjs, wctab, worig, wchunk); n_chunks = 0: none
    const DevObj* wobjs;
    const float* wctab;
    const int32_t* worig;
    const float* wchunk;
    int n_wobjs, n_chunks;
    int n_lights, n_dlights, n_objs;
    int n_bounded;
    int n_lead;      // CompiledScene::n_lead (0: none / RT_LEAD=0)
    int cam_nx, cam_ny;
    int rec_limit, cull;
    double eye[3], P[3], Lx, Ly;
    double medium_index;
    int bg_mat;   // the background colour: albedo of material slot bg_mat (appended after the scene's)
};

struct StdParams {
    int W, H;
    int n_rows;
    const int32_t* rows;
    const int32_t* jrow;   // jitter row of every listed row
    const double* jit;     // 16 draws per pixel: (dx, dy) of samples 0..7
    double* fb;
    unsigned long long* counters;
};

struct PaperParams {
    int W, H;
    int n_ext;
    int n_rows;
    int n_list;                  // primary pass: ext indices ext_list[0..n_list) of this launch
    const int32_t* ext_list;
    const int32_t* ext_rows;     // rows needing a primary hit
    const int32_t* ext_shade;    // 1 = row is rendered by this call (shade it)
    const int32_t* nbr;          // per rendered row: ext index of r-1, r, r+1 (-1 = outside frame)
    const int32_t* rows;         // rendered rows
    int* mat;                    // [n_ext*W]: primary hit's material (kPaperMiss for none) | crosshatch band << 24
    double* t;
    double* nx;
    double* ny;
    double* nz;
    double* fb;
    uint8_t* code;               // non-null: k_paper_finish writes paper_code bytes [n_rows*W] instead of fb
    unsigned int* gtime;         // non-null: a timed launch; primary waves store (start, end) wall-clock ticks (paper_wave_slot)
    unsigned long long* counters;
};

// A batch of ray queries (rt_query_intersect / rt_query_occluded): ray i of
// rays[0, n) is lane i % 64 of wave i / 64.  Closest hit: hits[i] and, when
// mask is set, mask[i] = 1 / 0; any hit: mask[i] = 1 / 0 (hits unused).
struct QueryParams {
    const rt_ray* rays;
    size_t n;
    rt_hit* hits;
    uint8_t* mask;
};
enum { kQueryIsect = 0, kQueryOccl = 1, kQueryRadiance = 2 };   // query kinds (k_query_isect / k_query_occl / k_radiance)

// A batch of radiance queries (rt_query_radiance): ray i of rays[0, n) is lane
// i % 64 of wave i / 64, rgb[3i .. 3i + 2] its colour (Tracer::trace); tmin /
// tmax of the rays are not read.  counters: the frames' kCounterSlots x
// kCounterWords slots (words 0, 1: the Scene::intersect / Scene::occluded calls).
struct RadianceParams {
    const rt_ray* rays;
    size_t n;
    double* rgb;
    unsigned long long* counters;
};

// A batch of shading queries (rt_query_shade): entry i of hits[0, n) / wo[3i ..
// 3i + 2] is lane i % 64 of wave i / 64, rgb[3i .. 3i + 2] its colour
// (shade_lambert_phong).  mask (may be null): entries with mask[i] == 0 are not
// read and get `miss`.  The call's point lights are SceneView::lights /
// n_lights of the launch.  counters: the frames' slots (word 1: the
// Scene::occluded calls).
struct ShadeParams {
    const rt_hit* hits;
    const double* wo;
    const uint8_t* mask;
    size_t n;
    double* rgb;
    double miss[3];
    unsigned long long* counters;
};

// Paper mode's output alphabet (tracer.cpp:258-281): every pixel is grey
// (r = g = b) and a function of the edge strength - the max of the constants
// {0.9, 0.6, 0.5, 0.3} over the neighbour tests, or 0, halved when a
// neighbour lies outside the frame (tracer.cpp:133-178) - and of the hatch
// bit apply_crosshatch returns (tracer.cpp:188-205).  So one byte holds a
// pixel exactly: bits 0-2 the index of the max in {0, 0.3, 0.5, 0.6, 0.9},
// bit 3 the halving, bit 4 the hatch bit (white).  The distributed frame
// gathers these bytes (1 B/px instead of 24) and the root decodes them with
// the reference's own FP64 expression, bit for bit.
__host__ __device__ inline double paper_code_value(unsigned code) {
    const unsigned i = code & 7;
    double edge = i == 1 ? 0.3 : i == 2 ? 0.5 : i == 3 ? 0.6 : i == 4 ? 0.9 : 0.0;
    if (code & 8) edge *= 0.5;
    if (edge > 0.8) return 0.0;
    if (edge > 0.5) return 0.2;
    double o = (code & 16) ? 1.0 : 0.0;
    if (edge > 0.3) {
        const double darken = (edge - 0.3) * 0.4;
        o *= (1.0 - darken);
    }
    return o;
}

constexpr int kCounterWords = 2 + 16;   // isect, occl, ops[16]
constexpr int kCounterSlots = 512;      // spread of the per-block counter atomics

// A trace kernel (its host handle) and its name as rocprofv3 prints it,
// without the namespace (e.g. "k_std_lean<false, 1, false>")
struct KernelEntry {
    const void* fn;
    const char* name;
};

// The launch log (rt_test.h rt_test_launch_log; defined in rt_test_hooks.hip):
// every launcher below reports the row it launches, "ns::name".  While the
// log is off this is one relaxed atomic load.
void note_launch(const char* ns, const char* name);

}  // namespace rtamd

// The trace kernels of one namespace (rt_kernels.hpp), by KernelVariant
// (frame_plan.hpp).  launch_*: hipErrorInvalidDeviceFunction when the
// namespace has no kernel for the variant.  launch_query / query_kernel: the
// ray-query kernels (rt_query_kernels.hpp, their own translation units; rtf
// has none).  launch_radiance / radiance_kernel: the radiance-query kernels
// (rt_radiance_kernels.hpp, likewise; rtd and rtdb only, rtf defines none).
// launch_shade / shade_kernel: the shading-query kernels (rt_shade_kernels.hpp,
// likewise).  *_row_name(i): row i of the namespace's table, nullptr past its
// end (rt_test_kernel_row, rt_test_radiance_kernel_row, rt_test_shade_kernel_row).
#define RT_DECLARE_LAUNCHERS(NS)                                                                                  \
    namespace NS {                                                                                                \
    hipError_t launch_std(const rtamd::KernelVariant& v, hipStream_t st, const rtamd::SceneView& V,               \
                          const rtamd::StdParams& P);                                                             \
    hipError_t launch_paper(const rtamd::KernelVariant& v, dim3 grid, hipStream_t st, const rtamd::SceneView& V,  \
                            const rtamd::PaperParams& P);                                                         \
    hipError_t launch_paper_finish(dim3 grid, hipStream_t st, const rtamd::PaperParams& P);                       \
    rtamd::KernelEntry std_kernel(const rtamd::KernelVariant& v);                                                 \
    rtamd::KernelEntry paper_kernel(const rtamd::KernelVariant& v);                                               \
    int kernel_block_threads(bool paper);                                                                         \
    size_t kernel_pool_bytes(bool paper);                                                                         \
    hipError_t launch_query(const rtamd::KernelVariant& v, int kind, hipStream_t st, const rtamd::SceneView& V,   \
                            const rtamd::QueryParams& P);                                                         \
    rtamd::KernelEntry query_kernel(const rtamd::KernelVariant& v, int kind);                                     \
    const char* std_row_name(int i);                                                                              \
    const char* paper_row_name(int i);                                                                            \
    const char* finish_row_name(int i);                                                                           \
    const char* query_row_name(int i);                                                                            \
    hipError_t launch_radiance(const rtamd::KernelVariant& v, hipStream_t st, const rtamd::SceneView& V,          \
                               const rtamd::RadianceParams& P);                                                   \
    rtamd::KernelEntry radiance_kernel(const rtamd::KernelVariant& v);                                            \
    const char* radiance_row_name(int i);                                                                         \
    hipError_t launch_shade(const rtamd::KernelVariant& v, hipStream_t st, const rtamd::SceneView& V,             \
                            const rtamd::ShadeParams& P);                                                         \
    rtamd::KernelEntry shade_kernel(const rtamd::KernelVariant& v);                                               \
    const char* shade_row_name(int i);                                                                            \
    }
RT_DECLARE_LAUNCHERS(rtd)
RT_DECLARE_LAUNCHERS(rtf)
RT_DECLARE_LAUNCHERS(rtdb)

// The launchers of a variant's namespace (the big-stack build has no finish
// pass of its own: k_paper_finish reads records only).
namespace rtamd {
inline hipError_t launch_std(const KernelVariant& v, hipStream_t st, const SceneView& V, const StdParams& P) {
    return v.ns == KernelVariant::kRtf ? rtf::launch_std(v, st, V, P)
                                       : v.ns == KernelVariant::kRtdb ? rtdb::launch_std(v, st, V, P) : rtd::launch_std(v, st, V, P);
}
inline hipError_t launch_paper(const KernelVariant& v, dim3 grid, hipStream_t st, const SceneView& V,
                               const PaperParams& P) {
    return v.ns == KernelVariant::kRtf ? rtf::launch_paper(v, grid, st, V, P)
                                       : v.ns == KernelVariant::kRtdb ? rtdb::launch_paper(v, grid, st, V, P)
                                                                      : rtd::launch_paper(v, grid, st, V, P);
}
inline hipError_t launch_paper_finish(const KernelVariant& v, dim3 grid, hipStream_t st, const PaperParams& P) {
    return v.ns == KernelVariant::kRtf ? rtf::launch_paper_finish(grid, st, P) : rtd::launch_paper_finish(grid, st, P);
}
// The variant's trace kernel of `mode` ({nullptr, nullptr}: none), and its launch shape
inline KernelEntry trace_kernel(const KernelVariant& v, bool paper) {
    if (v.ns == KernelVariant::kRtf) return paper ? rtf::paper_kernel(v) : rtf::std_kernel(v);
    if (v.ns == KernelVariant::kRtdb) return paper ? rtdb::paper_kernel(v) : rtdb::std_kernel(v);
    return paper ? rtd::paper_kernel(v) : rtd::std_kernel(v);
}
inline hipError_t launch_query(const KernelVariant& v, int kind, hipStream_t st, const SceneView& V,
                               const QueryParams& P) {
    return v.ns == KernelVariant::kRtf ? rtf::launch_query(v, kind, st, V, P)
                                       : v.ns == KernelVariant::kRtdb ? rtdb::launch_query(v, kind, st, V, P)
                                                                      : rtd::launch_query(v, kind, st, V, P);
}
inline KernelEntry query_kernel(const KernelVariant& v, int kind) {
    return v.ns == KernelVariant::kRtf ? rtf::query_kernel(v, kind)
                                       : v.ns == KernelVariant::kRtdb ? rtdb::query_kernel(v, kind) : rtd::query_kernel(v, kind);
}
// (pick_radiance_variant never picks rtf: no FP32 radiance queries)
inline hipError_t launch_radiance(const KernelVariant& v, hipStream_t st, const SceneView& V, const RadianceParams& P) {
    return v.ns == KernelVariant::kRtf ? hipErrorInvalidDeviceFunction
                                       : v.ns == KernelVariant::kRtdb ? rtdb::launch_radiance(v, st, V, P)
                                                                      : rtd::launch_radiance(v, st, V, P);
}
inline KernelEntry radiance_kernel(const KernelVariant& v) {
    return v.ns == KernelVariant::kRtf ? KernelEntry{nullptr, nullptr}
                                       : v.ns == KernelVariant::kRtdb ? rtdb::radiance_kernel(v) : rtd::radiance_kernel(v);
}
// (pick_shade_variant never picks rtf: no FP32 shading queries)
inline hipError_t launch_shade(const KernelVariant& v, hipStream_t st, const SceneView& V, const ShadeParams& P) {
    return v.ns == KernelVariant::kRtf ? hipErrorInvalidDeviceFunction
                                       : v.ns == KernelVariant::kRtdb ? rtdb::launch_shade(v, st, V, P)
                                                                      : rtd::launch_shade(v, st, V, P);
}
inline KernelEntry shade_kernel(const KernelVariant& v) {
    return v.ns == KernelVariant::kRtf ? KernelEntry{nullptr, nullptr}
                                       : v.ns == KernelVariant::kRtdb ? rtdb::shade_kernel(v) : rtd::shade_kernel(v);
}
inline int trace_block_threads(const KernelVariant& v, bool paper) {
    return v.ns == KernelVariant::kRtf ? rtf::kernel_block_threads(paper)
                                       : v.ns == KernelVariant::kRtdb ? rtdb::kernel_block_threads(paper)
                                                                      : rtd::kernel_block_threads(paper);
}
inline size_t trace_pool_bytes(const KernelVariant& v, bool paper) {
    return v.ns == KernelVariant::kRtf ? rtf::kernel_pool_bytes(paper)
                                       : v.ns == KernelVariant::kRtdb ? rtdb::kernel_pool_bytes(paper)
                                                                      : rtd::kernel_pool_bytes(paper);
}
}  // namespace rtamd
