// rt_launch.hpp — what the host side of librtamd hands to the render kernels.
//
// The kernels exist per namespace: rtd (FP64, the parity path), rtf (FP32,
// RT_FLAG_FP32, rt_kernels_f32.hip) and rtdb (FP64 with the big stacks, *_big.hip).
// All are built from rt_device.hpp + one kernel header; this header holds the
// precision-neutral launch interface: device pointers, the camera/medium in
// double, the per-launch parameter blocks, and - at its end - the kernel
// tables as the host sees them (KernelTable) with the one mapping from a
// KernelVariant's ns to a namespace (kernel_namespace).
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

// The same batch on the per-ray BVH (RT_FLAG_RAY_BVH, rt_query_bvh_kernels.hpp):
// the tree's nodes[0, n_nodes) over wobjs[n_lead, n_wobjs) (CompiledScene::rnodes
// / rlead), resident next to the scene.  The launcher fills in the flat object
// list (SceneView::objs / ctab / n_objs), which the kernels' fallback walks.
struct RayBvhParams {
    const rt_ray* rays;
    size_t n;
    rt_hit* hits;
    uint8_t* mask;
    const RayBvhNode* nodes;
    int n_nodes, n_lead;
    const DevObj* flat_objs;
    const float* flat_ctab;
    int n_flat;
};

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

// A batch of node queries (rt_query_node_intersect / rt_query_node_interval):
// ray i of rays[0, n) is lane i % 64 of wave i / 64, queried against ONE node
// of the scene graph.  A leaf row reads the leaf `node`; a program row runs
// ops[0, n_ops) (compile_node_program: a buffer of its own, not the scene's
// SceneView::ops).  Intersect: enter[i] the hit, mask[i] (may be null) 1 / 0;
// interval: enter[i] / exit[i] (either may be null) the enterHit / exitHit with
// t = tEnter / tExit, mask[i] (may be null) interval()'s return value.
struct NodeParams {
    const rt_ray* rays;
    size_t n;
    rt_hit* enter;
    rt_hit* exit;
    uint8_t* mask;
    const DevOp* ops;
    int n_ops;
    int node;
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
    // (every product and difference rounded once, as the reference's: the FP32 kernels' unit contracts, and
    // fused 1 - 0.2 * 0.4 into 0.92 where the reference has 0.9199999999999999; that unit is compiled with
    // -ffp-contract=fast-honor-pragmas, since plain fast fuses whatever this pragma says)
#pragma clang fp contract(off)
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
// every launcher reports the row it launches, "ns::name".  While the log is
// off this is one relaxed atomic load.
void note_launch(const char* ns, const char* name);

// One kernel table of one namespace as the host sees it (the rows: rt_kernels.hpp,
// rt_query_kernels.hpp, rt_radiance_kernels.hpp, rt_shade_kernels.hpp, rt_node_kernels.hpp, each in
// the form of rt_kernel_table.hpp and in translation units of its own).
// kind: the query table's rtamd::kQueryIsect / kQueryOccl; grid: the paper
// tables' (the host's 16x16-pixel units; the finish pass's x extent); a table
// without such a column ignores the argument.
template <class P>
struct KernelTable {
    // hipErrorInvalidDeviceFunction: the table has no row for the variant
    hipError_t (*launch)(const KernelVariant& v, int kind, dim3 grid, hipStream_t st, const SceneView& V, const P& p);
    KernelEntry (*kernel)(const KernelVariant& v, int kind);   // what launch picks; {nullptr, nullptr}: no row
    const char* (*row_name)(int i);                            // row i as written, nullptr past the end
    int block_threads;                                         // its launches' workgroup size
    size_t pool_bytes;                                         //   and dynamic LDS
};

// The tables of one namespace.  nullptr: the namespace lacks the family.
struct KernelNamespace {
    const char* name;
    const KernelTable<StdParams>* std;
    const KernelTable<PaperParams>*paper, *finish;
    const KernelTable<QueryParams>* query;
    const KernelTable<RadianceParams>* radiance;
    const KernelTable<ShadeParams>* shade;
    const KernelTable<NodeParams>* node;   // kind: kNodeIsect / kNodeIvl (scene_compile.hpp)
};

}  // namespace rtamd

// Each namespace's tables, defined next to their rows (functions: a const
// object with these initialisers would be emitted into the device code too)
#define RT_DECLARE_TABLES(NS)                                          \
    namespace NS {                                                     \
    const rtamd::KernelTable<rtamd::StdParams>& std_table();           \
    const rtamd::KernelTable<rtamd::PaperParams>& paper_table();       \
    const rtamd::KernelTable<rtamd::PaperParams>& finish_table();      \
    const rtamd::KernelTable<rtamd::QueryParams>& query_table();       \
    const rtamd::KernelTable<rtamd::RadianceParams>& radiance_table(); \
    const rtamd::KernelTable<rtamd::ShadeParams>& shade_table();       \
    const rtamd::KernelTable<rtamd::NodeParams>& node_table();         \
    }
RT_DECLARE_TABLES(rtd)
RT_DECLARE_TABLES(rtf)    // (defines the frame tables only)
RT_DECLARE_TABLES(rtdb)
#undef RT_DECLARE_TABLES
// The ray-BVH query kernels (rt_query_bvh_kernels.hpp): rtd only.  kind: kQueryIsect / kQueryOccl
namespace rtd {
const rtamd::KernelTable<rtamd::RayBvhParams>& ray_bvh_table();
}

namespace rtamd {
// KernelVariant::ns -> its namespace: the one place that choice is written.
// rtf has no query, radiance, shade or node kernels (no FP32 build of them: the
// pick_*_variant of those families never pick it); the big-stack build has no
// finish pass of its own (k_paper_finish reads records only): rtd's.
inline const KernelNamespace& kernel_namespace(int ns) {
    static const KernelNamespace k[] = {
        {"rtd", &rtd::std_table(), &rtd::paper_table(), &rtd::finish_table(), &rtd::query_table(),
         &rtd::radiance_table(), &rtd::shade_table(), &rtd::node_table()},
        {"rtf", &rtf::std_table(), &rtf::paper_table(), &rtf::finish_table(), nullptr, nullptr, nullptr, nullptr},
        {"rtdb", &rtdb::std_table(), &rtdb::paper_table(), &rtd::finish_table(), &rtdb::query_table(),
         &rtdb::radiance_table(), &rtdb::shade_table(), &rtdb::node_table()}};
    static_assert(KernelVariant::kRtd == 0 && KernelVariant::kRtf == 1 && KernelVariant::kRtdb == 2, "k's order");
    return k[ns == KernelVariant::kRtf || ns == KernelVariant::kRtdb ? ns : KernelVariant::kRtd];
}

// A launch / the kernel of a variant in table t; a family the namespace lacks
// answers as a table without the row does.
template <class P>
hipError_t launch_in(const KernelTable<P>* t, const KernelVariant& v, int kind, dim3 grid, hipStream_t st,
                     const SceneView& V, const P& p) {
    return t ? t->launch(v, kind, grid, st, V, p) : hipErrorInvalidDeviceFunction;
}
template <class P>
KernelEntry kernel_in(const KernelTable<P>* t, const KernelVariant& v, int kind = 0) {
    return t ? t->kernel(v, kind) : KernelEntry{nullptr, nullptr};
}

// The launchers of a variant's namespace
inline hipError_t launch_std(const KernelVariant& v, hipStream_t st, const SceneView& V, const StdParams& P) {
    return launch_in(kernel_namespace(v.ns).std, v, 0, dim3(), st, V, P);
}
inline hipError_t launch_paper(const KernelVariant& v, dim3 grid, hipStream_t st, const SceneView& V,
                               const PaperParams& P) {
    return launch_in(kernel_namespace(v.ns).paper, v, 0, grid, st, V, P);
}
inline hipError_t launch_paper_finish(const KernelVariant& v, dim3 grid, hipStream_t st, const SceneView& V,
                                      const PaperParams& P) {
    return launch_in(kernel_namespace(v.ns).finish, v, 0, grid, st, V, P);
}
inline hipError_t launch_query(const KernelVariant& v, int kind, hipStream_t st, const SceneView& V,
                               const QueryParams& P) {
    return launch_in(kernel_namespace(v.ns).query, v, kind, dim3(), st, V, P);
}
// (a variant outside rtd has no row there: hipErrorInvalidDeviceFunction)
inline hipError_t launch_ray_bvh(const KernelVariant& v, int kind, hipStream_t st, const SceneView& V,
                                 const RayBvhParams& P) {
    return launch_in(&rtd::ray_bvh_table(), v, kind, dim3(), st, V, P);
}
inline hipError_t launch_radiance(const KernelVariant& v, hipStream_t st, const SceneView& V, const RadianceParams& P) {
    return launch_in(kernel_namespace(v.ns).radiance, v, 0, dim3(), st, V, P);
}
inline hipError_t launch_shade(const KernelVariant& v, hipStream_t st, const SceneView& V, const ShadeParams& P) {
    return launch_in(kernel_namespace(v.ns).shade, v, 0, dim3(), st, V, P);
}
inline hipError_t launch_node(const KernelVariant& v, int kind, hipStream_t st, const SceneView& V, const NodeParams& P) {
    return launch_in(kernel_namespace(v.ns).node, v, kind, dim3(), st, V, P);
}
// The variant's trace kernel of `mode` ({nullptr, nullptr}: none), and its launch shape
inline KernelEntry trace_kernel(const KernelVariant& v, bool paper) {
    const KernelNamespace& n = kernel_namespace(v.ns);
    return paper ? kernel_in(n.paper, v) : kernel_in(n.std, v);
}
inline int trace_block_threads(const KernelVariant& v, bool paper) {
    const KernelNamespace& n = kernel_namespace(v.ns);
    return paper ? n.paper->block_threads : n.std->block_threads;
}
inline size_t trace_pool_bytes(const KernelVariant& v, bool paper) {
    const KernelNamespace& n = kernel_namespace(v.ns);
    return paper ? n.paper->pool_bytes : n.std->pool_bytes;
}
}  // namespace rtamd
