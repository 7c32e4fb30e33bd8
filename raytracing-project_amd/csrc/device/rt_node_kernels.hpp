// rt_node_kernels.hpp — the batched node-query kernels, built right after
// rt_device.hpp in translation units of their own (rt_node_f64.hip: RT_NS =
// rtd; rt_node_big.hip: RT_NS = rtdb, the big-stack build), so that every
// other kernel compiles exactly as it did without them.  There is no FP32 build.
//
//   k_node_isect: Primitive::intersect(node, ray, tmin, tmax) (geometry.h:62-68)
//   k_node_ivl:   Primitive::interval(node, ray)              (geometry.h:70-75)
//
// for a batch of rays against ONE node of the scene graph: the virtual pair
// every sphere, half-space, pokeball, transform and CSG node overrides, which
// the trace kernels evaluate inside their object loops.  The scene's other
// objects, its lights and its camera play no part, and there is no cull.
//
// PROG = false: the node is a leaf, evaluated by leaf_intersect / leaf_interval
// (no interpreter, no stacks).  PROG = true: the node's own post-order program
// (scene_compile.hpp compile_node_program): the intersect program runs through
// run_program, the interpreter of the frames' eager objects, as it stands;
// run_program returns only the intersect-mode hit, so the interval program
// runs through run_interval below, the same loop restricted to the interval
// ops and built from the same pieces (IStack, local_ray, leaf_interval,
// csg_interval, map_point, map_normal, project_t_world, set_face_normal),
// whose result is the stack's top after the last op.  Every lane of every wave
// runs the same ops, so op fetches and node reads are scalar loads and control
// flow is wave-uniform.  The host launches a program only in a namespace whose stacks
// hold it (frame_plan.hpp pick_node_variant).
//
// One ray per lane, one-wave workgroups; lanes past the batch's end take the
// last ray again and only their stores are masked; every store comes after
// the last scene read; no LDS, no counters (rt_query_kernels.hpp).
//
// The interval records: t is tEnter / tExit, the call's out-parameters (DHit
// carries no t: under a transform the reference records' own Hit::t keeps a
// local value nothing reads); p, n, mat, front_face are enterHit / exitHit.

#include "rt_kernel_table.hpp"

namespace RT_NS {

using rtamd::NodeParams;
using rtamd::SceneView;

namespace {

__device__ __forceinline__ DRay node_ray(const NodeParams& P, size_t i, real& tmin, real& tmax) {
    const rt_ray R = P.rays[i];
    tmin = (real)R.tmin;
    tmax = (real)R.tmax;
    return make_ray(v3((real)R.o[0], (real)R.o[1], (real)R.o[2]), v3((real)R.d[0], (real)R.d[1], (real)R.d[2]));
}

// (not ok: mat -1, every other field 0)
__device__ __forceinline__ rt_hit node_record(bool ok, real t, const DHit& h) {
    rt_hit o;
    o.t = ok ? (double)t : 0.0;
    o.p[0] = ok ? (double)h.p.x : 0.0;
    o.p[1] = ok ? (double)h.p.y : 0.0;
    o.p[2] = ok ? (double)h.p.z : 0.0;
    o.n[0] = ok ? (double)h.n.x : 0.0;
    o.n[1] = ok ? (double)h.n.y : 0.0;
    o.n[2] = ok ? (double)h.n.z : 0.0;
    o.mat = ok ? h.mat : -1;
    o.front_face = ok ? h.ff : 0;
    return o;
}

// the scene with the node's program as its op table (run_program reads S.ops)
__device__ __forceinline__ DevScene program_scene(const DevScene& S, const NodeParams& P) {
    DevScene T = S;
    T.ops = P.ops;
    return T;
}

// Primitive::interval(root, ray) of an interval program (compile_node_program,
// kNodeIvl): run_program's loop over the ops emit_ivl emits.
template <class CT>
__device__ __forceinline__ void run_interval(const DevScene& S, const DevOp* ops, int n_ops, const DRay& world, Ivl& out,
                                             CT& cnt) {
    DRay cur = world;
    DRay rstk[kMaxRayStack];
    int rsp = 0;
    IStack st;
    st.sp = 0;
    st.tos.ok = 0;
    for (int pc = 0; pc < n_ops; ++pc) {
        const DevOp op = ops[pc];
        const NodeT* nd = &S.nodes[op.node];
        switch (op.op) {
            case rtamd::OP_XPUSH:
                cnt.inc(RT_OPC_XFORM);
                rstk[rsp++] = cur;
                cur = local_ray(nd, cur);
                break;
            case rtamd::OP_LEAF_IVL: {
                Ivl v;
                leaf_interval(nd, cur, v, cnt);
                st.push(v);
                break;
            }
            case rtamd::OP_CSG: {
                Ivl r;
                csg_interval(op.csg_op, st.nos, st.tos, cur, r, cnt);
                st.reduce2(r);
                break;
            }
            case rtamd::OP_XPOP_IVL: {
                const DRay parent = rstk[--rsp];
                Ivl& v = st.tos;
                if (v.ok) {   // transform.cpp:55-82 (138-169, 224-255)
                    v.h0.p = map_point(nd, v.h0.p);
                    v.h1.p = map_point(nd, v.h1.p);
                    const V3 nE = map_normal(nd, v.h0.n);
                    const V3 nX = map_normal(nd, v.h1.n);
                    set_face_normal(v.h0, parent, nE);
                    set_face_normal(v.h1, parent, nX);
                    v.t0 = project_t_world(parent, v.h0.p);
                    v.t1 = project_t_world(parent, v.h1.p);
                }
                cur = parent;
                break;
            }
            default: {   // OP_NEVER, top = 2: a degenerate Scaling's interval is false (transform.cpp:97)
                Ivl v;
                v.ok = 0;
                st.push(v);
                break;
            }
        }
    }
    out = st.tos;
}

template <bool PROG>
__global__ __launch_bounds__(kQueryThreads) void k_node_isect(DevScene S, NodeParams P) {
    const size_t i0 = (size_t)blockIdx.x * kQueryThreads + threadIdx.x;
    const bool active = i0 < P.n;
    const size_t i = active ? i0 : P.n - 1;
    Cnt<false> cnt;
    cnt.init();
    real tmin, tmax;
    const DRay r = node_ray(P, i, tmin, tmax);
    real ht = RV(0.0);
    DHit h;
    h.mat = -1;
    h.p = h.n = v3(RV(0.0), RV(0.0), RV(0.0));
    h.ff = 0;
    bool hit;
    if constexpr (PROG) hit = run_program<true>(program_scene(S, P), 0, P.n_ops, r, tmin, tmax, ht, h, cnt);
    else hit = leaf_intersect(&S.nodes[P.node], r, tmin, tmax, ht, h, cnt);
    if (active) {
        P.enter[i] = node_record(hit, ht, h);
        if (P.mask) P.mask[i] = hit ? 1 : 0;
    }
}

template <bool PROG>
__global__ __launch_bounds__(kQueryThreads) void k_node_ivl(DevScene S, NodeParams P) {
    const size_t i0 = (size_t)blockIdx.x * kQueryThreads + threadIdx.x;
    const bool active = i0 < P.n;
    const size_t i = active ? i0 : P.n - 1;
    Cnt<false> cnt;
    cnt.init();
    real tmin, tmax;   // (not read: interval has no range)
    const DRay r = node_ray(P, i, tmin, tmax);
    Ivl v;
    v.ok = 0;
    if constexpr (PROG) {
        run_interval(S, P.ops, P.n_ops, r, v, cnt);
    } else {
        leaf_interval(&S.nodes[P.node], r, v, cnt);
    }
    if (active) {
        const bool ok = v.ok != 0;
        if (P.enter) P.enter[i] = node_record(ok, v.t0, v.h0);
        if (P.exit) P.exit[i] = node_record(ok, v.t1, v.h1);
        if (P.mask) P.mask[i] = ok ? 1 : 0;
    }
}

// The node kernels, in the tables' one form (rt_kernel_table.hpp).  Columns:
// kind (rtamd::kNodeIsect / kNodeIvl) PROG.  RT_GENERAL_ONLY (the big-stack
// build) keeps the program rows: a leaf has no stacks.
constexpr unsigned nkey(int kind, bool prog) { return (unsigned)kind | (unsigned)prog << 1; }
#define RT_NODE(kind, prog, ...) RT_KERNEL_ROW(nkey(kind, prog), __VA_ARGS__)
const KernelRow<DevScene, NodeParams> kNodeKernels[] = {
    RT_NODE(0, 1, k_node_isect<true>),
    RT_NODE(1, 1, k_node_ivl<true>),
#ifndef RT_GENERAL_ONLY
    RT_NODE(0, 0, k_node_isect<false>),
    RT_NODE(1, 0, k_node_ivl<false>),
#endif
};
#undef RT_NODE

const KernelRow<DevScene, NodeParams>* node_row(const rtamd::KernelVariant& v, int kind) {
    if (kind != rtamd::kNodeIsect && kind != rtamd::kNodeIvl) return nullptr;
    return find_kernel(kNodeKernels, nkey(kind, v.eager));
}

hipError_t launch_node(const rtamd::KernelVariant& v, int kind, dim3, hipStream_t st, const SceneView& V,
                       const NodeParams& P) {
    return launch_lanes(node_row(v, kind), 0, false, st, V, P);
}
rtamd::KernelEntry node_kernel(const rtamd::KernelVariant& v, int kind) { return kernel_entry(node_row(v, kind)); }
const char* node_row_name(int i) { return row_name(kNodeKernels, i); }

}  // namespace

const rtamd::KernelTable<NodeParams>& node_table() {
    static const rtamd::KernelTable<NodeParams> t = {launch_node, node_kernel, node_row_name, kQueryThreads, 0};
    return t;
}

}  // namespace RT_NS
