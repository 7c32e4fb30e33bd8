// rt_query_bvh_kernels.hpp — the ray queries on the per-ray BVH
// (RT_FLAG_RAY_BVH), built right after rt_device.hpp in a translation unit of
// its own (rt_query_bvh_f64.hip: RT_NS = rtd), so that every other kernel
// compiles exactly as it did without them.  There is no big-stack and no FP32
// build: the host launches these rows only for rtd variants without eager
// programs (frame_plan.hpp use_ray_bvh) and the flat rows otherwise.
//
//   k_query_isect_bvh: Scene::intersect (scene.cpp:10-24) for a batch of rays
//   k_query_occl_bvh:  Scene::occluded  (scene.cpp:33-42)
//
// The flat kernels (rt_query_kernels.hpp) walk the whole object list and skip
// an object only when no lane of the wave touches its ball; in an incoherent
// batch some lane touches nearly every ball.  Here each lane walks the tree of
// CompiledScene::rnodes (ray_bvh_rules.hpp) on its own: one node index per
// lane, i = touch ? i + 1 : skip[i], no stack - so no runtime-indexed private
// array, no scratch and no LDS.  S is the scene with the wave list
// (make_scene(V, true): S.objs / S.ctab / S.worig are wobjs / wctab / worig).
//
// The rules of the walk:
//  - Node test: ray_bvh_touch (ball_touch in scalar form) on the lane's own
//    segment, [tmin, closest so far] for the closest hit, [tmin, tmax] for
//    occluded; NaN passes.  No wave-wide bundle test.
//  - Closest hit: objects arrive in Morton order, so each is evaluated with the
//    range up to and INCLUDING the closest so far and merged by closest_takes
//    (rt_device.hpp), the merge of scene_intersect_wave<BV>.
//  - Object evaluation: object_hit on anything but a bare leaf holds wave-wide
//    tests and wave-uniform reads (OP_IVL_GROUP's __any, the leaf line masks,
//    exec_full()).  Bare leaves (OBJ_SPHERE / OBJ_HALF / OBJ_POKE) are
//    evaluated per lane, each lane its own object.  Every other candidate goes
//    through a wave-uniform loop at a point where the whole wave has
//    reconverged: one pending object is taken with readlane, all lanes
//    evaluate it as the flat loop does, and only the lanes whose candidate it
//    was keep the result.
//  - Rays whose order matters: the merge is order-independent only while every
//    accepted t is comparable.  If a lane's tmin or tmax is NaN, or an accepted
//    hit has t != t (a NaN or overflowing origin "hits" every sphere, and the
//    reference keeps the last object of its own order), the whole wave takes
//    the flat scene_intersect's result - the same bytes for its ordinary
//    lanes.  Occluded is order-free and needs no such path.
//  - Tail lanes replay the last ray and mask only their stores; every store
//    comes after the last scene read.

#include "ray_bvh_rules.hpp"
#include "rt_kernel_table.hpp"

namespace RT_NS {

using rtamd::RayBvhParams;
using rtamd::SceneView;

namespace {

// x's successor in the order of the reals (x not NaN; +inf stays): the closest
// hit so far becomes the inclusive end of the next object's range
__device__ __forceinline__ double range_incl(double x) {
    if (!(x < __builtin_inf())) return x;
    if (x == 0.0) return __longlong_as_double(1);
    const long long b = __double_as_longlong(x);
    return __longlong_as_double(x > 0.0 ? b + 1 : b - 1);
}

__device__ __forceinline__ bool node_touch(const float4 b, const FRay& fr, float t0, float t1) {
    return rtamd::ray_bvh_touch(b.x, b.y, b.z, b.w, fr.ox, fr.oy, fr.oz, fr.dx, fr.dy, fr.dz, t0, t1);
}
__device__ __forceinline__ float4 obj_ball(const DevObj& ob) { return make_float4(ob.fb[0], ob.fb[1], ob.fb[2], ob.fb[3]); }

// the scene with its flat object list again (P carries it next to the tree)
__device__ __forceinline__ DevScene flat_scene(const DevScene& S, const RayBvhParams& P) {
    DevScene F = S;
    F.objs = P.flat_objs;
    F.ctab = reinterpret_cast<const float4*>(P.flat_ctab);
    F.n_objs = P.n_flat;
    F.worig = nullptr;
    return F;
}

// A lane's closest hit so far and its winner (scene_intersect_wave<BV>'s locals)
struct Closest {
    real t;
    int win, win_orig;
    bool win_tie;
    V3 p;
    real ts;
    int code;
    bool odd;   // an accepted hit's t was NaN: the order of the objects matters
};
// object o of the wave list, hit (ok) at t on the range up to and including C.t
__device__ __forceinline__ void merge_hit(const DevScene& S, Closest& C, bool ok, int o, bool tie, real t, V3 p, real ts,
                                          int code) {
    const int oo = S.worig[o];
    C.odd = C.odd || (ok && t != t);
    if (closest_takes(ok, t, C.t, C.win, oo, C.win_orig, tie, C.win_tie)) {
        C.t = t;
        C.win = o;
        C.win_orig = oo;
        C.win_tie = tie;
        C.p = p;
        C.ts = ts;
        C.code = code;
    }
}

// Scene::intersect on the tree P (see the header).  Every lane of the wave
// must call it: the loops below are wave-uniform.
template <bool DEEP, class CT>
__device__ bool scene_intersect_bvh(const DevScene& S, const RayBvhParams& P, const DRay& r, real tmin, real tmax,
                                    real& t_best, DHit& best, CT& cnt) {
    Closest C;
    C.t = tmax;
    C.win = -1;
    C.win_orig = 0;
    C.win_tie = false;
    C.p = v3(RV(0.0), RV(0.0), RV(0.0));
    C.ts = RV(0.0);
    C.code = 0;
    C.odd = tmin != tmin || tmax != tmax;
    const FRay fr = to_fray(r);
    const float ftmin = (float)tmin;
    // the unbounded objects ahead of the tree: every lane, one object at a time
    for (int o = 0; o < P.n_lead; ++o) {
        const DevObj ob = S.objs[o];
        if (ob.kind == rtamd::OBJ_NEVER) continue;   // (padding)
        real t = RV(0.0), ts = RV(0.0);
        V3 p;
        int code = 0;
        const bool ok = object_hit<false, DEEP>(S, ob, r, tmin, range_incl(C.t), t, p, ts, code, cnt);
        merge_hit(S, C, ok, o, rtamd::accepts_tie(ob), t, p, ts, code);
    }
    int i = 0;
    while (__any(i < P.n_nodes)) {
        int first = 0, count = 0;
        if (i < P.n_nodes) {
            const float4* nd = reinterpret_cast<const float4*>(P.nodes + i);
            const float4 ball = nd[0];
            const int4 link = *reinterpret_cast<const int4*>(nd + 1);   // skip, first, count, pad
            if (node_touch(ball, fr, ftmin, (float)C.t)) {
                first = link.y;
                count = link.z;
                ++i;
            } else {
                i = link.x;
            }
        }
        for (int k = 0; __any(k < count); ++k) {
            const bool has = k < count;
            const int o = has ? first + k : 0;
            const DevObj& ob = S.objs[o];
            const bool cand = has && node_touch(obj_ball(ob), fr, ftmin, (float)C.t);
            const bool bare = !kCsg<CT> || ob.kind <= rtamd::OBJ_POKE;
            if (cand && bare) {   // (a bare leaf accepts t == tmax: accepts_tie)
                real t = RV(0.0);
                const bool ok = leaf_hit_t(&S.nodes[ob.node], r, tmin, range_incl(C.t), t, cnt);
                merge_hit(S, C, ok, o, true, t, ray_at(r, t), t, 0);
            }
            if constexpr (kCsg<CT>) {
                bool pend = cand && !bare;
                for (uint64_t m = __ballot(pend); m; m = __ballot(pend)) {
                    const int ou = __builtin_amdgcn_readlane(o, __builtin_ctzll(m));
                    const DevObj obu = S.objs[ou];
                    const bool mine = pend && o == ou;
                    real t = RV(0.0), ts = RV(0.0);
                    V3 p;
                    int code = 0;
                    const bool ok = object_hit<false, DEEP>(S, obu, r, tmin, range_incl(C.t), t, p, ts, code, cnt);
                    merge_hit(S, C, ok && mine, ou, rtamd::accepts_tie(obu), t, p, ts, code);
                    pend = pend && !mine;
                }
            }
        }
    }
    if (__any(C.odd)) return scene_intersect<false, DEEP>(flat_scene(S, P), r, tmin, tmax, t_best, best, cnt);
    if (C.win < 0) return false;
    resolve_hit<false>(S, C.win, r, tmin, C.p, C.ts, C.code, best, cnt);
    t_best = C.t;
    return true;
}

// Scene::occluded on the tree P.  Every lane of the wave must call it.
template <bool DEEP, class CT>
__device__ bool scene_occluded_bvh(const DevScene& S, const RayBvhParams& P, const DRay& r, real tmin, real tmax,
                                   CT& cnt) {
    bool hit = false;
    if (P.n_lead > 0) {   // the unbounded objects ahead of the tree, as the flat loop takes them
        DevScene L = S;
        L.n_objs = P.n_lead;
        hit = scene_occluded<false, DEEP>(L, r, tmin, tmax, cnt);
    }
    const FRay fr = to_fray(r);
    const float ftmin = (float)tmin, ftmax = (float)tmax;
    int i = 0;
    while (__any(!hit && i < P.n_nodes)) {
        int first = 0, count = 0;
        if (!hit && i < P.n_nodes) {
            const float4* nd = reinterpret_cast<const float4*>(P.nodes + i);
            const float4 ball = nd[0];
            const int4 link = *reinterpret_cast<const int4*>(nd + 1);   // skip, first, count, pad
            if (node_touch(ball, fr, ftmin, ftmax)) {
                first = link.y;
                count = link.z;
                ++i;
            } else {
                i = link.x;
            }
        }
        for (int k = 0; __any(!hit && k < count); ++k) {
            const bool has = !hit && k < count;
            const int o = has ? first + k : 0;
            const DevObj& ob = S.objs[o];
            const bool cand = has && node_touch(obj_ball(ob), fr, ftmin, ftmax);
            const bool bare = !kCsg<CT> || ob.kind <= rtamd::OBJ_POKE;
            if (cand && bare) {
                real t = RV(0.0);
                hit = leaf_hit_t(&S.nodes[ob.node], r, tmin, tmax, t, cnt);
            }
            if constexpr (kCsg<CT>) {
                bool pend = cand && !bare;
                for (uint64_t m = __ballot(pend); m; m = __ballot(pend)) {
                    const int ou = __builtin_amdgcn_readlane(o, __builtin_ctzll(m));
                    const DevObj obu = S.objs[ou];
                    const bool mine = pend && o == ou;
                    real t = RV(0.0), ts = RV(0.0);
                    V3 p;
                    int code = 0;
                    const bool h = object_hit<false, DEEP>(S, obu, r, tmin, tmax, t, p, ts, code, cnt);
                    hit = hit || (h && mine);
                    pend = pend && !mine;
                }
            }
        }
    }
    return hit;
}

// ray i of the batch (lanes past its end: the last ray), as Ray(o, d) (core.h:278)
__device__ __forceinline__ DRay bvh_query_ray(const RayBvhParams& P, size_t i, real& tmin, real& tmax) {
    const rt_ray R = P.rays[i];
    tmin = (real)R.tmin;
    tmax = (real)R.tmax;
    return make_ray(v3((real)R.o[0], (real)R.o[1], (real)R.o[2]), v3((real)R.d[0], (real)R.d[1], (real)R.d[2]));
}

template <bool D, bool PL>
__global__ __launch_bounds__(kQueryThreads) void k_query_isect_bvh(DevScene S, RayBvhParams P) {
    const size_t i0 = (size_t)blockIdx.x * kQueryThreads + threadIdx.x;
    const bool active = i0 < P.n;
    const size_t i = active ? i0 : P.n - 1;
    std::conditional_t<PL, CntPlain, Cnt<false>> cnt;
    cnt.init();
    real tmin, tmax;
    const DRay r = bvh_query_ray(P, i, tmin, tmax);
    real ht = RV(0.0);
    DHit h;
    h.mat = -1;
    h.p = h.n = v3(RV(0.0), RV(0.0), RV(0.0));
    h.ff = 0;
    const bool hit = scene_intersect_bvh<D>(S, P, r, tmin, tmax, ht, h, cnt);
    if (active) {
        rt_hit o;   // (a miss: mat -1, every other field 0)
        o.t = hit ? (double)ht : 0.0;
        o.p[0] = hit ? (double)h.p.x : 0.0;
        o.p[1] = hit ? (double)h.p.y : 0.0;
        o.p[2] = hit ? (double)h.p.z : 0.0;
        o.n[0] = hit ? (double)h.n.x : 0.0;
        o.n[1] = hit ? (double)h.n.y : 0.0;
        o.n[2] = hit ? (double)h.n.z : 0.0;
        o.mat = hit ? h.mat : -1;
        o.front_face = hit ? h.ff : 0;
        P.hits[i] = o;
        if (P.mask) P.mask[i] = hit ? 1 : 0;
    }
}

template <bool D, bool PL>
__global__ __launch_bounds__(kQueryThreads) void k_query_occl_bvh(DevScene S, RayBvhParams P) {
    const size_t i0 = (size_t)blockIdx.x * kQueryThreads + threadIdx.x;
    const bool active = i0 < P.n;
    const size_t i = active ? i0 : P.n - 1;
    std::conditional_t<PL, CntPlain, Cnt<false>> cnt;
    cnt.init();
    real tmin, tmax;
    const DRay r = bvh_query_ray(P, i, tmin, tmax);
    const bool occ = scene_occluded_bvh<D>(S, P, r, tmin, tmax, cnt);
    if (active) P.mask[i] = occ ? 1 : 0;
}

// The ray-BVH kernels by variant, in the tables' one form (rt_kernel_table.hpp).
// Columns: kind (rtamd::kQueryIsect / kQueryOccl) D PL.
constexpr unsigned bkey(int kind, bool d, bool pl) { return (unsigned)kind | (unsigned)d << 1 | (unsigned)pl << 2; }
#define RT_BQRY(kind, d, pl, ...) RT_KERNEL_ROW(bkey(kind, d, pl), __VA_ARGS__)
const KernelRow<DevScene, RayBvhParams> kRayBvhKernels[] = {
    RT_BQRY(0, 1, 0, k_query_isect_bvh<true, false>),
    RT_BQRY(1, 1, 0, k_query_occl_bvh<true, false>),
    RT_BQRY(0, 0, 0, k_query_isect_bvh<false, false>),
    RT_BQRY(1, 0, 0, k_query_occl_bvh<false, false>),
    RT_BQRY(0, 0, 1, k_query_isect_bvh<false, true>),
    RT_BQRY(1, 0, 1, k_query_occl_bvh<false, true>),
};
#undef RT_BQRY

const KernelRow<DevScene, RayBvhParams>* ray_bvh_row(const rtamd::KernelVariant& v, int kind) {
    if (kind != rtamd::kQueryIsect && kind != rtamd::kQueryOccl) return nullptr;
    if (v.ns != rtamd::KernelVariant::kRtd || v.eager) return nullptr;
    return find_kernel(kRayBvhKernels, bkey(kind, v.deep, v.plain));
}

// launch_lanes (rt_kernel_table.hpp) with the wave list for the scene's object
// list and the flat one, which the fallback reads, in the parameters
hipError_t launch_ray_bvh(const rtamd::KernelVariant& v, int kind, dim3, hipStream_t st, const SceneView& V,
                          const RayBvhParams& p0) {
    const KernelRow<DevScene, RayBvhParams>* k = ray_bvh_row(v, kind);
    if (!k) return hipErrorInvalidDeviceFunction;
    const size_t waves = (p0.n + kQueryThreads - 1) / kQueryThreads;
    if (!p0.n || waves > 0x7fffffffu || !p0.nodes || p0.n_nodes <= 0 || !V.wobjs || !V.worig) return hipErrorInvalidValue;
    RayBvhParams p = p0;
    p.flat_objs = V.objs;
    p.flat_ctab = V.ctab;
    p.n_flat = V.n_objs;
    const DevScene S = make_scene(V, /*bv=*/true);
    rtamd::note_launch(kNsName, k->name);
    hipLaunchKernelGGL(k->fn, dim3((unsigned)waves), dim3(kQueryThreads), 0, st, S, p);
    return hipGetLastError();
}
rtamd::KernelEntry ray_bvh_kernel(const rtamd::KernelVariant& v, int kind) { return kernel_entry(ray_bvh_row(v, kind)); }
const char* ray_bvh_row_name(int i) { return row_name(kRayBvhKernels, i); }

}  // namespace

const rtamd::KernelTable<RayBvhParams>& ray_bvh_table() {
    static const rtamd::KernelTable<RayBvhParams> t = {launch_ray_bvh, ray_bvh_kernel, ray_bvh_row_name, kQueryThreads, 0};
    return t;
}

}  // namespace RT_NS
