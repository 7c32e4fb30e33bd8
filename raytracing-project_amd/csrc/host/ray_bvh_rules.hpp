// ray_bvh_rules.hpp — the per-ray BVH's node record and its node test, shared
// by the host (scene_compile.cpp: the builder and the host restatement of the
// walk) and the device (rt_query_bvh_kernels.hpp), as paper_rules.hpp is.
//
// The tree (CompiledScene::rnodes) lies over the bounded part of the wave list
// (CompiledScene::wobjs, Morton order), nodes in depth-first pre-order.  A
// ray's walk keeps one index and no stack:
//
//     i = 0;  while (i < n_nodes)  i = touch(node i) ? i + 1 : node[i].skip;
//
// and evaluates objects [first, first + count) of every leaf it touches.
#pragma once

#include <cmath>
#include <cstdint>

#ifdef __HIP__
#define RT_RULE_FN __host__ __device__ inline
#else
#define RT_RULE_FN inline
#endif

namespace rtamd {

struct RayBvhNode {
    float c[4];      // the ball (cx, cy, cz, r): contains the f32 ball DevObj::fb of every object below the node
    int32_t skip;    // the next node when this subtree is culled (n_nodes: the walk ends)
    int32_t first;   // a leaf's objects: wobjs[first, first + count); an inner node has count 0
    int32_t count;
    int32_t pad;
};
static_assert(sizeof(RayBvhNode) == 32, "two 16-byte loads per node");

constexpr int kRayBvhLeaf = 4;   // objects per leaf at the most (the tree is binary)

// A lane's segment [o + t0 d, o + t1 d] against the ball (gx, gy, gz, gr):
// false only if the segment's point nearest the centre lies outside the ball
// by more than the f32 margin.  NaN passes.  This is ball_touch
// (rt_device.hpp) operation for operation, written with plain fmaf so that
// the host computes the device's bits (no contraction on either side: each
// packed half there rounds like the scalar operation here).
RT_RULE_FN bool ray_bvh_touch(float gx, float gy, float gz, float gr, float ox, float oy, float oz, float dx, float dy,
                              float dz, float t0, float t1) {
    const float px = ox - gx, py = oy - gy, pz = oz - gz;
    const float bx = px * dx, by = py * dy;
    const float b = fmaf(pz, dz, bx + by);
    const float t = fminf(fmaxf(-b, t0), t1);   // closest point of the segment
    const float qx = fmaf(t, dx, px), qy = fmaf(t, dy, py), qz = fmaf(t, dz, pz);
    const float sx = qx * qx, sy = qy * qy;
    const float q2 = fmaf(qz, qz, sx + sy);
    const float e = 4e-6f * (fabsf(px) + fabsf(py) + fabsf(pz) + fabsf(t) + gr);
    const float R = gr + e;
    return !(q2 > R * R);
}

}  // namespace rtamd
