// vx_octnode.h -- what the ray kernels on the octree share (k_octree_trace in vx_octrace.hip, k_octree_multihit in vx_octmulti.hip): the
// geometry block of their kernel arguments, a node's corner cell and float bounds, and the box of an item.  The argument for the bounds
// stands at the head of vx_octrace.hip.  Everything here is inlined into its caller.
#pragma once
#include "vx_internal.h"
#include "vx_ray.h"

#pragma clang fp contract(off)

namespace vx {

// the octree as a kernel reads it; each kernel's parameter block starts with this one
struct OctGeom {
    const vx_octree_node* nodes;
    const uint64_t* items;
    uint64_t nitems;  // 0: every ray misses
    GridParams g;     // org = root_min, vs, half (dims unused)
    uint32_t bits;
    uint32_t levels;  // LDS stack entries per lane (>= bits, >= 1)
};

inline void set_oct_geom(OctGeom& P, const vx_octree_node* nodes, const uint64_t* items, uint64_t nitems, uint32_t bits, const float root_min[3], float vs)
{
    P.nodes = nodes;
    P.items = items;
    P.nitems = nodes ? nitems : 0;
    for (int a = 0; a < 3; ++a) P.g.org[a] = root_min[a];
    P.g.vs = vs;
    P.g.half = vs * 0.5f;  // == k_emit_morton_aabbs
    P.bits = bits;
    P.levels = bits ? bits : 1u;
}

// corner cell of the node whose Morton prefix is `path` at depth `depth`
__device__ __forceinline__ void node_corner(uint64_t path, uint32_t depth, uint32_t bits, uint32_t c[3])
{
    const uint64_t m = path << (3u * (bits - depth));
    c[0] = compact_bits(m);
    c[1] = compact_bits(m >> 1);
    c[2] = compact_bits(m >> 2);
}

// Entry / exit of the box of `n` cells per axis from corner c (see the head of vx_octrace.hip): false when the ray misses it
__device__ __forceinline__ bool node_enter(const GridParams& g, const SlabRay& R, const uint32_t c[3], uint32_t n, float& t0, float& t1)
{
    float mn[3], mx[3];
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float lo = cell_centre(g.org[a], g.vs, c[a]) - g.half;
        const float hi = cell_centre(g.org[a], g.vs, c[a] + (n - 1u)) + g.half;
        const float p = R.inv[a] * (lo - R.o[a]), q = R.inv[a] * (hi - R.o[a]);
        mn[a] = R.deg[a] ? -INFINITY : fminf(p, q);
        mx[a] = R.deg[a] ? INFINITY : fmaxf(p, q);
        inside &= !R.deg[a] || (lo <= R.o[a] && R.o[a] <= hi);
    }
    t0 = fmaxf(mn[0], fmaxf(mn[1], mn[2]));
    t1 = fminf(mx[0], fminf(mx[1], mx[2]));
    return inside && t1 > fmaxf(t0, 0.0f);
}

// the box k_emit_morton_aabbs writes for item code m
__device__ __forceinline__ void item_aabb(const GridParams& g, uint64_t m, float bb[6]) { cell_aabb(g, compact_bits(m), compact_bits(m >> 1), compact_bits(m >> 2), bb); }

}  // namespace vx
