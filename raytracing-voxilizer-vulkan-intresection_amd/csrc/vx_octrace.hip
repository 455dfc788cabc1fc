// vx_octrace.hip -- first hit per ray against the octree's AABB list (vx_octree_aabbs: one box per Morton item, ascending code, duplicates
// included), by descending the node array itself -- the reference's second BLAS input (hello_vulkan.cpp:690-697 -> Octree::getAabbs) under
// the same procedural-hit stage raytrace.rint:46-71 that k_walk serves for the grids.
//
// Result contract (include/voxhip.h): t = the minimum over ALL list boxes of hitAabb, accepted iff t > 0 and tmin <= t <= tmax; prim = the
// smallest list index among the boxes reaching it -- exactly oracle.trace_brute over the list.
//
// One ray per lane, wave64, workgroups of kOctBlock lanes, a depth-first descent from the root:
//   * a node at depth d covers 2^(bits-d) cells per axis from the corner its Morton prefix decodes to (the path from the root IS that
//     prefix; the octree's codes decode to 21 bits per axis however many of them the reference's 16-bit interleave filled, so the tree is a
//     clean spatial subdivision of the decoded cells the list's boxes come from);
//   * its float bounds are the min corner of its FIRST cell's cell_aabb and the max corner of its LAST cell's.  cell_centre, `c - half`,
//     `c + half`, `plane - o` and `inv * x` are all monotone in float, so every voxel box inside lies within the node's bounds and each of
//     its computed slab times lies inside the node's slab interval: the node's computed entry t0 <= every inside voxel's t0, and its exit t1
//     >= theirs.  A voxel hit needs t1_v > max(t0_v, 0), so a node with !(t1 > max(t0, 0)) holds none, and a node with t0 > best holds none
//     that beats or ties best (the same argument vx_walk.hip makes for its slabs; no epsilon);
//   * an axis with an infinite 1/d (d = +-0 or denormal) is left out of t0 / t1: a product there can be 0 * inf = NaN, which hitAabb's
//     fminf / fmaxf skip.  On such an axis the ray's coordinate is the constant o, and a voxel whose slab does not contain o gets the slab
//     [inf, inf] or [-inf, -inf] there (a miss), so the node is entered only when lo <= o <= hi.  The remaining axes still bound t0_v from
//     below and t1_v from above (a NaN-skipped axis only drops a term from max / min), so both pruning rules stay exact;
//   * children are visited front to back, octant i ^ dirmask for i = 0..7 (dirmask: a bit per negative direction component), and only
//     those the ray enters, with t0 <= best, are kept -- as a mask of up to eight bits in the node's level entry of an LDS stack
//     ({node, mask} per level, bits entries at most: one per depth, never more, whatever rounding does at shared faces).  A popped child is
//     tested against best again when a hit has been found since;
//   * a leaf's items [start, start + count) are sorted: only the first code of each run of equal codes goes through hit_aabb (a leaf at the
//     full depth holds one code), on the box k_emit_morton_aabbs writes for it -- the reported t is the very float the brute force yields;
//   * ties: front-to-back order is not list order (negative directions), so a voxel is accepted on t < best, or on t == best with a smaller
//     index, and a node is pruned only on t0 STRICTLY greater than best;
//   * any_hit ends the ray at its first accepted hit.
// Outputs per ray: t, prim (list index), the cube-face normal of the box at prim (raytrace2.rchit:60-73), shadowed, and the compacted hit list.
#include "vx_internal.h"
#include "vx_octnode.h"
#include "vx_ray.h"

#include <cstring>

#pragma clang fp contract(off)

namespace vx {

namespace {

constexpr uint32_t kOctBlock = 256;  // lanes per workgroup (4 waves); the stack is [level][lane] in LDS

// the geometry block, node_corner, node_enter and item_aabb: vx_octnode.h, shared with k_octree_multihit
struct OctParams : OctGeom {
    RayArgs io;
};

}  // namespace

__global__ __launch_bounds__(kOctBlock) void k_octree_trace(OctParams P)
{
    extern __shared__ uint32_t oct_lds[];
    uint32_t* stk_node = oct_lds;                            // [level][lane]: consecutive lanes on consecutive banks
    uint32_t* stk_mask = oct_lds + P.levels * kOctBlock;
    const uint32_t tid = threadIdx.x;
    const uint64_t r = (uint64_t)blockIdx.x * kOctBlock + tid;
    const bool active = r < P.io.nrays;
    const GridParams g = P.g;
    const uint32_t bits = P.bits;

    float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 0.f, dz = 0.f;
    float best = -1.0f;
    uint32_t bp = 0xFFFFFFFFu;
    bool found = false;
    if (active) {
        load_ray(P.io.rays == nullptr, r, P.io.rays, P.io.cam, ox, oy, oz, dx, dy, dz);
        SlabRay R;
        make_slab_ray(ox, oy, oz, dx, dy, dz, R);
        const uint32_t dirmask = (signbit(dx) ? 1u : 0u) | (signbit(dy) ? 2u : 0u) | (signbit(dz) ? 4u : 0u);
        const float tmin = P.io.tmin;
        best = P.io.tmax_per_ray ? P.io.tmax_per_ray[r] : P.io.tmax;  // acceptance bound until the first hit (rint:69 + rgen:50-51)

        bool alive = P.nitems != 0 && !ray_nonfinite(ox, oy, oz, dx, dy, dz);  // a non-finite ray is a miss: no node is entered for it
        if (alive) {
            const uint32_t c0[3] = {0u, 0u, 0u};
            float t0, t1;
            alive = node_enter(g, R, c0, 1u << bits, t0, t1) && !(t0 > best) && t1 >= tmin;
        }
        uint32_t cur = 0, depth = 0;
        uint64_t path = 0;
        int top = -1;  // deepest level whose entry is live
        while (alive) {
            const uint2* np = reinterpret_cast<const uint2*>(P.nodes + cur);
            const uint2 q0 = np[0], q1 = np[1], q2 = np[2], q3 = np[3], q4 = np[4];
            const uint32_t ch[8] = {q0.x, q0.y, q1.x, q1.y, q2.x, q2.y, q3.x, q3.y};
            if (depth >= bits || (ch[0] & ch[1] & ch[2] & ch[3] & ch[4] & ch[5] & ch[6] & ch[7]) == 0xFFFFFFFFu) {
                // leaf: the first item of every run of equal codes (a leaf at the full depth holds a single code)
                const uint32_t start = q4.x, end = depth == bits ? q4.x + (q4.y ? 1u : 0u) : q4.x + q4.y;
                uint64_t prev = ~0ull;
                for (uint32_t j = start; j < end; ++j) {
                    const uint64_t m = P.items[j];
                    if (m == prev) continue;
                    prev = m;
                    float bb[6];
                    item_aabb(g, m, bb);
                    const float t = hit_aabb(bb, R.o, R.inv);
                    if (t > 0.0f && t >= tmin && (found ? (t < best || (t == best && j < bp)) : t <= best)) { best = t; bp = j; found = true; }  // rint:69
                }
                if (found && P.io.any_hit) break;  // gl_RayFlagsTerminateOnFirstHitEXT (raytrace2.rchit:108)
            } else {
                // interior: the children the ray enters, front to back, as bits of the level's mask.  Per axis the children's bounds are four
                // planes -- the node's own min and max and the two middle ones, cell_aabb of the last lower and the first upper cell -- the
                // very floats a child's own first / last cell gives, so the slab times are computed once per plane, not per child.
                uint32_t c[3];
                node_corner(path, depth, bits, c);
                const uint32_t h = 1u << (bits - depth - 1u);
                float lo_mn[3], lo_mx[3], hi_mn[3], hi_mx[3];  // slab interval of the lower / upper half along each axis
                bool lo_in[3], hi_in[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const float p0 = cell_centre(g.org[a], g.vs, c[a]) - g.half, p1 = cell_centre(g.org[a], g.vs, c[a] + (h - 1u)) + g.half;
                    const float p2 = cell_centre(g.org[a], g.vs, c[a] + h) - g.half, p3 = cell_centre(g.org[a], g.vs, c[a] + (2u * h - 1u)) + g.half;
                    const float s0 = R.inv[a] * (p0 - R.o[a]), s1 = R.inv[a] * (p1 - R.o[a]), s2 = R.inv[a] * (p2 - R.o[a]), s3 = R.inv[a] * (p3 - R.o[a]);
                    lo_mn[a] = R.deg[a] ? -INFINITY : fminf(s0, s1);
                    lo_mx[a] = R.deg[a] ? INFINITY : fmaxf(s0, s1);
                    hi_mn[a] = R.deg[a] ? -INFINITY : fminf(s2, s3);
                    hi_mx[a] = R.deg[a] ? INFINITY : fmaxf(s2, s3);
                    lo_in[a] = !R.deg[a] || (p0 <= R.o[a] && R.o[a] <= p1);
                    hi_in[a] = !R.deg[a] || (p2 <= R.o[a] && R.o[a] <= p3);
                }
                uint32_t mask = 0u;
#pragma unroll
                for (uint32_t oct = 0; oct < 8u; ++oct) {  // (octant order: ch[] stays in registers; the mask bit is the visiting position)
                    const bool ux = oct & 1u, uy = oct & 2u, uz = oct & 4u;
                    const float t0 = fmaxf(ux ? hi_mn[0] : lo_mn[0], fmaxf(uy ? hi_mn[1] : lo_mn[1], uz ? hi_mn[2] : lo_mn[2]));
                    const float t1 = fminf(ux ? hi_mx[0] : lo_mx[0], fminf(uy ? hi_mx[1] : lo_mx[1], uz ? hi_mx[2] : lo_mx[2]));
                    const bool inside = (ux ? hi_in[0] : lo_in[0]) && (uy ? hi_in[1] : lo_in[1]) && (uz ? hi_in[2] : lo_in[2]);
                    const bool in = ch[oct] != 0xFFFFFFFFu && inside && t1 > fmaxf(t0, 0.0f) && !(t0 > best) && t1 >= tmin;  // == node_enter
                    mask |= in ? 1u << (oct ^ dirmask) : 0u;
                }
                if (mask) {
                    stk_node[depth * kOctBlock + tid] = cur;
                    stk_mask[depth * kOctBlock + tid] = mask;
                    top = (int)depth;
                }
            }
            // next node: the nearest remaining child of the deepest live level
            bool next = false;
            while (top >= 0) {
                uint32_t m = stk_mask[(uint32_t)top * kOctBlock + tid];
                if (!m) { --top; continue; }
                const uint32_t i = (uint32_t)__builtin_ctz(m);
                m &= m - 1u;
                stk_mask[(uint32_t)top * kOctBlock + tid] = m;
                const uint32_t oct = i ^ dirmask;
                const uint32_t cd = (uint32_t)top + 1u;
                const uint64_t cpath = ((path >> (3u * (depth - (uint32_t)top))) << 3) | oct;
                if (found) {  // best has moved since the child was kept
                    uint32_t cc[3];
                    node_corner(cpath, cd, bits, cc);
                    float t0, t1;
                    (void)node_enter(g, R, cc, 1u << (bits - cd), t0, t1);
                    if (t0 > best) continue;
                }
                cur = P.nodes[stk_node[(uint32_t)top * kOctBlock + tid]].children[oct];
                depth = cd;
                path = cpath;
                next = true;
                break;
            }
            if (!next) break;
        }
    }
    const float tt = found ? best : -1.0f;
    const uint32_t prim = found ? bp : 0xFFFFFFFFu;
    if (active) {
        if (P.io.t_out) P.io.t_out[r] = tt;
        if (P.io.prim_out) P.io.prim_out[r] = prim;
        if (P.io.shadowed_out) P.io.shadowed_out[r] = found ? 1 : 0;
        if (P.io.normal_out) {
            float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
            if (found) {
                float bb[6];
                item_aabb(g, P.items[bp], bb);
                cube_normal(bb, ox, oy, oz, dx, dy, dz, tt, n0, n1, n2);
            }
            P.io.normal_out[3 * r] = n0; P.io.normal_out[3 * r + 1] = n1; P.io.normal_out[3 * r + 2] = n2;
        }
    }
    if (P.io.hits) compact_hit(found, r, prim, tt, P.io.hits, P.io.nhits);  // every lane of the workgroup gets here
}

void launch_octree_trace(const vx_octree_node* nodes, const uint64_t* items, uint64_t nitems, uint32_t bits, const float root_min[3], float vs, const TraceIO& io,
                         hipStream_t s)
{
    if (!io.nrays) return;
    OctParams P;
    std::memset(&P, 0, sizeof(P));
    set_oct_geom(P, nodes, items, nitems, bits, root_min, vs);
    set_ray_args(P.io, io, s);
    const size_t shmem = (size_t)P.levels * kOctBlock * 8u;
    const uint64_t nblk = (io.nrays + kOctBlock - 1) / kOctBlock;
    VX_KL(k_octree_trace, dim3((unsigned)nblk), dim3(kOctBlock), shmem, s, P);
}

}  // namespace vx
