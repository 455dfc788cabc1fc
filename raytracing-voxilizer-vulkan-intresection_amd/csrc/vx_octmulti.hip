// vx_octmulti.hip -- multi-hit ray query on the octree (vx_octree_trace_multi*): vx_hitlist.h's contract over the list vx_octree_aabbs
// returns (one box per Morton item, ascending code, duplicates included).  A run is a maximal range of equal codes of the list; its boxes
// are identical, it stands for one voxel and its prim is the first list index of the run -- the index k_octree_trace reports.  The
// primitives are the runs, t = hit_aabb(box).  Every output is bit-equal to the brute force over the de-duplicated list.
//
// Enumeration: the depth-first descent of k_octree_trace (vx_octrace.hip), with vx_octnode.h's node_corner / node_enter / item_aabb: the
// corner of a node from its Morton prefix, four planes per axis per interior node, children front to back by octant ^ dirmask as bits of a
// mask in the node's level entry of an LDS stack, the degenerate-axis rule (an axis with an infinite 1/d is left out of t0 / t1 and the node
// must contain the ray's constant coordinate there).  At a leaf the first item of every run goes through vx_math.h's hit_aabb on the
// cell_aabb box k_emit_morton_aabbs writes for it, and j of that first item is the prim: the brute force is the only arbiter of t.
//
// A run is never split by a leaf boundary.  A node's item range [start, start + count) is the set of ALL items that carry its Morton
// prefix (vx_octree.hip: k_oct_depths / k_oct_nodes start a node at the first item of a prefix and end it where the next prefix starts;
// the level-by-level form's k_oct_count / k_oct_emit split a range by the next three bits of the code), equal codes share every prefix,
// and a leaf at the full depth (depth == bits) holds exactly one code, of which only the first item is tested.  A cell belongs to one node
// per level, so it is reached along one path only: counts need no de-duplication beyond the run rule.
//
// Pruning stays exact, with no epsilon -- the argument at the head of vx_octrace.hip, extended.  hit_aabb returns a voxel's own entry time
// t0_v, and it accepts the voxel only if t1_v > max(t0_v, 0).  Every computed slab time of a voxel inside a node lies within the node's
// slab interval on that axis (all the expressions are monotone in float), so the node's t0 <= t0_v < t1_v <= t1 for every voxel inside that
// hit_aabb accepts.  A reported t is such a t0_v.  Hence a node holds no element of A(r), and is dropped, when
//   * !(t1 > max(t0, 0)), or the degenerate-axis test fails: no voxel inside is hit at all;
//   * t1 < tmin:          every t0_v < t1 < tmin;
//   * t1 < after_t (cursor): every t0_v < after_t, in front of the cursor whatever the prim;
//   * t0 STRICTLY greater than the list's bound(): every t0_v >= t0 is then behind the ray's tmax, or -- without `count`, once the list
//     holds K entries -- behind the K-th kept t and cannot enter the list.  An equal t0 may still hold a smaller prim (front-to-back order
//     is not list order for negative directions), so equality keeps the node.  A child kept in a level's mask before the list filled is
//     tested again when it is popped, as the first-hit kernel tests popped children against `best` again.  (The kept t are <= tmax, so
//     bound() <= tmax always: the one comparison covers both.)
// With `count` the ray visits every node its clipped interval enters.  A NaN tmin fails `t1 >= tmin` at the root, a NaN tmax lets nodes
// through (the list stays empty, bound() is that NaN) and fails `t <= tmax` at every voxel: nothing is accepted either way.  A non-finite
// ray enters no node.
//
// The list lives in LDS beside the descent stack, [level][lane] as well: {node, child mask} per level (levels = max(bits, 1) entries);
// 64 * 8 * (levels + KC) bytes per workgroup.
#include "vx_hitlist.h"
#include "vx_octnode.h"

#include <cstring>

#pragma clang fp contract(off)

namespace vx {

namespace {

struct OctMultiParams : OctGeom {
    MultiOut o;
};

}  // namespace

template <int KC>
__global__ __launch_bounds__(kMultiBlock) void k_octree_multihit(const OctMultiParams P)
{
    extern __shared__ uint32_t om_stack[];                   // [level][lane] node, then [level][lane] mask
    __shared__ uint32_t keys[HitList<KC, false, false>::kWords];
    uint32_t* stk_node = om_stack;
    uint32_t* stk_mask = om_stack + P.levels * kMultiBlock;
    const uint32_t lane = threadIdx.x;
    const GridParams g = P.g;
    const uint32_t bits = P.bits;
    const RayArgs& io = P.o.io;
    for (uint64_t r = (uint64_t)blockIdx.x * kMultiBlock + lane; r < io.nrays; r += (uint64_t)gridDim.x * kMultiBlock) {
        float ox, oy, oz, dx, dy, dz;
        load_ray(io.rays == nullptr, r, io.rays, io.cam, ox, oy, oz, dx, dy, dz);
        SlabRay R;
        make_slab_ray(ox, oy, oz, dx, dy, dz, R);
        const uint32_t dirmask = (signbit(dx) ? 1u : 0u) | (signbit(dy) ? 2u : 0u) | (signbit(dz) ? 4u : 0u);
        HitList<KC, false, false> L;
        list_begin(L, keys, lane, P.o, r);
        const float tmax = L.tmax, tmin = io.tmin, cur_t = L.cur_t;

        bool alive = P.nitems != 0 && !ray_nonfinite(ox, oy, oz, dx, dy, dz);  // a non-finite ray is a miss: no node is entered for it
        if (alive) {
            const uint32_t c0[3] = {0u, 0u, 0u};
            float t0, t1;
            alive = node_enter(g, R, c0, 1u << bits, t0, t1) && !(t0 > L.bound()) && t1 >= tmin && !(t1 < cur_t);
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
                    if (!(t > 0.0f && t >= tmin && t <= tmax)) continue;       // rint:69, rgen:50-51
                    L.offer(t, j);
                }
            } else {
                // interior: the children the ray enters, front to back, as bits of the level's mask; four planes per axis (vx_octrace.hip)
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
                const float bound = L.bound();
                uint32_t mask = 0u;
#pragma unroll
                for (uint32_t oct = 0; oct < 8u; ++oct) {  // (octant order: ch[] stays in registers; the mask bit is the visiting position)
                    const bool ux = oct & 1u, uy = oct & 2u, uz = oct & 4u;
                    const float t0 = fmaxf(ux ? hi_mn[0] : lo_mn[0], fmaxf(uy ? hi_mn[1] : lo_mn[1], uz ? hi_mn[2] : lo_mn[2]));
                    const float t1 = fminf(ux ? hi_mx[0] : lo_mx[0], fminf(uy ? hi_mx[1] : lo_mx[1], uz ? hi_mx[2] : lo_mx[2]));
                    const bool inside = (ux ? hi_in[0] : lo_in[0]) && (uy ? hi_in[1] : lo_in[1]) && (uz ? hi_in[2] : lo_in[2]);
                    const bool in = ch[oct] != 0xFFFFFFFFu && inside && t1 > fmaxf(t0, 0.0f) && !(t0 > bound) && t1 >= tmin && !(t1 < cur_t);
                    mask |= in ? 1u << (oct ^ dirmask) : 0u;
                }
                if (mask) {
                    stk_node[depth * kMultiBlock + lane] = cur;
                    stk_mask[depth * kMultiBlock + lane] = mask;
                    top = (int)depth;
                }
            }
            // next node: the nearest remaining child of the deepest live level
            bool next = false;
            while (top >= 0) {
                uint32_t m = stk_mask[(uint32_t)top * kMultiBlock + lane];
                if (!m) { --top; continue; }
                const uint32_t i = (uint32_t)__builtin_ctz(m);
                m &= m - 1u;
                stk_mask[(uint32_t)top * kMultiBlock + lane] = m;
                const uint32_t oct = i ^ dirmask;
                const uint32_t cd = (uint32_t)top + 1u;
                const uint64_t cpath = ((path >> (3u * (depth - (uint32_t)top))) << 3) | oct;
                if (L.tightened()) {  // the list may have filled since the child was kept
                    uint32_t cc[3];
                    node_corner(cpath, cd, bits, cc);
                    float t0, t1;
                    (void)node_enter(g, R, cc, 1u << (bits - cd), t0, t1);
                    if (t0 > L.bound()) continue;
                }
                cur = P.nodes[stk_node[(uint32_t)top * kMultiBlock + lane]].children[oct];
                depth = cd;
                path = cpath;
                next = true;
                break;
            }
            if (!next) break;
        }
        L.write(P.o, r);
    }
}

void launch_octree_multihit(const vx_octree_node* nodes, const uint64_t* items, uint64_t nitems, uint32_t bits, const float root_min[3], float vs, const TraceIO& io,
                            const MultiIO& m, hipStream_t s)
{
    if (!io.nrays || !m.K) return;
    OctMultiParams P;
    std::memset(&P, 0, sizeof(P));
    set_oct_geom(P, nodes, items, nitems, bits, root_min, vs);
    set_multi_out(P.o, io, m, s);
    const size_t shmem = (size_t)P.levels * kMultiBlock * 8u;  // the stack; the list is static
    VX_MULTI_LAUNCH(k_octree_multihit, io.nrays, m.K, shmem, s, P);
}

}  // namespace vx
