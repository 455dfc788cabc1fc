// vx_multihit.hip -- multi-hit ray query on the voxel grids (vx_trace_multi*): per ray the first K accepted hits in (t, prim) order and the
// number of all accepted hits, against the same boxes and under the same acceptance rule as K6 (vx_walk.hip; raytrace.rint:46-71).
//
// Contract: vx_hitlist.h's, over the occupied cells c with t_c = hit_aabb(cell_aabb(c)) and prim_c = the cell's rank in the Bool list.
// Every output is bit-equal to the brute force over all boxes.  The list below is this kernel's own text of vx_hitlist.h's HitList (the
// same order, cursor, eviction and strict pruning), kept because the kernel sits at 147-155 VGPRs with its SGPRs spilled and ran 2-4 %
// slower on the shared struct; what it adds is the lazy prim, below.
//
// Enumeration.  The candidate cells come from the major-axis slab walk of vx_walk.hip, on the structure k_build_bricks3 / k_build_mip2 make for
// it (level-0 bricks in the orientation of the ray's major axis, level-1 and level-2 mips): the same position tolerance, the same [ta, tb] of
// a slab, ta = inv_w * ((P_near -/+ tol) - o_w), tb = inv_w * ((P_far +/- tol) - o_w), the same u/v rectangle
// [min(p(ta), p(tb)) - 2 tol, max(p(ta), p(tb)) + 2 tol] at 32-cell, 8-cell and 1-cell granularity.  The superset argument at the head of
// vx_walk.hip carries over word for word: every cell whose float box the ray can enter lies in the rectangle of its 1-cell slab, and every
// box of a slab has a computed entry time >= the slab's ta.  k_walk keeps that argument in a state machine built for its persistent waves;
// here the same expressions stand in three nested loops (block slabs, the brick slabs of an occupied block rectangle, the occupied bricks of
// a brick slab's rectangle and their 1-cell slabs), restated in this file so that vx_walk.hip stays untouched in source and code generation.
// Every candidate goes through vx_math.h's hit_aabb on the cell_aabb box vx_grid_aabbs emits for it: the brute force is the only arbiter.
//
// A cell is tested at most once per ray, by construction: a ray visits every slab index along its major axis once, the slabs of one level
// are disjoint along that axis, a brick slab's rectangle lists each of its bricks once, and a cell is one bit of one brick word.  (The
// rectangles of neighbouring slabs overlap in u and v only, never along w.)  So counting needs no de-duplication.
//
// The K nearest hits of a lane live in LDS, [slot][lane], as (t bits, prim), sorted by insertion.  Accepted t are positive floats, so the
// order of their bits as unsigned integers is their float order.  The walk runs front to back along the major axis: almost every insertion
// lands at the tail.  prim = rank of the cell in the Bool list = word prefix + popcount of the bits below it, as k_rank computes it; it is
// looked up only for a hit that the buffer keeps or that ties the cursor's t.
//
// Termination.  Without `count` a ray stops at the first slab (any level) whose ta is STRICTLY greater than the K-th kept t once the buffer
// is full -- an equal t may still carry a smaller prim; inside a brick only the rest of that brick is dropped, its siblings in the same brick
// slab lie beside it, not behind.  With `count` the ray walks its whole interval [tn, tf].
//
// One ray per lane, workgroups of one wave (no barrier anywhere); the buffer is K' * 8 B * 64 lanes for K' = 4, 8, 16, 32 >= K, chosen at
// launch: 2, 4, 8, 16 KiB per workgroup, so K = 32 still leaves ten workgroups on a CU's 160 KiB of LDS.
#include "vx_hitlist.h"

#include <cstring>

#pragma clang fp contract(off)

namespace vx {

namespace {

struct MultiParams {
    GridParams g;
    const unsigned long long* bricks3;  // [3 orientations][bricks][8 slabs]
    uint64_t ori_stride;                // uint64 words per orientation
    const uint32_t* w0;                 // the reference-layout bitmask and its word prefix (prim)
    const uint32_t* prefix;
    const uint32_t* w1;                 // level-1 mip: one bit per brick
    const uint32_t* w2;                 // level-2 mip: one bit per 4^3 bricks
    uint32_t d1[3], d2[3];
    float inv_vs;
    uint32_t K;
    uint32_t* count;                    // optional
    const float* after_t;               // optional cursor (both or neither)
    const uint32_t* after_prim;
    RayArgs io;                         // rays / camera / nrays / tmin / tmax / tmax_per_ray; t_out and prim_out hold K entries per ray
};

__device__ __forceinline__ float sel3f(int p, float a, float b, float c) { return p == 0 ? a : (p == 1 ? b : c); }
__device__ __forceinline__ int sel3i(int p, int a, int b, int c) { return p == 0 ? a : (p == 1 ? b : c); }
// (cu, cv, cw) in permuted order -> (x, y, z):  w=0: x=cw y=cu z=cv;  w=1: x=cv y=cw z=cu;  w=2: x=cu y=cv z=cw   (vx_walk.hip)
__device__ __forceinline__ void unperm(int p, int cu, int cv, int cw, int& x, int& y, int& z)
{
    x = sel3i(p, cw, cv, cu);
    y = sel3i(p, cu, cw, cv);
    z = sel3i(p, cv, cu, cw);
}
__device__ __forceinline__ unsigned long long rep8(uint32_t m)  // the low byte of m in all eight bytes
{
    uint32_t r = m | (m << 8);
    r |= r << 16;
    return ((unsigned long long)r << 32) | r;
}
__device__ __forceinline__ unsigned long long sel8(int i, unsigned long long a, unsigned long long b, unsigned long long c, unsigned long long d,
                                                   unsigned long long e, unsigned long long f, unsigned long long g, unsigned long long h)
{
    const unsigned long long lo = i & 2 ? (i & 1 ? d : c) : (i & 1 ? b : a);
    const unsigned long long hi = i & 2 ? (i & 1 ? h : g) : (i & 1 ? f : e);
    return i & 4 ? hi : lo;
}

// The ray in permuted axis order (w = major axis, u and v the axes after it cyclically) and what the slab expressions read: vx_walk.hip's
// WalkLane without the state of its step machine.
struct MhRay {
    float ou, ov, ow, du, dv, iw;
    float orgu, orgv, orgw;
    int dimu, dimv, dimw, perm;
    float tol, tn, tf;
    bool pos;
};

struct MhRect { int u0, u1, v0, v1; };

// [ta, tb] of the slab of cells [i0, i1) along w
__device__ __forceinline__ void slab_interval(const MhRay& R, float vs, int i0, int i1, float& ta, float& tb)
{
    const float lo = (R.orgw + (float)i0 * vs) - R.tol, hi = (R.orgw + (float)i1 * vs) + R.tol;
    const float t_lo = R.iw * (lo - R.ow), t_hi = R.iw * (hi - R.ow);
    ta = R.pos ? t_lo : t_hi;
    tb = R.pos ? t_hi : t_lo;
}

// the cells the ray can touch inside the slab; false: none (the slab lies outside the ray's interval, or the rectangle outside the grid)
__device__ __forceinline__ bool slab_rect(const MhRay& R, float inv_vs, float ta, float tb, MhRect& q)
{
    const float ca = fmaxf(ta, R.tn), cb = fminf(tb, R.tf);
    if (!(ca <= cb)) return false;
    const float tol2 = 2.0f * R.tol;
    const float ua = R.ou + ca * R.du, ub = R.ou + cb * R.du;
    const float va = R.ov + ca * R.dv, vb = R.ov + cb * R.dv;
    int u0 = (int)floorf(((fminf(ua, ub) - tol2) - R.orgu) * inv_vs), u1 = (int)floorf(((fmaxf(ua, ub) + tol2) - R.orgu) * inv_vs);
    int v0 = (int)floorf(((fminf(va, vb) - tol2) - R.orgv) * inv_vs), v1 = (int)floorf(((fmaxf(va, vb) + tol2) - R.orgv) * inv_vs);
    q.u0 = u0 < 0 ? 0 : u0;
    q.v0 = v0 < 0 ? 0 : v0;
    q.u1 = u1 > R.dimu - 1 ? R.dimu - 1 : u1;
    q.v1 = v1 > R.dimv - 1 ? R.dimv - 1 : v1;
    return q.u0 <= q.u1 && q.v0 <= q.v1;
}

// bit (x, y, z) of a mip of dims D (x-fastest), the coordinates given in permuted order
__device__ __forceinline__ bool mip_bit(const uint32_t* __restrict__ m, const uint32_t D[3], int perm, int cu, int cv, int cw)
{
    int x, y, z;
    unperm(perm, cu, cv, cw, x, y, z);
    const uint32_t i = (uint32_t)x + D[0] * ((uint32_t)y + D[1] * (uint32_t)z);
    return (m[i >> 5] >> (i & 31u)) & 1u;
}

}  // namespace

template <int KC>
__global__ __launch_bounds__(kMultiBlock) void k_multihit(const MultiParams P)
{
    __shared__ uint32_t key_t[KC][kMultiBlock];  // [slot][lane]: consecutive lanes on consecutive banks
    __shared__ uint32_t key_p[KC][kMultiBlock];
    const uint32_t lane = threadIdx.x;
    const GridParams& g = P.g;
    const uint32_t K = P.K;
    const bool counting = P.count != nullptr;
    for (uint64_t r = (uint64_t)blockIdx.x * kMultiBlock + lane; r < P.io.nrays; r += (uint64_t)gridDim.x * kMultiBlock) {
        float ox, oy, oz, dx, dy, dz;
        load_ray(P.io.rays == nullptr, r, P.io.rays, P.io.cam, ox, oy, oz, dx, dy, dz);
        const float tmax = P.io.tmax_per_ray ? P.io.tmax_per_ray[r] : P.io.tmax;
        const float tmin = P.io.tmin;
        const float cur_t = P.after_t ? P.after_t[r] : -1.0f;
        const uint32_t cur_p = P.after_prim ? P.after_prim[r] : 0u;
        const float o[3] = {ox, oy, oz};
        const float inv[3] = {1.0f / dx, 1.0f / dy, 1.0f / dz};  // rint:48
        uint32_t n = 0;          // hits kept, <= K
        uint32_t total = 0;      // |A(r)|
        float kth = INFINITY;    // the K-th kept t once the buffer is full

        // ---- ray set-up: vx_walk.hip's walk_setup (major axis, tolerance, clip against the dilated grid box, first block slab)
        const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
        const int p = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
        MhRay R;
        R.perm = p;
        R.ow = sel3f(p, ox, oy, oz); R.iw = sel3f(p, inv[0], inv[1], inv[2]);
        R.ou = sel3f(p, oy, oz, ox); R.du = sel3f(p, dy, dz, dx);
        R.ov = sel3f(p, oz, ox, oy); R.dv = sel3f(p, dz, dx, dy);
        R.orgw = sel3f(p, g.org[0], g.org[1], g.org[2]);
        R.orgu = sel3f(p, g.org[1], g.org[2], g.org[0]);
        R.orgv = sel3f(p, g.org[2], g.org[0], g.org[1]);
        R.dimw = sel3i(p, (int)g.dim[0], (int)g.dim[1], (int)g.dim[2]);
        R.dimu = sel3i(p, (int)g.dim[1], (int)g.dim[2], (int)g.dim[0]);
        R.dimv = sel3i(p, (int)g.dim[2], (int)g.dim[0], (int)g.dim[1]);
        R.pos = R.iw > 0.0f;
        const float hx = g.org[0] + (float)g.dim[0] * g.vs, hy = g.org[1] + (float)g.dim[1] * g.vs, hz = g.org[2] + (float)g.dim[2] * g.vs;
        float Mx = fmaxf(fmaxf(fabsf(ox), fabsf(oy)), fabsf(oz));
        Mx = fmaxf(Mx, fmaxf(fmaxf(fabsf(g.org[0]), fabsf(g.org[1])), fabsf(g.org[2])));
        Mx = fmaxf(Mx, fmaxf(fmaxf(fabsf(hx), fabsf(hy)), fabsf(hz)));
        const float tol = Mx * 9.5367431640625e-07f;  // 16 * 2^-24 * max|coordinate| (vx_walk.hip)
        R.tol = tol;
        float tn = 0.0f, tf = tmax;
        bool miss = !(ax > 0.0f || ay > 0.0f || az > 0.0f) || !g.nvox || ray_nonfinite(ox, oy, oz, dx, dy, dz);  // (miss: nothing below runs)
#define VX_CLIP(o_, d_, inv_, lo_, hi_)                                                                  \
        {                                                                                                 \
            const float t1 = (((lo_)-tol) - (o_)) * (inv_), t2 = (((hi_) + tol) - (o_)) * (inv_);         \
            const bool z = (d_) == 0.0f;                                                                  \
            miss |= z && (((o_) < (lo_)-tol) || ((o_) > (hi_) + tol));                                    \
            tn = fmaxf(tn, z ? -INFINITY : fminf(t1, t2));                                                \
            tf = fminf(tf, z ? INFINITY : fmaxf(t1, t2));                                                 \
        }
        VX_CLIP(ox, dx, inv[0], g.org[0], hx)
        VX_CLIP(oy, dy, inv[1], g.org[1], hy)
        VX_CLIP(oz, dz, inv[2], g.org[2], hz)
#undef VX_CLIP
        const float tslack = 2.0f * tol * fabsf(R.iw);
        tn = fmaxf(tn - tslack, 0.0f);
        tf = tf + tslack;
        R.tn = tn;
        R.tf = tf;

        if (!miss && tn <= tf) {
            const int s = R.pos ? 1 : -1;
            const float pw = sel3f(p, ox + tn * dx, oy + tn * dy, oz + tn * dz);
            int cw = (int)floorf((pw - R.orgw) * P.inv_vs) + (R.pos ? -1 : 1);  // one cell of slack against the rounding of this estimate
            cw = cw < 0 ? 0 : (cw > R.dimw - 1 ? R.dimw - 1 : cw);
            constexpr int kBlkShift = (int)kBlockCellsShift, kBlkBricksShift = (int)kBlockBricksShift, kBlkBricks = (int)kBlockBricks;
            const int nk2 = (R.dimw + (int)kBlockCells - 1) >> kBlkShift, nk1 = (R.dimw + 7) >> 3;
            bool done = false;
            // ---- block slabs (32 cells), from the one that holds the entry point
            for (int k2 = cw >> kBlkShift; k2 >= 0 && k2 < nk2 && !done; k2 += s) {
                float ta, tb;
                const int e2 = (k2 + 1) << kBlkShift;
                slab_interval(R, g.vs, k2 << kBlkShift, e2 > R.dimw ? R.dimw : e2, ta, tb);
                if (ta > R.tf || (!counting && n == K && ta > kth)) break;  // beyond the interval / no box from here on can enter the list
                MhRect q2;
                if (!slab_rect(R, P.inv_vs, ta, tb, q2)) continue;
                bool occ2 = false;
                for (int cv = q2.v0 >> kBlkShift; cv <= (q2.v1 >> kBlkShift); ++cv)
                    for (int cu = q2.u0 >> kBlkShift; cu <= (q2.u1 >> kBlkShift); ++cu) occ2 |= mip_bit(P.w2, P.d2, p, cu, cv, k2);
                if (!occ2) continue;
                // ---- its brick slabs (8 cells), in travel order
                for (int j = 0; j < kBlkBricks && !done; ++j) {
                    const int k1 = (k2 << kBlkBricksShift) + (R.pos ? j : kBlkBricks - 1 - j);
                    if (k1 >= nk1) continue;
                    const int e1 = (k1 + 1) << 3;
                    slab_interval(R, g.vs, k1 << 3, e1 > R.dimw ? R.dimw : e1, ta, tb);
                    if (ta > R.tf || (!counting && n == K && ta > kth)) { done = true; break; }
                    MhRect q1;
                    if (!slab_rect(R, P.inv_vs, ta, tb, q1)) continue;
                    // ---- the occupied bricks of its rectangle, each walked through its 1-cell slabs
                    for (int cv = q1.v0 >> 3; cv <= (q1.v1 >> 3); ++cv)
                        for (int cu = q1.u0 >> 3; cu <= (q1.u1 >> 3); ++cu) {
                            if (!mip_bit(P.w1, P.d1, p, cu, cv, k1)) continue;
                            int bx, by, bz;
                            unperm(p, cu, cv, k1, bx, by, bz);
                            const uint64_t bi = (uint64_t)(uint32_t)bx + (uint64_t)P.d1[0] * ((uint64_t)(uint32_t)by + (uint64_t)P.d1[1] * (uint32_t)bz);
                            const ulonglong2* wp = reinterpret_cast<const ulonglong2*>(P.bricks3 + (uint64_t)p * P.ori_stride + bi * 8ull);
                            const ulonglong2 w01 = wp[0], w23 = wp[1], w45 = wp[2], w67 = wp[3];  // one 64-byte line
                            const int bu = cu << 3, bv = cv << 3;
                            uint32_t sm;  // slabs of the brick whose word meets the rectangle the ray sweeps across the whole brick slab
                            {
                                const int a0 = (q1.u0 > bu ? q1.u0 : bu) - bu, a1 = (q1.u1 < bu + 7 ? q1.u1 : bu + 7) - bu;
                                const int b0 = (q1.v0 > bv ? q1.v0 : bv) - bv, b1 = (q1.v1 < bv + 7 ? q1.v1 : bv + 7) - bv;
                                const unsigned long long rect = rep8((2u << a1) - (1u << a0)) & (~0ull >> (8 * (7 - b1))) & (~0ull << (8 * b0));
                                sm = ((w01.x & rect) ? 1u : 0u) | ((w01.y & rect) ? 2u : 0u) | ((w23.x & rect) ? 4u : 0u) | ((w23.y & rect) ? 8u : 0u) |
                                     ((w45.x & rect) ? 16u : 0u) | ((w45.y & rect) ? 32u : 0u) | ((w67.x & rect) ? 64u : 0u) | ((w67.y & rect) ? 128u : 0u);
                            }
                            while (sm) {
                                const int sl = R.pos ? (__ffs(sm) - 1) : (31 - __clz(sm));  // next candidate slab in travel order
                                sm &= ~(1u << sl);
                                const int c = (k1 << 3) + sl;
                                slab_interval(R, g.vs, c, c + 1, ta, tb);
                                if (ta > R.tf || (!counting && n == K && ta > kth)) break;  // the rest of THIS brick; its siblings lie beside it
                                MhRect q0;
                                if (!slab_rect(R, P.inv_vs, ta, tb, q0)) continue;
                                int a0 = q0.u0 - bu, a1 = q0.u1 - bu, b0 = q0.v0 - bv, b1 = q0.v1 - bv;
                                a0 = a0 < 0 ? 0 : a0; b0 = b0 < 0 ? 0 : b0;
                                a1 = a1 > 7 ? 7 : a1; b1 = b1 > 7 ? 7 : b1;
                                if (a0 > a1 || b0 > b1) continue;
                                unsigned long long cand = sel8(sl, w01.x, w01.y, w23.x, w23.y, w45.x, w45.y, w67.x, w67.y) & rep8((2u << a1) - (1u << a0)) &
                                                          (~0ull >> (8 * (7 - b1))) & (~0ull << (8 * b0));
                                // ---- exact tests: hitAabb on the box the list holds for the cell
                                while (cand) {
                                    const int b = __ffsll((long long)cand) - 1;
                                    cand &= cand - 1ull;
                                    int x, y, z;
                                    unperm(p, bu + (b & 7), bv + (b >> 3), c, x, y, z);
                                    float bb[6];
                                    cell_aabb(g, (uint32_t)x, (uint32_t)y, (uint32_t)z, bb);
                                    const float t = hit_aabb(bb, o, inv);
                                    if (!(t > 0.0f && t >= tmin && t <= tmax)) continue;  // rint:69, rgen:50-51
                                    if (t < cur_t) continue;                             // in front of the cursor
                                    const bool keep = n < K || !(t > kth);               // (an equal t may carry a smaller prim)
                                    if (!keep && t != cur_t) { ++total; continue; }      // counted; its prim is never read
                                    const uint64_t vi = (uint64_t)(uint32_t)x + (uint64_t)g.dim[0] * ((uint64_t)(uint32_t)y + (uint64_t)g.dim[1] * (uint32_t)z);
                                    const uint32_t prim = voxel_rank(vi, P.w0, P.prefix, nullptr);  // as k_rank
                                    if (t == cur_t && prim <= cur_p) continue;           // not strictly after the cursor
                                    ++total;
                                    if (!keep) continue;
                                    const uint32_t tbits = __float_as_uint(t);
                                    uint32_t jn = n < K ? n : K - 1u;  // where the list's new tail goes: the K-th entry falls out of a full list
                                    if (n == K && !(tbits < key_t[jn][lane] || (tbits == key_t[jn][lane] && prim < key_p[jn][lane]))) continue;
                                    while (jn > 0u) {
                                        const uint32_t pt = key_t[jn - 1u][lane], pp = key_p[jn - 1u][lane];
                                        if (!(tbits < pt || (tbits == pt && prim < pp))) break;
                                        key_t[jn][lane] = pt;
                                        key_p[jn][lane] = pp;
                                        --jn;
                                    }
                                    key_t[jn][lane] = tbits;
                                    key_p[jn][lane] = prim;
                                    if (n < K) ++n;
                                    if (n == K) kth = __uint_as_float(key_t[K - 1u][lane]);
                                }
                            }
                        }
                }
            }
        }
        // ---- outputs: K entries per ray, ray-major
        float* t_out = P.io.t_out ? P.io.t_out + r * K : nullptr;
        uint32_t* p_out = P.io.prim_out ? P.io.prim_out + r * K : nullptr;
        for (uint32_t jn = 0; jn < K; ++jn) {
            if (t_out) t_out[jn] = jn < n ? __uint_as_float(key_t[jn][lane]) : -1.0f;
            if (p_out) p_out[jn] = jn < n ? key_p[jn][lane] : 0xFFFFFFFFu;
        }
        if (counting) P.count[r] = total;
    }
}

void launch_multihit(const GridParams& g, const TraceMips& mips, const uint32_t* word_prefix, const TraceIO& io, const MultiIO& m, hipStream_t s)
{
    if (!io.nrays || !m.K) return;
    MultiParams P;
    std::memset(&P, 0, sizeof(P));
    P.g = g;
    if (!mips.bricks3 || !word_prefix) P.g.nvox = 0;  // nothing to walk: every ray misses
    P.bricks3 = mips.bricks3;
    P.ori_stride = (uint64_t)mips.d1[0] * mips.d1[1] * mips.d1[2] * 8ull;
    P.w0 = mips.w0;
    P.prefix = word_prefix;
    P.w1 = mips.w1;
    P.w2 = mips.w2;
    for (int a = 0; a < 3; ++a) { P.d1[a] = mips.d1[a]; P.d2[a] = mips.d2[a]; }
    P.inv_vs = 1.0f / g.vs;
    P.K = m.K;
    P.count = m.count;
    P.after_t = m.after_t;
    P.after_prim = m.after_prim;
    set_ray_args(P.io, io, s);
    VX_MULTI_LAUNCH(k_multihit, io.nrays, m.K, 0, s, P);
}

}  // namespace vx
