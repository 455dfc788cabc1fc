// vx_tlas.hip -- instanced triangle scenes: the reference's top-level acceleration structure (createTopLevelAS, hello_vulkan.cpp:760-790)
// over transformed instances of triangle BVHs (vx_bvh, the BLAS), built on the device and traced two levels deep.
//
// Contract (include/voxhip.h): instance i with object-to-world M_i (row-major 3x4) and its world-to-object W_i (the float64 adjugate
// inverse, rounded to float32) moves the ray into object space, o' = ((w0*ox + w1*oy) + w2*oz) + w3 and d' = (w0*dx + w1*dy) + w2*dz per
// row, and tests its BLAS's triangles there with vx_bvh's Moeller-Trumbore and the same interval.  t = the minimum over all active
// (instance, triangle) pairs, (instance, prim) = the lexicographically smallest pair reaching it, bary its (u, v): the brute force over
// every pair (tests/instance_ref.py).  The TLAS only accelerates.
//
// Build and update, all on the device (no host synchronisation):
//   k_tlas_prep    per instance: the inverse, the active flag, the world box of the 8 transformed corners of its BLAS's root box (widened
//                  by that BLAS's own pad), widened by the instance's margin (below); the union of the boxes and the largest condition
//                  number of an active instance (ordered-int atomics);
//   k_tlas_keys    30-bit Morton code of the box centre, key = code << 32 | instance;
//   launch_sort_u64 over 62 bits, k_bvh_karras (vx_bvh.hip, unchanged) for the radix tree;
//   k_tlas_bounds  one lane per leaf (one instance per leaf) writes its node and climbs: the second lane to reach a node merges the two
//                  children's boxes and goes on, as k_bvh_bounds.  The node array is the radix tree itself (2n-1 nodes, root at 0).
// The height is at most min(n - 1, 30 + ceil(log2 n)): along a path the split bit strictly descends, and only the 30 Morton bits and the
// low ceil(log2 n) bits of the instance index can differ between keys.  The trace sizes its stack to that bound, which the host knows
// without reading the tree back.
//
// Margin.  A BLAS hit at t lies, in object space, in its root box widened by the BLAS pad (the BLAS's own guarantee, §6c).
// Mapped back, the world point o + t*d differs from M (o' + t*d') + T by M (e_o + t*e_d), the rounding of the ray transform and of W:
// to first order at most ~6 eps cond(M) (|o| + |T| + t|d|) in the infinity norm, with cond(M) = |M| |W|.  Near the box t|d| <= |x| + |o|,
// so the error is at most ~6 eps cond(M) (2|o| + |T| + |x|).  The instance's world box therefore carries 2^-16 cond(M) (|T| + its largest
// |world coordinate|) + 2^-18 (|M| |object corner| + |T|) (the rounding of the corners) + 2^-10 of its largest side, and every TLAS box
// test adds 2^-15 cond_max |o| for the ray (cond_max over the active instances) and the slab widening kTRel: at least 40 times the
// first-order bound.  At a TLAS leaf the instance is entered on its BLAS root box in OBJECT space, exactly as k_bvh_trace enters its root.
#include "vx_internal.h"
#include "vx_ray.h"
#include "vx_blas.h"

#include <cstring>

#pragma clang fp contract(off)

namespace vx {

namespace {

constexpr uint32_t kBuildBlock = 256;
constexpr uint32_t kTlasBlock = 128;         // lanes per trace workgroup; the stack is [level][lane] in LDS
constexpr float kCond = 1.0f / 65536.0f;     // world-box margin per unit of cond(M) (|T| + |x|)
constexpr float kCorner = 1.0f / 262144.0f;  // the rounding of the transformed corners
constexpr float kExt = 1.0f / 1024.0f;       // relative to the instance's world extent
constexpr float kRayPad = 1.0f / 32768.0f;   // per ray: cond_max |o|

__device__ __forceinline__ float fabs_max3(float a, float b, float c) { return fmaxf(fmaxf(fabsf(a), fabsf(b)), fabsf(c)); }

// row r of a 3x4 matrix applied to a point, in the pinned association ((m0*x + m1*y) + m2*z) + m3
__device__ __forceinline__ float xf_row(const float* m, float x, float y, float z) { return ((m[0] * x + m[1] * y) + m[2] * z) + m[3]; }

}  // namespace

// Per instance: inverse, active flag, widened world box (ibox: lo, hi as float4 pairs; inactive: the empty box +inf / -inf; a box that
// overflows float32: the whole space -inf / +inf, left out of the union), the union of
// the active boxes (small[0..5], ordered uint, initialised to ~0 / 0) and the largest condition number (small[6], ordered uint, init 0).
__global__ __launch_bounds__(kBuildBlock) void k_tlas_prep(const vx_instance* __restrict__ in, uint32_t n, const TlasBlas* __restrict__ tab, uint32_t nb,
                                                           float* __restrict__ xf, float* __restrict__ w2o, uint32_t* __restrict__ iblas,
                                                           float4* __restrict__ ibox, uint32_t* __restrict__ small)
{
    const uint32_t i = blockIdx.x * kBuildBlock + threadIdx.x;
    if (i >= n) return;
    const vx_instance I = in[i];
    float m[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = I.transform[k];
    // the pinned float64 inverse (include/voxhip.h): cofactors, det = (m0*c00 + m1*c01) + m2*c02, inv[r][c] = C[c][r] / det, w3 = -(inv T)
    const double a0 = m[0], a1 = m[1], a2 = m[2], a4 = m[4], a5 = m[5], a6 = m[6], a8 = m[8], a9 = m[9], a10 = m[10];
    const double C[9] = {a5 * a10 - a6 * a9, a6 * a8 - a4 * a10, a4 * a9 - a5 * a8,
                         a2 * a9 - a1 * a10, a0 * a10 - a2 * a8, a1 * a8 - a0 * a9,
                         a1 * a6 - a2 * a5, a2 * a4 - a0 * a6, a0 * a5 - a1 * a4};
    const double det = (a0 * C[0] + a1 * C[1]) + a2 * C[2];
    const double t0 = m[3], t1 = m[7], t2 = m[11];
    float w[12];
    bool finite = true;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double i0 = C[0 * 3 + r] / det, i1 = C[1 * 3 + r] / det, i2 = C[2 * 3 + r] / det;
        const double tr = -((i0 * t0 + i1 * t1) + i2 * t2);
        w[4 * r] = (float)i0; w[4 * r + 1] = (float)i1; w[4 * r + 2] = (float)i2; w[4 * r + 3] = (float)tr;
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        finite &= isfinite(w[k]);
        xf[12ull * i + k] = m[k];
        w2o[12ull * i + k] = w[k];
    }
    const bool active = I.mask != 0u && I.blas < nb && tab[I.blas < nb ? I.blas : 0].ntri != 0u && isfinite(det) && det != 0.0 && finite;
    iblas[i] = active ? I.blas : blas::kNone;
    if (!active) {
        ibox[2ull * i] = make_float4(INFINITY, INFINITY, INFINITY, 0.0f);
        ibox[2ull * i + 1] = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.0f);
        return;
    }
    const TlasBlas& B = tab[I.blas];
    const float lo[3] = {B.rmin[0] - B.pad, B.rmin[1] - B.pad, B.rmin[2] - B.pad}, hi[3] = {B.rmax[0] + B.pad, B.rmax[1] + B.pad, B.rmax[2] + B.pad};
    float bmin[3] = {INFINITY, INFINITY, INFINITY}, bmax[3] = {-INFINITY, -INFINITY, -INFINITY};
    float omax = 0.0f;
    bool whole = false;  // a corner that overflows (or 0 * Inf = NaN, which fminf / fmaxf would drop): the box is the whole space
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float x = (c & 1) ? hi[0] : lo[0], y = (c & 2) ? hi[1] : lo[1], z = (c & 4) ? hi[2] : lo[2];
        omax = fmaxf(omax, fabs_max3(x, y, z));
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float v = xf_row(m + 4 * r, x, y, z);
            whole |= !isfinite(v);
            bmin[r] = fminf(bmin[r], v);
            bmax[r] = fmaxf(bmax[r], v);
        }
    }
    float nm = 0.0f, nw = 0.0f;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        nm = fmaxf(nm, (fabsf(m[4 * r]) + fabsf(m[4 * r + 1])) + fabsf(m[4 * r + 2]));
        nw = fmaxf(nw, (fabsf(w[4 * r]) + fabsf(w[4 * r + 1])) + fabsf(w[4 * r + 2]));
    }
    const float cond = fminf(nm * nw, 3.0e38f);
    const float tn = fabs_max3(m[3], m[7], m[11]);
    const float cmax = fmaxf(fabs_max3(bmin[0], bmin[1], bmin[2]), fabs_max3(bmax[0], bmax[1], bmax[2]));
    const float ext = fmaxf(fmaxf(bmax[0] - bmin[0], bmax[1] - bmin[1]), bmax[2] - bmin[2]);
    const float pad = (kCond * cond * (tn + cmax) + kCorner * (nm * omax + tn)) + kExt * ext;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        bmin[r] = bmin[r] - pad;
        bmax[r] = bmax[r] + pad;
        whole |= !isfinite(bmin[r]) || !isfinite(bmax[r]);
    }
    atomicMax(&small[6], f2ord(cond));
    if (whole) {
        // a world box that is not finite bounds nothing: the instance is entered by every ray (its BLAS root box, in object space, still
        // prunes), and it stays out of the union, so that the Morton codes of the other instances keep their resolution (its own is 0)
        ibox[2ull * i] = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.0f);
        ibox[2ull * i + 1] = make_float4(INFINITY, INFINITY, INFINITY, 0.0f);
        return;
    }
    ibox[2ull * i] = make_float4(bmin[0], bmin[1], bmin[2], 0.0f);
    ibox[2ull * i + 1] = make_float4(bmax[0], bmax[1], bmax[2], 0.0f);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        atomicMin(&small[a], f2ord(bmin[a]));
        atomicMax(&small[3 + a], f2ord(bmax[a]));
    }
}

__global__ __launch_bounds__(kBuildBlock) void k_tlas_keys(const float4* __restrict__ ibox, uint32_t n, const uint32_t* __restrict__ small,
                                                           uint64_t* __restrict__ keys)
{
    const uint32_t i = blockIdx.x * kBuildBlock + threadIdx.x;
    if (i >= n) return;
    const float4 b0 = ibox[2ull * i], b1 = ibox[2ull * i + 1];
    const float c[3] = {(b0.x + b1.x) * 0.5f, (b0.y + b1.y) * 0.5f, (b0.z + b1.z) * 0.5f};
    uint32_t q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float lo = ord2f(small[a]), hi = ord2f(small[3 + a]);
        const float ext = hi - lo;
        const float f = ext > 0.0f ? (c[a] - lo) / ext * 1024.0f : 0.0f;
        q[a] = f >= 1023.0f ? 1023u : (f > 0.0f ? (uint32_t)f : 0u);  // (NaN: inactive or whole-space instances, an empty union -> 0)
    }
    const uint64_t code = (uint64_t)(spread10(q[0]) | (spread10(q[1]) << 1) | (spread10(q[2]) << 2));
    keys[i] = (code << 32) | i;
}

// nodes: {min xyz, a, max xyz, b} (vx_bvh_node); interior a, b = children (radix-tree numbering: internal i -> i, leaf j -> n-1+j);
// leaf a = instance, b = VX_BVH_LEAF | 1.  hgt: the height of every node; small[7] = the root's.
__global__ __launch_bounds__(kBuildBlock) void k_tlas_bounds(uint32_t n, const uint64_t* __restrict__ keys, const float4* __restrict__ ibox,
                                                             const uint32_t* __restrict__ child, const uint32_t* __restrict__ parent,
                                                             uint32_t* __restrict__ arrived, float4* nodes, uint32_t* hgt, uint32_t* small)
{
    const uint32_t j = blockIdx.x * kBuildBlock + threadIdx.x;
    if (j >= n) return;
    const uint32_t inst = (uint32_t)(keys[j] & 0xFFFFFFFFull);
    const uint32_t leaf = n - 1 + j;
    const float4 b0 = ibox[2ull * inst], b1 = ibox[2ull * inst + 1];
    nodes[2ull * leaf] = make_float4(b0.x, b0.y, b0.z, __uint_as_float(inst));
    nodes[2ull * leaf + 1] = make_float4(b1.x, b1.y, b1.z, __uint_as_float(blas::kLeafBit | 1u));
    hgt[leaf] = 0u;
    if (leaf == 0) { small[7] = 0u; return; }  // one instance: the leaf is the root
    uint32_t node = parent[leaf];
    while (node != blas::kNone) {
        __threadfence();                                   // release this lane's node
        if (atomicAdd(&arrived[node], 1u) == 0u) return;   // the sibling is not there yet: its lane carries on
        __threadfence();                                   // acquire the sibling's
        const uint32_t a = child[2 * node], b = child[2 * node + 1];
        const float4 a0 = nodes[2ull * a], a1 = nodes[2ull * a + 1];  // (nodes / hgt are not __restrict__: these loads stay behind the fence)
        const float4 c0 = nodes[2ull * b], c1 = nodes[2ull * b + 1];
        const uint32_t ha = hgt[a], hb = hgt[b];
        const uint32_t h = 1u + (ha > hb ? ha : hb);
        nodes[2ull * node] = make_float4(fminf(a0.x, c0.x), fminf(a0.y, c0.y), fminf(a0.z, c0.z), __uint_as_float(a));
        nodes[2ull * node + 1] = make_float4(fmaxf(a1.x, c1.x), fmaxf(a1.y, c1.y), fmaxf(a1.z, c1.z), __uint_as_float(b));
        hgt[node] = h;
        if (node == 0) small[7] = h;
        node = parent[node];
    }
}

void launch_tlas_prep(const vx_instance* in, uint32_t n, const TlasBlas* tab, uint32_t nb, float* xf, float* w2o, uint32_t* iblas, float* ibox,
                      uint32_t* small, uint64_t* keys, hipStream_t s)
{
    const dim3 g((n + kBuildBlock - 1) / kBuildBlock);
    VX_KL(k_tlas_prep, g, dim3(kBuildBlock), 0, s, in, n, tab, nb, xf, w2o, iblas, reinterpret_cast<float4*>(ibox), small);
    VX_KL(k_tlas_keys, g, dim3(kBuildBlock), 0, s, reinterpret_cast<const float4*>(ibox), n, small, keys);
}

void launch_tlas_tree(uint32_t n, const uint64_t* keys, const float* ibox, uint32_t* child, uint32_t* parent, uint32_t* range, uint32_t* arrived,
                      float* nodes, uint32_t* hgt, uint32_t* small, hipStream_t s)
{
    (void)hipMemsetAsync(parent, 0xFF, (size_t)(2ull * n - 1) * 4, s);
    (void)hipMemsetAsync(arrived, 0, (size_t)n * 4, s);
    launch_bvh_karras(keys, n, child, parent, range, s);
    VX_KL(k_tlas_bounds, dim3((n + kBuildBlock - 1) / kBuildBlock), dim3(kBuildBlock), 0, s, n, keys, reinterpret_cast<const float4*>(ibox), child,
          parent, arrived, reinterpret_cast<float4*>(nodes), hgt, small);
}

// ---- trace ----------------------------------------------------------------------------------------------------------------------------
namespace {

struct TlasParams {
    const float4* nodes;     // 2n-1 TLAS nodes
    const float4* w2o;       // 3 float4 rows per instance
    const float4* xf;        // object-to-world, 3 float4 rows per instance
    const uint32_t* iblas;   // BLAS of each instance, kNone = inactive
    const TlasBlas* tab;
    const uint32_t* small;   // [6] = the largest condition number (ordered uint)
    uint32_t ninst;          // 0: every ray misses
    uint32_t levels;         // LDS stack entries per lane (>= TLAS height bound + the largest BLAS height, >= 1)
    RayArgs io;
    float* bary_out;
    uint32_t* inst_out;
};

// a TLAS box: empty boxes (inactive instances, subtrees of them) are never entered
__device__ __forceinline__ bool tlas_enter(const float4& m0, const float4& m1, const SlabRay& R, float pad, float tlow, float best, float& t0)
{
    return m0.x <= m1.x && m0.y <= m1.y && m0.z <= m1.z && blas::box_enter(m0, m1, R, pad, tlow, best, t0);
}

}  // namespace

__global__ __launch_bounds__(kTlasBlock) void k_tlas_trace(TlasParams P)
{
    extern __shared__ uint32_t tlas_lds[];  // [level][lane]: the TLAS's entries below, the current BLAS's above them
    const uint32_t tid = threadIdx.x;
    const uint64_t r = (uint64_t)blockIdx.x * kTlasBlock + tid;
    const bool active = r < P.io.nrays;

    blas::Hit h;
    if (active) {
        float ox, oy, oz, dx, dy, dz;
        load_ray(P.io.rays == nullptr, r, P.io.rays, P.io.cam, ox, oy, oz, dx, dy, dz);
        SlabRay Rw;
        make_slab_ray(ox, oy, oz, dx, dy, dz, Rw);
        const float tmin = P.io.tmin, tlow = fmaxf(tmin, 0.0f);
        h.best = P.io.tmax_per_ray ? P.io.tmax_per_ray[r] : P.io.tmax;  // acceptance bound until the first hit
        const float rpad = kRayPad * ord2f(P.small[6]) * fabs_max3(ox, oy, oz);
        bool alive = P.ninst != 0 && !ray_nonfinite(ox, oy, oz, dx, dy, dz);  // a non-finite ray is a miss: no box, no instance sees it
        if (alive) {
            float t0;
            alive = tlas_enter(P.nodes[0], P.nodes[1], Rw, rpad, tlow, h.best, t0);
        }
        uint32_t cur = 0, sp = 0;
        while (alive) {
            const float4 n0 = P.nodes[2ull * cur], n1 = P.nodes[2ull * cur + 1];
            const uint32_t na = __float_as_uint(n0.w), nb = __float_as_uint(n1.w);
            if (nb & blas::kLeafBit) {
                const uint32_t b = P.iblas[na];
                if (b != blas::kNone) {  // enter instance na: its object-space ray, its side list, its BLAS from the root
                    const float4* W = P.w2o + 3ull * na;
                    const float4 W0 = W[0], W1 = W[1], W2 = W[2];
                    blas::Ray y;
                    y.ox = ((W0.x * ox + W0.y * oy) + W0.z * oz) + W0.w;
                    y.oy = ((W1.x * ox + W1.y * oy) + W1.z * oz) + W1.w;
                    y.oz = ((W2.x * ox + W2.y * oy) + W2.z * oz) + W2.w;
                    y.dx = (W0.x * dx + W0.y * dy) + W0.z * dz;
                    y.dy = (W1.x * dx + W1.y * dy) + W1.z * dz;
                    y.dz = (W2.x * dx + W2.y * dy) + W2.z * dz;
                    make_slab_ray(y.ox, y.oy, y.oz, y.dx, y.dy, y.dz, y.R);
                    y.tmin = tmin;
                    y.tlow = tlow;
                    const TlasBlas& D = P.tab[b];
                    const float4* bn = reinterpret_cast<const float4*>(D.nodes);
                    const float4* bt = reinterpret_cast<const float4*>(D.tris);
                    for (uint32_t k = 0; k < D.nill; ++k) blas::test_tri<blas::TieInst>(bt, D.ill[k], y, na, h);
                    // After a side-list hit with any_hit the BLAS is not entered, while k_bvh_trace still walks from its root to the first
                    // leaf.  The contract allows either (any_hit reports `shadowed` and an arbitrary accepted t).
                    bool enter = !(h.found && P.io.any_hit);
                    if (enter) {
                        float t0;
                        enter = blas::box_enter(bn[0], bn[1], y.R, D.pad, tlow, h.best, t0);
                    }
                    blas::descend<blas::TieInst, kTlasBlock>(bn, bt, y, D.pad, P.io.any_hit, tlas_lds, tid, sp, na, h, enter);
                }
                if (h.found && P.io.any_hit) break;
            } else {
                const float4 l0 = P.nodes[2ull * na], l1 = P.nodes[2ull * na + 1];
                const float4 r0 = P.nodes[2ull * nb], r1 = P.nodes[2ull * nb + 1];
                float tl, tr;
                const bool hl = tlas_enter(l0, l1, Rw, rpad, tlow, h.best, tl);
                const bool hr = tlas_enter(r0, r1, Rw, rpad, tlow, h.best, tr);
                if (hl && hr) {
                    const bool lnear = tl <= tr;
                    tlas_lds[sp * kTlasBlock + tid] = lnear ? nb : na;  // sp < TLAS height bound: one push per interior node of the path
                    ++sp;
                    cur = lnear ? na : nb;
                    continue;
                }
                if (hl || hr) { cur = hl ? na : nb; continue; }
            }
            bool next = false;
            while (sp > 0) {
                --sp;
                const uint32_t c = tlas_lds[sp * kTlasBlock + tid];
                if (h.found) {  // best has moved since the node was pushed
                    float t0;
                    if (!tlas_enter(P.nodes[2ull * c], P.nodes[2ull * c + 1], Rw, rpad, tlow, h.best, t0)) continue;
                }
                cur = c;
                next = true;
                break;
            }
            if (!next) break;
        }
    }
    const bool found = h.found;
    const float tt = found ? h.best : -1.0f;
    const uint32_t prim = found ? h.bp : blas::kNone;
    if (active) {
        if (P.io.t_out) P.io.t_out[r] = tt;
        if (P.io.prim_out) P.io.prim_out[r] = prim;
        if (P.inst_out) P.inst_out[r] = found ? h.bi : blas::kNone;
        if (P.io.shadowed_out) P.io.shadowed_out[r] = found ? 1 : 0;
        if (P.bary_out) { P.bary_out[2 * r] = found ? h.bu : 0.0f; P.bary_out[2 * r + 1] = found ? h.bv : 0.0f; }
        if (P.io.normal_out) {
            float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
            if (found) tlas_world_normal(P.tab, P.iblas, reinterpret_cast<const float*>(P.xf), h.bi, h.bk, n0, n1, n2);
            P.io.normal_out[3 * r] = n0; P.io.normal_out[3 * r + 1] = n1; P.io.normal_out[3 * r + 2] = n2;
        }
    }
    if (P.io.hits) compact_hit(found, r, prim, tt, P.io.hits, P.io.nhits);  // every lane of the workgroup gets here
}

float tlas_ray_pad() { return kRayPad; }

uint32_t tlas_height_bound(uint64_t n)
{
    if (n <= 1) return 0;
    uint32_t lg = 0;
    while ((1ull << lg) < n) ++lg;
    const uint64_t b = 30ull + lg;
    return (uint32_t)(n - 1 < b ? n - 1 : b);
}

void launch_tlas_trace(const TlasDev& T, const TraceIO& io, float* bary_out, uint32_t* inst_out, hipStream_t s)
{
    if (!io.nrays) return;
    TlasParams P;
    std::memset(&P, 0, sizeof(P));
    P.nodes = reinterpret_cast<const float4*>(T.nodes);
    P.w2o = reinterpret_cast<const float4*>(T.w2o);
    P.xf = reinterpret_cast<const float4*>(T.xf);
    P.iblas = T.iblas;
    P.tab = T.tab;
    P.small = T.small;
    P.ninst = T.ninst;
    P.levels = T.levels ? T.levels : 1u;
    set_ray_args(P.io, io, s);
    P.bary_out = bary_out;
    P.inst_out = inst_out;
    const size_t shmem = (size_t)P.levels * kTlasBlock * 4u;
    const uint64_t nblk = (io.nrays + kTlasBlock - 1) / kTlasBlock;
    VX_KL(k_tlas_trace, dim3((unsigned)nblk), dim3(kTlasBlock), shmem, s, P);
}

}  // namespace vx

namespace vx {
namespace {
struct TabChunk {
    TlasBlas e[8];
    uint32_t first, count;
};
// the BLAS table, 8 records per launch from a kernel argument: no host copy that must outlive the call, no synchronisation
__global__ __launch_bounds__(64) void k_tlas_table(TabChunk c, TlasBlas* out)
{
    if (threadIdx.x < c.count) out[c.first + threadIdx.x] = c.e[threadIdx.x];
}
}  // namespace

void launch_tlas_table(const TlasBlas* host, uint32_t nb, TlasBlas* dev, hipStream_t s)
{
    for (uint32_t f = 0; f < nb; f += 8) {
        TabChunk c;
        std::memset(&c, 0, sizeof(c));
        c.first = f;
        c.count = nb - f < 8 ? nb - f : 8;
        for (uint32_t k = 0; k < c.count; ++k) c.e[k] = host[f + k];
        VX_KL(k_tlas_table, dim3(1), dim3(64), 0, s, c, dev);
    }
}

}  // namespace vx
