// vx_meshmulti.hip -- multi-hit ray queries on the triangle mesh (vx_bvh_trace_multi*, vx_tlas_trace_multi*): vx_hitlist.h's contract over
// the triangles (the active (instance, triangle) pairs) whose pinned Moeller-Trumbore on ray r (on its object-space ray) gives u >= 0,
// u <= 1, v >= 0, u + v <= 1 -- the acceptance rule of k_bvh_trace / k_tlas_trace (include/voxhip.h) -- with the barycentrics as one more
// output, (0, 0) in an empty slot.  Every output is bit-equal to the brute force over all triangles (tests/mesh_multihit_ref.py).
//
// Enumeration.  The descent is k_bvh_trace's (vx_blas.h's for a BLAS under a TLAS), with the same box test -- blas::box_enter, the per-BVH
// pad, kTRel, the TLAS's per-ray pad -- and ONE change: where the first-hit kernels prune against the best t found so far, these prune
// against the list's bound().  A node is entered on t0 <= bound (an equal t may carry a smaller key), the nearer child first, a popped node
// re-tested once the bound has moved.  The superset argument of the first-hit kernels carries over with `bound` in the
// place of `best`: it is stated per accepted (ray, triangle) pair -- the pair's t lies in the widened slab interval of every box above the
// triangle -- and never uses that the pair is the closest one.  Its two documented gaps carry over with it: triangles whose rounding no box
// bounds are on the build's side list and tested one by one before the descent; under a TLAS that list is tested only when the ray reaches
// the instance's leaf.
//
// Every triangle counts once.  A side-listed triangle also sits in a leaf; the build marks it (the w lane of the second float4 of its 48-byte
// copy, k_bvh_bounds), and the leaf loop skips marked triangles.  Each leaf is visited at most once per ray and holds each of its triangles
// once, so counts need no further de-duplication.
//
// Barycentrics are not kept in the list: at write-out (u, v) of a kept hit are evaluated again from its leaf-order position with the same
// expressions on the same (object-space) ray, bit-equal by construction.  The traversal stack [level][lane] follows the list in LDS, sized
// by the built height (TLAS: its height bound plus the tallest BLAS).
#include "vx_hitlist.h"
#include "vx_blas.h"

#include <cstring>

#pragma clang fp contract(off)

namespace vx {

namespace {

struct BvhMultiParams {
    const float4* nodes;
    const float4* tris;
    const uint32_t* ill;
    uint32_t nill;
    uint32_t ntri;  // 0: every ray misses
    float pad;
    MultiOut o;
};

struct TlasMultiParams {
    const float4* nodes;
    const float4* w2o;
    const uint32_t* iblas;
    const TlasBlas* tab;
    const uint32_t* small;  // [6] = the largest condition number (ordered uint)
    uint32_t ninst;         // 0: every ray misses
    float ray_pad;          // tlas_ray_pad()
    MultiOut o;
};

// Moeller-Trumbore of one triangle copy on ray y: blas::test_tri's expressions, in its order; true iff accepted with t <= tmax
__device__ __forceinline__ bool mt_eval(const float4& A, const float4& B, const float4& Cc, const blas::Ray& y, float tmax, float& t, float& u, float& v)
{
    const float ox = y.ox, oy = y.oy, oz = y.oz, dx = y.dx, dy = y.dy, dz = y.dz;
    const float e1x = B.x - A.x, e1y = B.y - A.y, e1z = B.z - A.z;
    const float e2x = Cc.x - A.x, e2y = Cc.y - A.y, e2z = Cc.z - A.z;
    const float px = dy * e2z - dz * e2y, py = dz * e2x - dx * e2z, pz = dx * e2y - dy * e2x;
    const float det = (e1x * px + e1y * py) + e1z * pz;
    const float inv = 1.0f / det;
    const float sx = ox - A.x, sy = oy - A.y, sz = oz - A.z;
    u = ((sx * px + sy * py) + sz * pz) * inv;
    const float qx = sy * e1z - sz * e1y, qy = sz * e1x - sx * e1z, qz = sx * e1y - sy * e1x;
    v = ((dx * qx + dy * qy) + dz * qz) * inv;
    t = ((e2x * qx + e2y * qy) + e2z * qz) * inv;
    return u >= 0.0f && u <= 1.0f && v >= 0.0f && u + v <= 1.0f && t > 0.0f && t >= y.tmin && t <= tmax;
}

// the object-space ray of an instance, as k_tlas_trace forms it: o' = ((w0*ox + w1*oy) + w2*oz) + w3, d' = (w0*dx + w1*dy) + w2*dz per row
__device__ __forceinline__ void object_ray(const float4* __restrict__ W, float ox, float oy, float oz, float dx, float dy, float dz, float tmin,
                                           float tlow, blas::Ray& y)
{
    const float4 W0 = W[0], W1 = W[1], W2 = W[2];
    y.ox = ((W0.x * ox + W0.y * oy) + W0.z * oz) + W0.w;
    y.oy = ((W1.x * ox + W1.y * oy) + W1.z * oz) + W1.w;
    y.oz = ((W2.x * ox + W2.y * oy) + W2.z * oz) + W2.w;
    y.dx = (W0.x * dx + W0.y * dy) + W0.z * dz;
    y.dy = (W1.x * dx + W1.y * dy) + W1.z * dz;
    y.dz = (W2.x * dx + W2.y * dy) + W2.z * dz;
    make_slab_ray(y.ox, y.oy, y.oz, y.dx, y.dy, y.dz, y.R);
    y.tmin = tmin;
    y.tlow = tlow;
}

// All accepted triangles of one BVH on ray y into L: the side list, then blas::descend's walk from the root with L.bound() in the place
// of the best t.  stack: LDS [level][lane], entries sp0 .. sp0 + the BVH's height - 1.
template <int KC, bool kInst>
__device__ __forceinline__ void blas_multi(const float4* __restrict__ nodes, const float4* __restrict__ tris, const uint32_t* __restrict__ ill, uint32_t nill,
                                           const blas::Ray& y, float pad, uint32_t* stack, uint32_t sp0, uint32_t inst, HitList<KC, true, kInst>& L)
{
    const uint32_t lane = L.lane;
    for (uint32_t i = 0; i < nill; ++i) {
        const uint32_t k = ill[i];
        const float4 A = tris[3ull * k], B = tris[3ull * k + 1], Cc = tris[3ull * k + 2];
        float t, u, v;
        if (mt_eval(A, B, Cc, y, L.tmax, t, u, v)) L.offer(t, __float_as_uint(A.w), k, inst);
    }
    float t0;
    bool alive = blas::box_enter(nodes[0], nodes[1], y.R, pad, y.tlow, L.bound(), t0);
    uint32_t cur = 0, sp = sp0;
    while (alive) {
        const float4 n0 = nodes[2ull * cur], n1 = nodes[2ull * cur + 1];
        const uint32_t na = __float_as_uint(n0.w), nb = __float_as_uint(n1.w);
        if (nb & blas::kLeafBit) {
            const uint32_t end = na + (nb & ~blas::kLeafBit);
            for (uint32_t k = na; k < end; ++k) {
                const float4 A = tris[3ull * k], B = tris[3ull * k + 1], Cc = tris[3ull * k + 2];
                if (__float_as_uint(B.w)) continue;  // on the side list: tested above
                float t, u, v;
                if (mt_eval(A, B, Cc, y, L.tmax, t, u, v)) L.offer(t, __float_as_uint(A.w), k, inst);
            }
        } else {
            const float4 l0 = nodes[2ull * na], l1 = nodes[2ull * na + 1];
            const float4 r0 = nodes[2ull * nb], r1 = nodes[2ull * nb + 1];
            const float bound = L.bound();
            float tl, tr;
            const bool hl = blas::box_enter(l0, l1, y.R, pad, y.tlow, bound, tl);
            const bool hr = blas::box_enter(r0, r1, y.R, pad, y.tlow, bound, tr);
            if (hl && hr) {
                const bool lnear = tl <= tr;
                stack[sp * kMultiBlock + lane] = lnear ? nb : na;  // sp < sp0 + height: one push per interior node of the path
                ++sp;
                cur = lnear ? na : nb;
                continue;
            }
            if (hl || hr) { cur = hl ? na : nb; continue; }
        }
        bool next = false;
        while (sp > sp0) {
            --sp;
            const uint32_t c = stack[sp * kMultiBlock + lane];
            if (L.tightened()) {  // the bound may have moved since the node was pushed
                if (!blas::box_enter(nodes[2ull * c], nodes[2ull * c + 1], y.R, pad, y.tlow, L.bound(), t0)) continue;
            }
            cur = c;
            next = true;
            break;
        }
        if (!next) break;
    }
}

// a TLAS box: empty boxes (inactive instances, subtrees of them) are never entered (k_tlas_trace's tlas_enter)
__device__ __forceinline__ bool tlas_box_enter(const float4& m0, const float4& m1, const SlabRay& R, float pad, float tlow, float bound, float& t0)
{
    return m0.x <= m1.x && m0.y <= m1.y && m0.z <= m1.z && blas::box_enter(m0, m1, R, pad, tlow, bound, t0);
}

}  // namespace

template <int KC>
__global__ __launch_bounds__(kMultiBlock) void k_bvh_multihit(const BvhMultiParams P)
{
    __shared__ uint32_t keys[HitList<KC, true, false>::kWords];
    extern __shared__ uint32_t mm_stack[];  // [level][lane]
    const uint32_t lane = threadIdx.x;
    const MultiOut& o = P.o;
    const uint32_t K = o.K;
    for (uint64_t r = (uint64_t)blockIdx.x * kMultiBlock + lane; r < o.io.nrays; r += (uint64_t)gridDim.x * kMultiBlock) {
        blas::Ray y;
        load_ray(o.io.rays == nullptr, r, o.io.rays, o.io.cam, y.ox, y.oy, y.oz, y.dx, y.dy, y.dz);
        make_slab_ray(y.ox, y.oy, y.oz, y.dx, y.dy, y.dz, y.R);
        y.tmin = o.io.tmin;
        y.tlow = fmaxf(y.tmin, 0.0f);
        HitList<KC, true, false> L;
        list_begin(L, keys, lane, o, r);
        // (a non-finite ray is a miss: an empty list, before the side list or a box sees it)
        if (P.ntri && !ray_nonfinite(y.ox, y.oy, y.oz, y.dx, y.dy, y.dz)) blas_multi(P.nodes, P.tris, P.ill, P.nill, y, P.pad, mm_stack, 0u, 0u, L);
        L.write(o, r);
        if (o.bary_out) {
            for (uint32_t j = 0; j < K; ++j) {
                float t, u = 0.0f, v = 0.0f;
                if (j < L.n) {
                    const uint32_t k = L.at(L.kFieldPos, j);
                    (void)mt_eval(P.tris[3ull * k], P.tris[3ull * k + 1], P.tris[3ull * k + 2], y, L.tmax, t, u, v);
                }
                o.bary_out[(r * K + j) * 2] = u;
                o.bary_out[(r * K + j) * 2 + 1] = v;
            }
        }
    }
}

template <int KC>
__global__ __launch_bounds__(kMultiBlock) void k_tlas_multihit(const TlasMultiParams P)
{
    __shared__ uint32_t keys[HitList<KC, true, true>::kWords];
    extern __shared__ uint32_t mm_stack[];  // [level][lane]: the TLAS's entries below, the current BLAS's above them
    const uint32_t lane = threadIdx.x;
    const MultiOut& o = P.o;
    const uint32_t K = o.K;
    for (uint64_t r = (uint64_t)blockIdx.x * kMultiBlock + lane; r < o.io.nrays; r += (uint64_t)gridDim.x * kMultiBlock) {
        float ox, oy, oz, dx, dy, dz;
        load_ray(o.io.rays == nullptr, r, o.io.rays, o.io.cam, ox, oy, oz, dx, dy, dz);
        SlabRay Rw;
        make_slab_ray(ox, oy, oz, dx, dy, dz, Rw);
        const float tmin = o.io.tmin, tlow = fmaxf(tmin, 0.0f);
        HitList<KC, true, true> L;
        list_begin(L, keys, lane, o, r);
        const float rpad = P.ninst ? P.ray_pad * ord2f(P.small[6]) * fmaxf(fmaxf(fabsf(ox), fabsf(oy)), fabsf(oz)) : 0.0f;
        float t0;
        // (a non-finite ray is a miss: an empty list, before a box or an instance sees it)
        bool alive = P.ninst != 0 && !ray_nonfinite(ox, oy, oz, dx, dy, dz) && tlas_box_enter(P.nodes[0], P.nodes[1], Rw, rpad, tlow, L.bound(), t0);
        uint32_t cur = 0, sp = 0;
        while (alive) {
            const float4 n0 = P.nodes[2ull * cur], n1 = P.nodes[2ull * cur + 1];
            const uint32_t na = __float_as_uint(n0.w), nb = __float_as_uint(n1.w);
            if (nb & blas::kLeafBit) {
                const uint32_t b = P.iblas[na];
                if (b != blas::kNone) {  // instance na: its object-space ray, its side list, its BLAS from the root
                    blas::Ray y;
                    object_ray(P.w2o + 3ull * na, ox, oy, oz, dx, dy, dz, tmin, tlow, y);
                    const TlasBlas& D = P.tab[b];
                    blas_multi(reinterpret_cast<const float4*>(D.nodes), reinterpret_cast<const float4*>(D.tris), D.ill, D.nill, y, D.pad, mm_stack, sp, na, L);
                }
            } else {
                const float4 l0 = P.nodes[2ull * na], l1 = P.nodes[2ull * na + 1];
                const float4 r0 = P.nodes[2ull * nb], r1 = P.nodes[2ull * nb + 1];
                const float bound = L.bound();
                float tl, tr;
                const bool hl = tlas_box_enter(l0, l1, Rw, rpad, tlow, bound, tl);
                const bool hr = tlas_box_enter(r0, r1, Rw, rpad, tlow, bound, tr);
                if (hl && hr) {
                    const bool lnear = tl <= tr;
                    mm_stack[sp * kMultiBlock + lane] = lnear ? nb : na;  // sp < TLAS height bound: one push per interior node of the path
                    ++sp;
                    cur = lnear ? na : nb;
                    continue;
                }
                if (hl || hr) { cur = hl ? na : nb; continue; }
            }
            bool next = false;
            while (sp > 0) {
                --sp;
                const uint32_t c = mm_stack[sp * kMultiBlock + lane];
                if (L.tightened()) {  // the bound may have moved since the node was pushed
                    if (!tlas_box_enter(P.nodes[2ull * c], P.nodes[2ull * c + 1], Rw, rpad, tlow, L.bound(), t0)) continue;
                }
                cur = c;
                next = true;
                break;
            }
            if (!next) break;
        }
        L.write(o, r);
        for (uint32_t j = 0; j < K; ++j) {
            const bool have = j < L.n;
            if (o.inst_out) o.inst_out[r * K + j] = have ? L.at(L.kFieldInst, j) : blas::kNone;
            if (o.bary_out) {
                float t, u = 0.0f, v = 0.0f;
                if (have) {  // the hit's own object-space ray again, then its triangle
                    const uint32_t inst = L.at(L.kFieldInst, j), k = L.at(L.kFieldPos, j);
                    blas::Ray y;
                    object_ray(P.w2o + 3ull * inst, ox, oy, oz, dx, dy, dz, tmin, tlow, y);
                    const float4* bt = reinterpret_cast<const float4*>(P.tab[P.iblas[inst]].tris);
                    (void)mt_eval(bt[3ull * k], bt[3ull * k + 1], bt[3ull * k + 2], y, L.tmax, t, u, v);
                }
                o.bary_out[(r * K + j) * 2] = u;
                o.bary_out[(r * K + j) * 2 + 1] = v;
            }
        }
    }
}

void launch_bvh_multihit(const float* nodes, const float* tris, const uint32_t* ill, uint32_t nill, uint32_t ntri, uint32_t height, float extent,
                         float coord_max, const TraceIO& io, const MultiIO& m, hipStream_t s)
{
    if (!io.nrays || !m.K) return;
    BvhMultiParams P;
    std::memset(&P, 0, sizeof(P));
    P.nodes = reinterpret_cast<const float4*>(nodes);
    P.tris = reinterpret_cast<const float4*>(tris);
    P.ill = ill;
    P.ntri = nodes ? ntri : 0;
    P.nill = nodes ? nill : 0;
    P.pad = bvh_pad(extent, coord_max);
    set_multi_out(P.o, io, m, s);
    const size_t shmem = (size_t)(height ? height : 1u) * kMultiBlock * 4u;  // the stack: one entry per level and lane
    VX_MULTI_LAUNCH(k_bvh_multihit, io.nrays, m.K, shmem, s, P);
}

void launch_tlas_multihit(const TlasDev& T, const TraceIO& io, const MultiIO& m, hipStream_t s)
{
    if (!io.nrays || !m.K) return;
    TlasMultiParams P;
    std::memset(&P, 0, sizeof(P));
    P.nodes = reinterpret_cast<const float4*>(T.nodes);
    P.w2o = reinterpret_cast<const float4*>(T.w2o);
    P.iblas = T.iblas;
    P.tab = T.tab;
    P.small = T.small;
    P.ninst = T.ninst;
    P.ray_pad = tlas_ray_pad();
    set_multi_out(P.o, io, m, s);
    const size_t shmem = (size_t)(T.levels ? T.levels : 1u) * kMultiBlock * 4u;  // TLAS height bound + the tallest BLAS
    VX_MULTI_LAUNCH(k_tlas_multihit, io.nrays, m.K, shmem, s, P);
}

}  // namespace vx
