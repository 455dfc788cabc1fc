// vx_meshmulti.hip -- multi-hit ray queries on the triangle mesh (vx_bvh_trace_multi*, vx_tlas_trace_multi*): per ray the first K accepted
// triangles in (t, prim) order -- (t, instance, prim) on a TLAS -- their barycentrics, and the number of all accepted triangles, under the
// acceptance rule and with the pinned Moeller-Trumbore of k_bvh_trace / k_tlas_trace (include/voxhip.h).
//
// Contract: A(r) = the triangles (the active (instance, triangle) pairs) whose pinned Moeller-Trumbore on ray r (on its object-space ray) gives
// u >= 0, u <= 1, v >= 0, u + v <= 1, t > 0, tmin <= t <= tmax (or tmax_per_ray[r]) and, with a cursor, a key strictly after the cursor's;
// sorted by key with t compared as float.  Slots j < min(K, |A|) hold the j-th element, the others -1.0f / 0xFFFFFFFF / (0, 0); count = |A|.
// Every output is bit-equal to the brute force over all triangles (tests/mesh_multihit_ref.py).
//
// Enumeration.  The descent is k_bvh_trace's (vx_blas.h's for a BLAS under a TLAS), with the same box test -- blas::box_enter, the per-BVH
// pad, kTRel, the TLAS's per-ray pad -- and ONE change: where the first-hit kernels prune against the best t found so far, these prune
// against `bound` = the ray's tmax while the count is wanted or the list is not yet full, the K-th kept t otherwise.  A node is entered on
// t0 <= bound (an equal t may carry a smaller key), the nearer child first, a popped node re-tested once the bound has moved.  The superset
// argument of the first-hit kernels carries over with `bound` in the place of `best`: it is stated per accepted
// (ray, triangle) pair -- the pair's t lies in the widened slab interval of every box above the triangle -- and never uses that the pair is
// the closest one.  Its two documented gaps carry over with it: triangles whose rounding no box bounds are on the build's side list and
// tested one by one before the descent; under a TLAS that list is tested only when the ray reaches the instance's leaf.
//
// Every triangle counts once.  A side-listed triangle also sits in a leaf; the build marks it (the w lane of the second float4 of its 48-byte
// copy, k_bvh_bounds), and the leaf loop skips marked triangles.  Each leaf is visited at most once per ray and holds each of its triangles
// once, so counts need no further de-duplication.
//
// The K nearest hits of a lane live in LDS, [field][slot][lane]: t bits, prim, leaf-order position, and the instance under a TLAS -- 12 / 16
// bytes per slot, consecutive lanes on consecutive banks.  Accepted t are positive floats, so their bits order as they do.  Insertion from
// the tail.  Barycentrics are not kept: at write-out (u, v) of a kept hit are evaluated again from its leaf-order position with the same
// expressions on the same (object-space) ray, bit-equal by construction.  The traversal stack [level][lane] follows the hit buffer in LDS,
// sized by the built height (TLAS: its height bound plus the tallest BLAS).
//
// One ray per lane, workgroups of one wave, no barrier, a grid-stride loop over the batch.
#include "vx_internal.h"
#include "vx_ray.h"
#include "vx_blas.h"

#include <cstring>

#pragma clang fp contract(off)

namespace vx {

#define VX_KL(kern, grid, block, shmem, stream, ...)                         \
    do {                                                                     \
        ProfScope ps_(#kern, stream);                                        \
        hipLaunchKernelGGL(kern, grid, block, shmem, stream, __VA_ARGS__);   \
    } while (0)

namespace {

constexpr uint32_t kMmBlock = 64;  // lanes per workgroup: one wave

// what both kernels take besides their structure: the list length, the optional outputs and cursor, the ray batch (t_out / prim_out hold K
// entries per ray)
struct MultiOut {
    uint32_t K;
    uint32_t* count;               // optional
    float* bary_out;               // optional, 2 per slot
    uint32_t* inst_out;            // optional (TLAS)
    const float* after_t;          // optional cursor (all of its arrays or none)
    const uint32_t* after_inst;    // (TLAS)
    const uint32_t* after_prim;
    RayArgs io;
};

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

enum : uint32_t { kFieldT = 0, kFieldPrim = 1, kFieldPos = 2, kFieldInst = 3 };

// One lane's list: the K smallest keys (t, instance, prim) seen so far, sorted, in LDS; the count of all keys offered behind the cursor.
// kInst false: one BVH, the instance part is 0 everywhere and not stored.
template <int KC, bool kInst>
struct HitList {
    uint32_t* keys;  // [field][slot][lane]
    uint32_t lane, K;
    uint32_t n = 0, total = 0;
    bool counting;
    float tmax;              // the acceptance bound
    float kth = INFINITY;    // the K-th kept t once the list is full
    float cur_t;             // the cursor; (-1, ...) = none
    uint32_t cur_i, cur_p;

    __device__ __forceinline__ uint32_t& at(uint32_t f, uint32_t s) const { return keys[(f * KC + s) * kMmBlock + lane]; }
    // no accepted hit behind this t can change the outputs
    __device__ __forceinline__ float bound() const { return (counting || n < K) ? tmax : kth; }
    __device__ __forceinline__ bool tightened() const { return !counting && n == K; }
    __device__ __forceinline__ bool before(uint32_t tb, uint32_t inst, uint32_t prim, uint32_t s) const
    {
        const uint32_t st = at(kFieldT, s);
        if (tb != st) return tb < st;
        if (kInst) {
            const uint32_t si = at(kFieldInst, s);
            if (inst != si) return inst < si;
        }
        return prim < at(kFieldPrim, s);
    }
    // an accepted hit: triangle prim of instance inst at leaf-order position pos
    __device__ __forceinline__ void offer(float t, uint32_t inst, uint32_t prim, uint32_t pos)
    {
        if (!(t > cur_t || (t == cur_t && (inst > cur_i || (inst == cur_i && prim > cur_p))))) return;  // not strictly after the cursor
        ++total;
        const uint32_t tb = __float_as_uint(t);
        if (n == K && !before(tb, inst, prim, K - 1u)) return;
        uint32_t j = n < K ? n : K - 1u;  // where the list's new tail goes: the K-th entry falls out of a full list
        while (j > 0u && before(tb, inst, prim, j - 1u)) {
            at(kFieldT, j) = at(kFieldT, j - 1u);
            at(kFieldPrim, j) = at(kFieldPrim, j - 1u);
            at(kFieldPos, j) = at(kFieldPos, j - 1u);
            if (kInst) at(kFieldInst, j) = at(kFieldInst, j - 1u);
            --j;
        }
        at(kFieldT, j) = tb;
        at(kFieldPrim, j) = prim;
        at(kFieldPos, j) = pos;
        if (kInst) at(kFieldInst, j) = inst;
        if (n < K) ++n;
        if (n == K) kth = __uint_as_float(at(kFieldT, K - 1u));
    }
};

// All accepted triangles of one BVH on ray y into L: the side list, then blas::descend's walk from the root with L.bound() in the place
// of the best t.  stack: LDS [level][lane], entries sp0 .. sp0 + the BVH's height - 1.
template <int KC, bool kInst>
__device__ __forceinline__ void blas_multi(const float4* __restrict__ nodes, const float4* __restrict__ tris, const uint32_t* __restrict__ ill, uint32_t nill,
                                           const blas::Ray& y, float pad, uint32_t* stack, uint32_t sp0, uint32_t inst, HitList<KC, kInst>& L)
{
    const uint32_t lane = L.lane;
    for (uint32_t i = 0; i < nill; ++i) {
        const uint32_t k = ill[i];
        const float4 A = tris[3ull * k], B = tris[3ull * k + 1], Cc = tris[3ull * k + 2];
        float t, u, v;
        if (mt_eval(A, B, Cc, y, L.tmax, t, u, v)) L.offer(t, inst, __float_as_uint(A.w), k);
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
                if (mt_eval(A, B, Cc, y, L.tmax, t, u, v)) L.offer(t, inst, __float_as_uint(A.w), k);
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
                stack[sp * kMmBlock + lane] = lnear ? nb : na;  // sp < sp0 + height: one push per interior node of the path
                ++sp;
                cur = lnear ? na : nb;
                continue;
            }
            if (hl || hr) { cur = hl ? na : nb; continue; }
        }
        bool next = false;
        while (sp > sp0) {
            --sp;
            const uint32_t c = stack[sp * kMmBlock + lane];
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

template <int KC, bool kInst>
__device__ __forceinline__ void list_begin(HitList<KC, kInst>& L, uint32_t* keys, uint32_t lane, const MultiOut& o, uint64_t r)
{
    L.keys = keys;
    L.lane = lane;
    L.K = o.K;
    L.counting = o.count != nullptr;
    L.tmax = o.io.tmax_per_ray ? o.io.tmax_per_ray[r] : o.io.tmax;
    L.cur_t = o.after_t ? o.after_t[r] : -1.0f;
    L.cur_i = kInst && o.after_inst ? o.after_inst[r] : 0u;
    L.cur_p = o.after_prim ? o.after_prim[r] : 0u;
}

}  // namespace

template <int KC>
__global__ __launch_bounds__(kMmBlock) void k_bvh_multihit(const BvhMultiParams P)
{
    __shared__ uint32_t keys[3 * KC * kMmBlock];
    extern __shared__ uint32_t mm_stack[];  // [level][lane]
    const uint32_t lane = threadIdx.x;
    const MultiOut& o = P.o;
    const uint32_t K = o.K;
    for (uint64_t r = (uint64_t)blockIdx.x * kMmBlock + lane; r < o.io.nrays; r += (uint64_t)gridDim.x * kMmBlock) {
        blas::Ray y;
        load_ray(o.io.rays == nullptr, r, o.io.rays, o.io.cam, y.ox, y.oy, y.oz, y.dx, y.dy, y.dz);
        make_slab_ray(y.ox, y.oy, y.oz, y.dx, y.dy, y.dz, y.R);
        y.tmin = o.io.tmin;
        y.tlow = fmaxf(y.tmin, 0.0f);
        HitList<KC, false> L;
        list_begin(L, keys, lane, o, r);
        // (a non-finite ray is a miss: an empty list, before the side list or a box sees it)
        if (P.ntri && !ray_nonfinite(y.ox, y.oy, y.oz, y.dx, y.dy, y.dz)) blas_multi(P.nodes, P.tris, P.ill, P.nill, y, P.pad, mm_stack, 0u, 0u, L);
        // ---- outputs: K entries per ray, ray-major
        for (uint32_t j = 0; j < K; ++j) {
            const bool have = j < L.n;
            if (o.io.t_out) o.io.t_out[r * K + j] = have ? __uint_as_float(L.at(kFieldT, j)) : -1.0f;
            if (o.io.prim_out) o.io.prim_out[r * K + j] = have ? L.at(kFieldPrim, j) : blas::kNone;
            if (o.bary_out) {
                float t, u = 0.0f, v = 0.0f;
                if (have) {
                    const uint32_t k = L.at(kFieldPos, j);
                    (void)mt_eval(P.tris[3ull * k], P.tris[3ull * k + 1], P.tris[3ull * k + 2], y, L.tmax, t, u, v);
                }
                o.bary_out[(r * K + j) * 2] = u;
                o.bary_out[(r * K + j) * 2 + 1] = v;
            }
        }
        if (o.count) o.count[r] = L.total;
    }
}

template <int KC>
__global__ __launch_bounds__(kMmBlock) void k_tlas_multihit(const TlasMultiParams P)
{
    __shared__ uint32_t keys[4 * KC * kMmBlock];
    extern __shared__ uint32_t mm_stack[];  // [level][lane]: the TLAS's entries below, the current BLAS's above them
    const uint32_t lane = threadIdx.x;
    const MultiOut& o = P.o;
    const uint32_t K = o.K;
    for (uint64_t r = (uint64_t)blockIdx.x * kMmBlock + lane; r < o.io.nrays; r += (uint64_t)gridDim.x * kMmBlock) {
        float ox, oy, oz, dx, dy, dz;
        load_ray(o.io.rays == nullptr, r, o.io.rays, o.io.cam, ox, oy, oz, dx, dy, dz);
        SlabRay Rw;
        make_slab_ray(ox, oy, oz, dx, dy, dz, Rw);
        const float tmin = o.io.tmin, tlow = fmaxf(tmin, 0.0f);
        HitList<KC, true> L;
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
                    mm_stack[sp * kMmBlock + lane] = lnear ? nb : na;  // sp < TLAS height bound: one push per interior node of the path
                    ++sp;
                    cur = lnear ? na : nb;
                    continue;
                }
                if (hl || hr) { cur = hl ? na : nb; continue; }
            }
            bool next = false;
            while (sp > 0) {
                --sp;
                const uint32_t c = mm_stack[sp * kMmBlock + lane];
                if (L.tightened()) {  // the bound may have moved since the node was pushed
                    if (!tlas_box_enter(P.nodes[2ull * c], P.nodes[2ull * c + 1], Rw, rpad, tlow, L.bound(), t0)) continue;
                }
                cur = c;
                next = true;
                break;
            }
            if (!next) break;
        }
        // ---- outputs: K entries per ray, ray-major
        for (uint32_t j = 0; j < K; ++j) {
            const bool have = j < L.n;
            if (o.io.t_out) o.io.t_out[r * K + j] = have ? __uint_as_float(L.at(kFieldT, j)) : -1.0f;
            if (o.io.prim_out) o.io.prim_out[r * K + j] = have ? L.at(kFieldPrim, j) : blas::kNone;
            if (o.inst_out) o.inst_out[r * K + j] = have ? L.at(kFieldInst, j) : blas::kNone;
            if (o.bary_out) {
                float t, u = 0.0f, v = 0.0f;
                if (have) {  // the hit's own object-space ray again, then its triangle
                    const uint32_t inst = L.at(kFieldInst, j), k = L.at(kFieldPos, j);
                    blas::Ray y;
                    object_ray(P.w2o + 3ull * inst, ox, oy, oz, dx, dy, dz, tmin, tlow, y);
                    const float4* bt = reinterpret_cast<const float4*>(P.tab[P.iblas[inst]].tris);
                    (void)mt_eval(bt[3ull * k], bt[3ull * k + 1], bt[3ull * k + 2], y, L.tmax, t, u, v);
                }
                o.bary_out[(r * K + j) * 2] = u;
                o.bary_out[(r * K + j) * 2 + 1] = v;
            }
        }
        if (o.count) o.count[r] = L.total;
    }
}

namespace {

void fill_out(MultiOut& o, const TraceIO& io, const MeshMultiIO& m, hipStream_t s)
{
    o.K = m.K;
    o.count = m.count;
    o.bary_out = m.bary;
    o.inst_out = m.instance;
    o.after_t = m.after_t;
    o.after_inst = m.after_instance;
    o.after_prim = m.after_prim;
    set_ray_args(o.io, io, s);
}

dim3 multi_grid(uint64_t nrays)
{
    uint64_t nblk = (nrays + kMmBlock - 1) / kMmBlock;
    if (nblk > (1ull << 22)) nblk = 1ull << 22;  // grid-stride beyond 2^28 rays
    return dim3((unsigned)nblk);
}

}  // namespace

void launch_bvh_multihit(const float* nodes, const float* tris, const uint32_t* ill, uint32_t nill, uint32_t ntri, uint32_t height, float extent,
                         float coord_max, const TraceIO& io, const MeshMultiIO& m, hipStream_t s)
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
    fill_out(P.o, io, m, s);
    const size_t shmem = (size_t)(height ? height : 1u) * kMmBlock * 4u;  // the stack: one entry per level and lane
    const dim3 grid = multi_grid(io.nrays), block(kMmBlock);
    if (m.K <= 4) VX_KL(k_bvh_multihit<4>, grid, block, shmem, s, P);
    else if (m.K <= 8) VX_KL(k_bvh_multihit<8>, grid, block, shmem, s, P);
    else if (m.K <= 16) VX_KL(k_bvh_multihit<16>, grid, block, shmem, s, P);
    else VX_KL(k_bvh_multihit<32>, grid, block, shmem, s, P);
}

void launch_tlas_multihit(const TlasDev& T, const TraceIO& io, const MeshMultiIO& m, hipStream_t s)
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
    fill_out(P.o, io, m, s);
    const size_t shmem = (size_t)(T.levels ? T.levels : 1u) * kMmBlock * 4u;  // TLAS height bound + the tallest BLAS
    const dim3 grid = multi_grid(io.nrays), block(kMmBlock);
    if (m.K <= 4) VX_KL(k_tlas_multihit<4>, grid, block, shmem, s, P);
    else if (m.K <= 8) VX_KL(k_tlas_multihit<8>, grid, block, shmem, s, P);
    else if (m.K <= 16) VX_KL(k_tlas_multihit<16>, grid, block, shmem, s, P);
    else VX_KL(k_tlas_multihit<32>, grid, block, shmem, s, P);
}

}  // namespace vx
