// vx_hitlist.h -- what the multi-hit kernels share: one lane's list of the K nearest hits, the block of kernel arguments that describes the
// query and the write-out (k_octree_multihit, k_bvh_multihit, k_tlas_multihit), and the launch (those three and k_multihit).  The kernels
// keep their enumeration (the octree descent, the BVH / TLAS descent) and the argument why it visits every accepted primitive.  k_multihit
// (vx_multihit.hip) implements the same contract on its own text: on this list it ran 2-4 % slower.
//
// Contract (include/voxhip.h), the same on every structure.  A(r) = the primitives ray r accepts -- t > 0, tmin <= t <= tmax (or
// tmax_per_ray[r]), each counted once -- whose key lies STRICTLY after the cursor's, sorted by key.  The key is (t, prim), on a TLAS
// (t, instance, prim), with t compared as float; the cursor (-1, ...) means none.  Slots j < min(K, |A|) of a ray's outputs hold the j-th
// element, the others -1.0f / 0xFFFFFFFF; count = |A|.  Every output is bit-equal to the brute force over all primitives.
//
// The list.  A lane keeps the K smallest keys offered so far, sorted, in LDS as [field][slot][lane] -- consecutive lanes on consecutive
// banks -- with the fields t bits, prim, then the leaf-order position (BVH, TLAS: the barycentrics are evaluated again from it at write-out)
// and the instance (TLAS).  Accepted t are positive floats, so their bits order as they do.  Insertion is from the tail: the enumerations
// run roughly front to back, almost every hit lands there.  The K-th entry falls out of a full list.
//
// Pruning.  bound() is the t behind which no accepted hit can change the outputs: the ray's tmax while the count is wanted or the list is
// not full, the K-th kept t otherwise.  An enumeration drops whatever starts at t0 > bound() -- strictly: an equal t may still carry a
// smaller key -- and tests again what it had queued before the list filled (tightened()).
//
// One ray per lane, workgroups of one wave (no barrier anywhere), a grid-stride loop over the batch; the list holds KC = 4, 8, 16 or 32 >= K
// slots, chosen at launch: KC * 64 lanes * 4 B per field.
#pragma once
#include "vx_internal.h"
#include "vx_ray.h"

namespace vx {

constexpr uint32_t kMultiBlock = 64;  // lanes per workgroup: one wave

// The query, as a block of the kernel arguments: the list length, the optional outputs and cursor, the ray batch (t_out / prim_out and the
// mesh kernels' bary_out / inst_out hold K entries per ray, ray-major).
struct MultiOut {
    uint32_t K;
    uint32_t* count;               // optional
    float* bary_out;               // optional, 2 per slot (BVH, TLAS)
    uint32_t* inst_out;            // optional (TLAS)
    const float* after_t;          // optional cursor (all of its arrays or none)
    const uint32_t* after_inst;    // (TLAS)
    const uint32_t* after_prim;
    RayArgs io;
};

inline void set_multi_out(MultiOut& o, const TraceIO& io, const MultiIO& m, hipStream_t s)
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

inline dim3 multi_grid(uint64_t nrays)
{
    uint64_t nblk = (nrays + kMultiBlock - 1) / kMultiBlock;
    if (nblk > (1ull << 22)) nblk = 1ull << 22;  // grid-stride beyond 2^28 rays
    return dim3((unsigned)nblk);
}

// kern<KC> for the smallest KC >= K over the batch, P its argument block
#define VX_MULTI_LAUNCH(kern, nrays, K, shmem, stream, P)                                \
    do {                                                                                 \
        const dim3 grid_ = multi_grid(nrays), block_(kMultiBlock);                       \
        if ((K) <= 4) VX_KL(kern<4>, grid_, block_, shmem, stream, P);                   \
        else if ((K) <= 8) VX_KL(kern<8>, grid_, block_, shmem, stream, P);              \
        else if ((K) <= 16) VX_KL(kern<16>, grid_, block_, shmem, stream, P);            \
        else VX_KL(kern<32>, grid_, block_, shmem, stream, P);                           \
    } while (0)

// One lane's list and the count of all keys offered behind the cursor.  kPos: the hits carry a leaf-order position; kInst: the keys have
// an instance part (otherwise it is 0 everywhere and not stored).
template <int KC, bool kPos, bool kInst>
struct HitList {
    static_assert(kPos || !kInst, "the instance field follows the position");
    enum : uint32_t { kFieldT = 0, kFieldPrim = 1, kFieldPos = 2, kFieldInst = 3, kWords = (2 + kPos + kInst) * KC * kMultiBlock };
    uint32_t* keys;  // [field][slot][lane], kWords of LDS
    uint32_t lane, K;
    uint32_t n = 0, total = 0;
    bool counting;
    float tmax;              // the acceptance bound
    float kth = INFINITY;    // the K-th kept t once the list is full
    float cur_t;             // the cursor; (-1, ...) = none
    uint32_t cur_i, cur_p;

    __device__ __forceinline__ uint32_t& at(uint32_t f, uint32_t s) const { return keys[(f * KC + s) * kMultiBlock + lane]; }
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
    // an accepted hit: primitive prim (at leaf-order position pos, of instance inst)
    __device__ __forceinline__ void offer(float t, uint32_t prim, uint32_t pos = 0u, uint32_t inst = 0u)
    {
        if (!(t > cur_t || (t == cur_t && (inst > cur_i || (inst == cur_i && prim > cur_p))))) return;  // not strictly after the cursor
        ++total;
        const uint32_t tb = __float_as_uint(t);
        if (n == K && !before(tb, inst, prim, K - 1u)) return;
        uint32_t j = n < K ? n : K - 1u;  // where the list's new tail goes: the K-th entry falls out of a full list
        while (j > 0u && before(tb, inst, prim, j - 1u)) {
            at(kFieldT, j) = at(kFieldT, j - 1u);
            at(kFieldPrim, j) = at(kFieldPrim, j - 1u);
            if (kPos) at(kFieldPos, j) = at(kFieldPos, j - 1u);
            if (kInst) at(kFieldInst, j) = at(kFieldInst, j - 1u);
            --j;
        }
        at(kFieldT, j) = tb;
        at(kFieldPrim, j) = prim;
        if (kPos) at(kFieldPos, j) = pos;
        if (kInst) at(kFieldInst, j) = inst;
        if (n < K) ++n;
        if (n == K) kth = __uint_as_float(at(kFieldT, K - 1u));
    }
    // ray r's t_out, prim_out (K entries, the empty slots padded) and count; the mesh kernels add their own outputs slot by slot
    __device__ __forceinline__ void write(const MultiOut& o, uint64_t r) const
    {
        for (uint32_t j = 0; j < K; ++j) {
            if (o.io.t_out) o.io.t_out[r * K + j] = j < n ? __uint_as_float(at(kFieldT, j)) : -1.0f;
            if (o.io.prim_out) o.io.prim_out[r * K + j] = j < n ? at(kFieldPrim, j) : 0xFFFFFFFFu;
        }
        if (o.count) o.count[r] = total;
    }
};

// an empty list for ray r of the query: its tmax, its cursor
template <int KC, bool kPos, bool kInst>
__device__ __forceinline__ void list_begin(HitList<KC, kPos, kInst>& L, uint32_t* keys, uint32_t lane, const MultiOut& o, uint64_t r)
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
}  // namespace vx
