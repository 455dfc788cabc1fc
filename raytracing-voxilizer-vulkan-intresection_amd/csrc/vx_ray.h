// vx_ray.h -- pieces every ray kernel shares: the ray of a batch (buffer or camera model), the closest-hit stage's cube-face normal and
// the wavefront compaction of the hit list (k_walk / k_rank, k_octree_trace, k_bvh_trace, k_tlas_trace); and, for the last three, the
// ray-batch block of their kernel arguments and the slab form of a ray.  Their epilogues (t / prim / shadowed / own outputs / hit list)
// stay in the kernels: a shared one changed the order of k_tlas_trace's stores and with it its register allocation.
#pragma once
#include "vx_internal.h"

#pragma clang fp contract(off)

namespace vx {

// The ray batch of k_octree_trace / k_bvh_trace / k_tlas_trace as a block of their kernel arguments: TraceIO's fields, the camera in
// device memory.
struct RayArgs {
    const float* rays;
    const Camera* cam;
    uint64_t nrays;
    float tmin, tmax;
    const float* tmax_per_ray;
    int any_hit;
    float* t_out;
    uint32_t* prim_out;
    float* normal_out;
    uint8_t* shadowed_out;
    vx_hit* hits;
    unsigned long long* nhits;
};

// fills the block from io and queues the clear of the hit counter on `s`
inline void set_ray_args(RayArgs& a, const TraceIO& io, hipStream_t s)
{
    a.rays = io.rays;
    a.cam = io.cam_dev;
    a.nrays = io.nrays;
    a.tmin = io.tmin;
    a.tmax = io.tmax;
    a.tmax_per_ray = io.tmax_per_ray;
    a.any_hit = io.any_hit ? 1 : 0;
    a.t_out = io.t_out;
    a.prim_out = io.prim_out;
    a.normal_out = io.normal_out;
    a.shadowed_out = io.shadowed_out;
    a.hits = io.hits;
    a.nhits = io.nhits;
    if (io.hits && io.nhits) (void)hipMemsetAsync(io.nhits, 0, sizeof(unsigned long long), s);
}

// A ray as the slab tests read it: origin, 1/d (raytrace.rint:48), and the axes on which 1/d is infinite (d = +-0 or denormal)
struct SlabRay {
    float o[3], inv[3];
    bool deg[3];
};

__device__ __forceinline__ void make_slab_ray(float ox, float oy, float oz, float dx, float dy, float dz, SlabRay& R)
{
    R.o[0] = ox; R.o[1] = oy; R.o[2] = oz;
    R.inv[0] = 1.0f / dx; R.inv[1] = 1.0f / dy; R.inv[2] = 1.0f / dz;
#pragma unroll
    for (int a = 0; a < 3; ++a) R.deg[a] = isinf(R.inv[a]);
}

// Ray r of the batch: from the ray buffer, or generated from the reference camera model (raytrace.rgen:41-47; mat*vec in glm's
// association (m0*v0 + m1*v1) + (m2*v2 + m3*v3)).
__device__ __forceinline__ void load_ray(bool primary, uint64_t r, const float* __restrict__ rays, const Camera* __restrict__ camp, float& ox, float& oy,
                                         float& oz, float& dx, float& dy, float& dz)
{
    if (primary) {
        const Camera& cam = *camp;  // in device memory: 34 dwords of kernel arguments would otherwise sit in (spilled) SGPRs
        const uint32_t px = (uint32_t)(r % cam.width), py = (uint32_t)(r / cam.width);
        const float u = ((float)px + 0.5f) / (float)cam.width, v = ((float)py + 0.5f) / (float)cam.height;
        const float ndx = u * 2.0f - 1.0f, ndy = v * 2.0f - 1.0f;
        float tg[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            tg[k] = (cam.projInv[0 + k] * ndx + cam.projInv[4 + k] * ndy) + (cam.projInv[8 + k] * 1.0f + cam.projInv[12 + k] * 1.0f);
        const float il = 1.0f / sqrtf((tg[0] * tg[0] + tg[1] * tg[1]) + tg[2] * tg[2]);
        const float n0 = tg[0] * il, n1 = tg[1] * il, n2 = tg[2] * il;
        ox = cam.viewInv[12]; oy = cam.viewInv[13]; oz = cam.viewInv[14];
        dx = (cam.viewInv[0] * n0 + cam.viewInv[4] * n1) + cam.viewInv[8] * n2;
        dy = (cam.viewInv[1] * n0 + cam.viewInv[5] * n1) + cam.viewInv[9] * n2;
        dz = (cam.viewInv[2] * n0 + cam.viewInv[6] * n1) + cam.viewInv[10] * n2;
    } else {
        const float2* rp = reinterpret_cast<const float2*>(rays + 6 * r);
        const float2 a = rp[0], b = rp[1], c = rp[2];
        ox = a.x; oy = a.y; oz = b.x; dx = b.y; dy = c.x; dz = c.y;
    }
}

// The non-finite rule of voxhip.h: a ray with NaN or +-Inf in any of its six components is a miss on every query.  Every ray kernel
// asks this once per ray in its set-up, right after load_ray, and retires the ray before an integer, an index or an interval is derived
// from its components.  x * 0 is NaN exactly for NaN (any sign, any payload) and +-Inf, and NaN survives the sum; no finite x can
// overflow it.  Without fast-math the products may not be folded to 0 (checked in the generated code: six v_mul, one v_cmp_u).
__device__ __forceinline__ bool ray_nonfinite(float ox, float oy, float oz, float dx, float dy, float dz)
{
    const float s = ((ox * 0.0f + oy * 0.0f) + oz * 0.0f) + ((dx * 0.0f + dy * 0.0f) + dz * 0.0f);
    return s != s;
}

// The cube-face normal of raytrace2.rchit:60-73 for a hit at t on box bb.
__device__ __forceinline__ void cube_normal(const float bb[6], float ox, float oy, float oz, float dx, float dy, float dz, float tt, float& n0, float& n1,
                                            float& n2)
{
    // worldPos = origin + direction * t; worldNrm = normalize(worldPos - (min + max) * 0.5)      rchit:60-65
    const float vx_ = (ox + dx * tt) - ((bb[0] + bb[3]) * 0.5f);
    const float vy_ = (oy + dy * tt) - ((bb[1] + bb[4]) * 0.5f);
    const float vz_ = (oz + dz * tt) - ((bb[2] + bb[5]) * 0.5f);
    const float il = 1.0f / sqrtf((vx_ * vx_ + vy_ * vy_) + vz_ * vz_);
    const float nx = vx_ * il, ny = vy_ * il, nz = vz_ * il;
    const float ax = fabsf(nx), ay = fabsf(ny), az = fabsf(nz);
    const float maxC = fmaxf(fmaxf(ax, ay), az);                                                // rchit:70
    if (maxC == ax) n0 = nx > 0.0f ? 1.0f : (nx < 0.0f ? -1.0f : 0.0f);                         // rchit:71-73
    else if (maxC == ay) n1 = ny > 0.0f ? 1.0f : (ny < 0.0f ? -1.0f : 0.0f);
    else n2 = nz > 0.0f ? 1.0f : (nz < 0.0f ? -1.0f : 0.0f);
}

// Primitive id of occupied voxel i (== gl_PrimitiveID: its rank in the ascending AABB list) = the set bits of the mask below it.
// prefix16 given (every 16th entry of the word prefix, dense: it stays in L2): the rank from the voxel's own 64-byte line of the mask -- one
// random line per ray instead of two (word_prefix[wi] is a line of its own; 19.7 -> 16.3 us per 1M rays); the line must lie inside the
// mask (nwords % 16 == 0).  Otherwise word_prefix[wi] + the bits below in the voxel's word.  (k_rank, k_walk's epilogue, k_multihit.)
__device__ __forceinline__ uint32_t voxel_rank(unsigned long long i, const uint32_t* __restrict__ words, const uint32_t* __restrict__ word_prefix,
                                               const uint32_t* __restrict__ prefix16)
{
    const uint64_t wi = i >> 5;
    const uint32_t bit = (uint32_t)i & 31u;
    if (prefix16) {
        const uint64_t g0 = wi & ~15ull;
        const uint32_t k = (uint32_t)wi & 15u;
        const uint4* lp = reinterpret_cast<const uint4*>(words + g0);
        const uint4 a = lp[0], b = lp[1], c = lp[2], d = lp[3];
        const uint32_t w16[16] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
        uint32_t cnt = prefix16[wi >> 4];
#pragma unroll
        for (uint32_t j = 0; j < 16u; ++j) cnt += __popc(j < k ? w16[j] : (j == k ? (w16[j] & ((1u << bit) - 1u)) : 0u));
        return cnt;
    }
    return word_prefix[wi] + __popc(words[wi] & ((1u << bit) - 1u));
}

// Hit compaction: ONE touch of the global counter per workgroup (of at most 16 waves; every thread of the workgroup calls this).
// One per wave meant 15 600 returning atomics on one address for 1M rays, ~10 ns each at the memory-side atomic unit: 196 us
// instead of 23 with 1024-thread workgroups.
__device__ __forceinline__ void compact_hit(bool hit, uint64_t r, uint32_t prim, float tt, vx_hit* __restrict__ hits, unsigned long long* nhits)
{
    __shared__ unsigned wcnt[16];
    __shared__ unsigned long long bbase;
    const unsigned long long bal = __ballot(hit);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = (int)(blockDim.x >> 6);
    if (lane == 0) wcnt[wv] = (unsigned)__popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned tot = 0;
        for (int w = 0; w < nw; ++w) tot += wcnt[w];
        bbase = tot ? atomicAdd(nhits, (unsigned long long)tot) : 0ull;
    }
    __syncthreads();
    if (hit) {
        unsigned long long off = bbase;
        for (int w = 0; w < wv; ++w) off += wcnt[w];
        vx_hit h;
        h.ray = (uint32_t)r; h.prim = prim; h.t = tt;
        hits[off + __popcll(bal & ((1ull << lane) - 1ull))] = h;
    }
}

}  // namespace vx
