// vx_trace.hip -- the ray stage around the walk kernel (vx_walk.hip): the occupancy mips of the traversal structure, the per-ray
// post-pass (primitive id, cube-face normal, hit compaction) and the launch sequence.  Replaces what the reference gets from the
// driver around its procedural-hit shader: the acceleration-structure build (hello_vulkan.cpp:737-760), gl_PrimitiveID, and the
// closest-hit stage's normal (raytrace2.rchit:60-73).
#include "vx_internal.h"
#include "vx_ray.h"

#include <cstddef>
#include <cstdlib>
#include <cstring>

#pragma clang fp contract(off)

namespace vx {

// Level-1 mip: one bit per brick, x-fastest, from the z-oriented brick words.
__global__ __launch_bounds__(256) void k_brick_mip1(const unsigned long long* __restrict__ bricks, uint64_t nbricks, uint32_t* __restrict__ m1)
{
    // one pass over whole 64-brick groups: the mip -- 64 bits per wave -- is written as two plain words per wave
    const uint64_t ngroups = (nbricks + 63) / 64;
    for (uint64_t gidx = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 6; gidx < ngroups; gidx += ((uint64_t)gridDim.x * 256u) >> 6) {
        const uint64_t b = gidx * 64 + (threadIdx.x & 63);
        unsigned long long any = 0;
        if (b < nbricks) {
            const ulonglong2* p = reinterpret_cast<const ulonglong2*>(bricks + b * 8ull);
            const ulonglong2 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];
            any = q0.x | q0.y | q1.x | q1.y | q2.x | q2.y | q3.x | q3.y;
        }
        const unsigned long long occ = __ballot(any != 0);
        if ((threadIdx.x & 63) == 0) {
            m1[gidx * 2] = (uint32_t)occ;
            m1[gidx * 2 + 1] = (uint32_t)(occ >> 32);
        }
    }
}

void launch_brick_mip1(const unsigned long long* bricks, uint64_t nbricks, uint32_t* m1, hipStream_t s)
{
    if (!nbricks) return;
    uint64_t nblk = (nbricks + 255) / 256;
    if (nblk > 4096) nblk = 4096;
    VX_KL(k_brick_mip1, dim3((unsigned)nblk), dim3(256), 0, s, bricks, nbricks, m1);
}

// (the level-2 mip is built in vx_kernels.hip: its kernel shares a launch with the line-count scan)

// Per-ray post-pass over all rays: primitive id (== gl_PrimitiveID: rank of the voxel in the ascending AABB list), the
// cube-face normal of raytrace2.rchit:60-73, and wavefront hit compaction.
__global__ __launch_bounds__(1024) void k_rank(const float* __restrict__ t, const void* __restrict__ idx_any, int idx32, uint64_t nrays, GridParams g,
                                              const uint32_t* __restrict__ words, const uint32_t* __restrict__ word_prefix, const float* __restrict__ rays,
                                              const Camera* __restrict__ cam, uint32_t* __restrict__ prim_out, float* __restrict__ normal_out, vx_hit* __restrict__ hits,
                                              unsigned long long* nhits, const uint32_t* __restrict__ prefix16 /*optional: word_prefix[16 i], dense*/)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = r < nrays;
    float tt = -1.0f;
    uint32_t prim = 0xFFFFFFFFu;
    if (active) {
        tt = t[r];
        unsigned long long i;  // k_walk writes 32-bit voxel indices when the grid has fewer than 2^32 - 1 voxels, 64-bit ones otherwise
        if (idx32) { const uint32_t i32 = reinterpret_cast<const uint32_t*>(idx_any)[r]; i = i32 == 0xFFFFFFFFu ? ~0ull : (unsigned long long)i32; }
        else i = reinterpret_cast<const unsigned long long*>(idx_any)[r];
        float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
        if (i != ~0ull) {
            prim = voxel_rank(i, words, word_prefix, prefix16);
            if (normal_out) {
                const uint64_t XY = (uint64_t)g.dim[0] * g.dim[1];
                const uint32_t z = (uint32_t)(i / XY);
                const uint64_t rem = i - (uint64_t)z * XY;  // (X * Y may exceed 32 bits on a long thin grid)
                const uint32_t y = (rem >> 32) ? (uint32_t)(rem / g.dim[0]) : (uint32_t)rem / g.dim[0];
                const uint32_t x = (uint32_t)(rem - (uint64_t)y * g.dim[0]);
                float bb[6], ox, oy, oz, dx, dy, dz;
                cell_aabb(g, x, y, z, bb);
                load_ray(rays == nullptr, r, rays, cam, ox, oy, oz, dx, dy, dz);
                cube_normal(bb, ox, oy, oz, dx, dy, dz, tt, n0, n1, n2);
            }
        }
        if (prim_out) prim_out[r] = prim;
        if (normal_out) { normal_out[3 * r] = n0; normal_out[3 * r + 1] = n1; normal_out[3 * r + 2] = n2; }
    }
    if (hits) compact_hit(active && prim != 0xFFFFFFFFu, r, prim, tt, hits, nhits);  // launched with 1024 threads: one counter touch per 16 waves
}

bool launch_walk(const GridParams& g, const TraceMips& mips, const TraceIO& io, unsigned long long* counters, int* phase, void* idx_out, bool idx32, hipStream_t s, WalkQueue* queue,
                 const WalkRank* rank);

// A gate in front of work that is to run BESIDE a ray batch on another stream (the Vec list's emission, VX_VOXELIZE_LIST_ASYNC): one wave
// that leaves once the ray kernel's work counter has reached `at_least` -- 1: the first wave has come back for more rays, the kernel's
// persistent workgroups are on the machine -- or after the time bound (300 us), whichever comes first.  The bound makes it safe under tools
// that serialise the kernels of all streams (counter-collecting profilers): a stream-level wait on the counter (hipStreamWaitValue64,
// which polls without a wave) hung three of five rocprofv3 --pmc passes there, because the waiting packet went first and the ray kernel
// was never let through.  The counter is only ever changed by memory-side atomics: read it the same way.
__global__ __launch_bounds__(64) void k_queue_gate(unsigned long long* counter, unsigned long long at_least, unsigned long long timeout_ticks /*100 MHz*/)
{
    if (threadIdx.x != 0) return;
    const unsigned long long t0 = (unsigned long long)wall_clock64();
    for (;;) {
        if (atomicAdd(counter, 0ull) >= at_least) break;
        if ((unsigned long long)wall_clock64() - t0 > timeout_ticks) break;
        __builtin_amdgcn_s_sleep(32);  // ~0.9 us at 2.4 GHz
    }
}
void launch_queue_gate(const WalkQueue& q, hipStream_t s)
{
    if (!q.counter) return;
    VX_KL(k_queue_gate, dim3(1), dim3(64), 0, s, q.counter, /*at_least=*/1ull, /*timeout_ticks=*/300ull * 100ull);
}

bool launch_trace(const GridParams& g, const TraceMips& mips, const uint32_t* word_prefix, const TraceIO& io, unsigned long long* counters /*2*/,
                  int* phase, void* idx_tmp, hipStream_t s, const uint32_t* prefix16, WalkQueue* queue, const WalkRing* ring)
{
    const uint64_t nrays = io.nrays;
    if (!nrays) return true;
    // (the rank pass reads prefix16 where it is given and word_prefix otherwise: a build that left only prefix16 passes no word_prefix)
    const bool can_rank = (io.prim_out || io.hits || io.normal_out) && (word_prefix || prefix16) && idx_tmp;
    // prim and nothing else that k_rank makes (no hit list, no normals): the waves of k_walk rank the rays they retired as they leave,
    // where the batch allows it (launch_walk); k_rank, which also reads t, stays for everything else
    const bool idx32 = trace_idx32(g);
    const bool in_walk = can_rank && ring && ring->cap && io.prim_out && !io.hits && !io.normal_out && idx32;
    const bool want_rank = can_rank && (io.t_out || in_walk);
    WalkRank wr;
    if (in_walk) { wr.words = mips.w0; wr.word_prefix = word_prefix; wr.prefix16 = prefix16; wr.prim_out = io.prim_out; wr.ring = *ring; }
    const bool ranked = launch_walk(g, mips, io, counters, phase, want_rank ? idx_tmp : nullptr, idx32, s, queue, in_walk ? &wr : nullptr);
    if (want_rank && !ranked && !io.t_out) return false;  // (the caller gave a ring and kept no t: see vx_internal.h)
    if (want_rank && !ranked) {
        if (io.hits && io.nhits) (void)hipMemsetAsync(io.nhits, 0, sizeof(unsigned long long), s);
        const unsigned rthreads = io.hits ? 1024u : 256u;  // the hit list's compaction touches the global counter once per workgroup
        const dim3 rgrid((unsigned)((nrays + rthreads - 1) / rthreads)), rblock(rthreads);
        VX_KL(k_rank, rgrid, rblock, 0, s, io.t_out, (const void*)idx_tmp, idx32 ? 1 : 0, nrays, g, mips.w0, word_prefix, io.rays, io.cam_dev, io.prim_out, io.normal_out,
              io.hits, io.nhits, prefix16);
    }
    return true;
}

}  // namespace vx
