// vx_poses.hip -- pose queries on a vx_field: per pose the smallest clearance over a body's points, the point that has it and the number of
// points within the margin (k_field_poses, k_field_poses_narrow), then the outputs from the reduced keys (k_field_poses_finish).  The
// arithmetic is vx_poses.h's, which a host driver compiles too.
//
// A lane keeps one point and its radius in registers and walks poses; the lanes of a wave sample neighbouring positions of one posed
// body, so the eight-corner gathers of a wave fall into few lines (the coherent regime of DESIGN 6w).  Two shapes, chosen by P:
//   P > 64   k_field_poses: a workgroup is a chunk of 256 points and walks a tile of kPoseTile poses.  The transform is wave-uniform
//            (scalar loads).  Per pose a wave reduces its 64 orderable values with shuffles and takes the winner and the count from two
//            ballots; the waves leave their partials in LDS, and after the tile one lane per pose combines the four and, where the body
//            spans several chunks, merges into the per-pose scratch with a 64-bit atomicMin and an atomicAdd.
//   P <= 64  k_field_poses_narrow<W>: a group of W = 2^k >= P lanes is one pose, a wave holds 64 / W poses at once; the same shuffles
//            over W lanes and the same ballots masked to the group.  The group's first lane stores the pose's key and count: no LDS, no
//            atomics.
// Integer min and add do not depend on order, so the scratch -- and with it every output -- is the same whatever the launch shape.
// No workgroup waits for another: the finish kernel follows in stream order.
#include "vx_internal.h"
#include "vx_poses.h"

#pragma clang fp contract(off)

namespace vx {

constexpr uint32_t kOrdNone = 0xFFFFFFFFu;  // a lane without a value: no orderable(g) equals it (vx_poses.h)
constexpr uint32_t kPoseMaxGrid = 1u << 20; // blocks of 256: the grid stays below 2^32 threads; the kernels stride over the rest

// the lane's orderable clearance under transform m (kOrdNone: no point here, or skipped) and whether it lies within the margin
__device__ __forceinline__ uint32_t pose_lane(const float* __restrict__ S, const FieldGeom& G, const float* __restrict__ m, bool live, const float p[3],
                                              float radius, float margin, bool* within)
{
    uint32_t ord = kOrdNone;
    *within = false;
    if (live) {
        const float g = pose_gap(S, G, m, p, radius);
        if (g == g) {
            ord = pose_orderable(g);
            *within = pose_within(g, margin);
        }
    }
    return ord;
}

template <uint32_t W> __device__ __forceinline__ uint32_t pose_group_min(uint32_t v)
{
#pragma unroll
    for (uint32_t s = W / 2; s >= 1; s >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, (int)s, 64);
        v = o < v ? o : v;
    }
    return v;
}

template <bool ATOMIC>
__global__ __launch_bounds__(256) void k_field_poses(const float* __restrict__ S, FieldGeom G, FieldPoseIO io, uint32_t chunks, uint64_t items)
{
    __shared__ unsigned long long skey[kPoseTile][4];
    __shared__ uint32_t scnt[kPoseTile][4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t chunk = (uint32_t)(item % chunks);
        const uint64_t n0 = (item / chunks) * kPoseTile;
        const uint32_t nt = io.nposes - n0 < kPoseTile ? (uint32_t)(io.nposes - n0) : kPoseTile;
        const uint64_t i = (uint64_t)chunk * kPoseChunk + threadIdx.x;
        const bool live = i < io.npoints;
        float p[3] = {0.0f, 0.0f, 0.0f}, radius = 0.0f;
        if (live) {
            p[0] = io.points[3 * i]; p[1] = io.points[3 * i + 1]; p[2] = io.points[3 * i + 2];
            if (io.radii) radius = io.radii[i];
        }
        for (uint32_t t = 0; t < nt; ++t) {
            const float* m = io.transforms + 12 * (n0 + t);
            bool within;
            const uint32_t ord = pose_lane(S, G, m, live, p, radius, io.margin, &within);
            const uint32_t mn = pose_group_min<64>(ord);
            const unsigned long long eq = __ballot(ord == mn && ord != kOrdNone);  // (lanes hold ascending indices: the lowest lane wins)
            const unsigned long long in = __ballot(within);
            if (lane == 0) {
                const uint32_t first = chunk * kPoseChunk + wave * 64u + (uint32_t)__builtin_ctzll(eq | (1ull << 63));
                skey[t][wave] = eq ? (((unsigned long long)mn << 32) | first) : kPoseNone;
                scnt[t][wave] = (uint32_t)__popcll(in);
            }
        }
        __syncthreads();
        if (threadIdx.x < nt) {
            unsigned long long k = skey[threadIdx.x][0];
            uint32_t c = scnt[threadIdx.x][0];
            for (int w = 1; w < 4; ++w) {
                const unsigned long long o = skey[threadIdx.x][w];
                k = o < k ? o : k;
                c += scnt[threadIdx.x][w];
            }
            const uint64_t n = n0 + threadIdx.x;
            if (ATOMIC) {  // (the scratch was set to "none" and 0 in front of this launch)
                if (k != kPoseNone) atomicMin(&io.keys[n], k);
                if (c) atomicAdd(&io.counts[n], c);
            } else {
                io.keys[n] = k;
                io.counts[n] = c;
            }
        }
        __syncthreads();
    }
}

template <uint32_t W>
__global__ __launch_bounds__(256) void k_field_poses_narrow(const float* __restrict__ S, FieldGeom G, FieldPoseIO io, uint64_t items)
{
    constexpr uint32_t kGroups = 256u / W;
    const uint32_t grp = threadIdx.x / W, l = threadIdx.x % W;
    const uint32_t base = (threadIdx.x & 63u) & ~(W - 1u);  // the group's first lane in its wave
    const unsigned long long gmask = (W == 64u ? ~0ull : ((1ull << (W & 63u)) - 1ull)) << base;
    const bool live = l < io.npoints;
    float p[3] = {0.0f, 0.0f, 0.0f}, radius = 0.0f;
    if (live) {
        p[0] = io.points[3 * l]; p[1] = io.points[3 * l + 1]; p[2] = io.points[3 * l + 2];
        if (io.radii) radius = io.radii[l];
    }
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        for (uint32_t k = 0; k < kPoseNarrowRounds; ++k) {
            const uint64_t n0 = (item * kPoseNarrowRounds + k) * kGroups;
            if (n0 >= io.nposes) break;
            const uint64_t n = n0 + grp;
            const bool has = n < io.nposes;
            bool within;
            const uint32_t ord = pose_lane(S, G, io.transforms + 12 * (has ? n : n0), live && has, p, radius, io.margin, &within);
            const uint32_t mn = pose_group_min<W>(ord);
            const unsigned long long eq = __ballot(ord == mn && ord != kOrdNone) & gmask;
            const unsigned long long in = __ballot(within) & gmask;
            if (has && l == 0) {
                const uint32_t first = (uint32_t)__builtin_ctzll(eq | (1ull << 63)) - base;
                io.keys[n] = eq ? (((unsigned long long)mn << 32) | first) : kPoseNone;
                io.counts[n] = (uint32_t)__popcll(in);
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_field_poses_finish(const float* __restrict__ S, FieldGeom G, FieldPoseIO io)
{
    for (uint64_t n = (uint64_t)blockIdx.x * 256u + threadIdx.x; n < io.nposes; n += (uint64_t)gridDim.x * 256u) {
        float clr, pos[3], grad[3];
        uint32_t point;
        pose_finish(S, G, io.transforms + 12 * n, io.points, io.keys[n], io.position != nullptr, io.gradient != nullptr, &clr, &point, pos, grad);
        if (io.clearance) io.clearance[n] = clr;
        if (io.point) io.point[n] = point;
        if (io.count) io.count[n] = io.counts[n];
        if (io.position) { io.position[3 * n] = pos[0]; io.position[3 * n + 1] = pos[1]; io.position[3 * n + 2] = pos[2]; }
        if (io.gradient) { io.gradient[3 * n] = grad[0]; io.gradient[3 * n + 1] = grad[1]; io.gradient[3 * n + 2] = grad[2]; }
    }
}

template <uint32_t W> static void launch_narrow(const float* S, const FieldGeom& G, const FieldPoseIO& io, hipStream_t s)
{
    const uint64_t per = (uint64_t)kPoseNarrowRounds * (256u / W), items = (io.nposes + per - 1) / per;
    VX_KL(k_field_poses_narrow<W>, dim3((unsigned)(items < kPoseMaxGrid ? items : kPoseMaxGrid)), dim3(256), 0, s, S, G, io, items);
}

hipError_t launch_field_poses(const float* S, const FieldGeom& G, const FieldPoseIO& io, hipStream_t s)
{
    if (!io.nposes) return hipSuccess;
    const uint32_t P = io.npoints;
    if (P > 64u) {
        const uint32_t chunks = (uint32_t)(((uint64_t)P + kPoseChunk - 1) / kPoseChunk);
        const uint64_t items = (uint64_t)chunks * ((io.nposes + kPoseTile - 1) / kPoseTile);
        const dim3 grid((unsigned)(items < kPoseMaxGrid ? items : kPoseMaxGrid));
        if (chunks > 1) {
            hipError_t e = hipMemsetAsync(io.keys, 0xFF, io.nposes * 8, s);
            if (e == hipSuccess) e = hipMemsetAsync(io.counts, 0, io.nposes * 4, s);
            if (e != hipSuccess) return e;
            VX_KL(k_field_poses<true>, grid, dim3(256), 0, s, S, G, io, chunks, items);
        } else {
            VX_KL(k_field_poses<false>, grid, dim3(256), 0, s, S, G, io, chunks, items);
        }
    }
    else if (P > 32u) launch_narrow<64>(S, G, io, s);
    else if (P > 16u) launch_narrow<32>(S, G, io, s);
    else if (P > 8u) launch_narrow<16>(S, G, io, s);
    else if (P > 4u) launch_narrow<8>(S, G, io, s);
    else if (P > 2u) launch_narrow<4>(S, G, io, s);
    else if (P > 1u) launch_narrow<2>(S, G, io, s);
    else launch_narrow<1>(S, G, io, s);
    const uint64_t blocks = (io.nposes + 255) / 256;
    VX_KL(k_field_poses_finish, dim3((unsigned)(blocks < kPoseMaxGrid ? blocks : kPoseMaxGrid)), dim3(256), 0, s, S, G, io);
    return hipGetLastError();
}

}  // namespace vx
