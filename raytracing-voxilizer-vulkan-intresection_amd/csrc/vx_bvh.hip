// vx_bvh.hip -- ray queries on the triangle mesh itself: the reference's triangle BLAS (hello_vulkan.cpp:596-635, objectToVkGeometryKHR over
// the model loadModel read) under raytrace.rchit, as a binary LBVH built on the device and a one-ray-per-lane traversal.
//
// Result contract (include/voxhip.h): per (ray, triangle) Moeller-Trumbore in float32 in the pinned order, accepted iff u >= 0, u <= 1,
// v >= 0, u + v <= 1, t > 0, tmin <= t <= tmax; t = the minimum accepted t over ALL triangles, prim = the smallest triangle index reaching
// it, bary = (u, v) of that triangle -- exactly the brute force over the mesh (tests/mesh_ref.py).
//
// Build (Karras 2012, "Maximizing parallelism in the construction of BVHs, octrees and k-d trees"):
//   k_bvh_prep    triangle bounds, their union (ordered-int atomics, one per block and component) and the index check of borrowed meshes;
//   k_bvh_keys    30-bit Morton code of the bounds centre over that union, key = code << 32 | triangle: unique, so the order is total;
//   launch_sort_u64 over 62 bits;
//   k_bvh_karras  the radix tree over the sorted keys: internal node i splits the range it covers at the highest differing key bit;
//   k_bvh_bounds  one lane per leaf writes the de-indexed triangle at its sorted position and climbs: the FIRST lane to reach a node
//                 stops, the second (both children's boxes are then written) merges them and goes on.  Nothing waits on another lane.
//                 Boxes are the exact float min / max of the vertices below; the height of every node comes along;
//   k_bvh_alive + scan + k_bvh_emit  collapse: a subtree of at most max_leaf triangles becomes ONE leaf (its triangles are contiguous in
//                 sorted order), the surviving nodes are renumbered densely with the root at 0.
// The tree depth is bounded by construction: a child's common key prefix is strictly longer than its parent's and keys have 62 bits, so
// no path holds more than 62 interior nodes.  The traversal stack needs at most one entry per interior node on the current path; the
// build reports the actual height (<= 62) and the trace kernel sizes its LDS stack to it.
//
// Traversal: front to back (the nearer child first, the farther one on the stack), a popped node re-tested against the best t found
// since.  A node is entered on its box WIDENED by kBoxExt of the mesh's extent plus kBoxPos of its largest |coordinate|, and its
// slab interval widened by kTRel relative to t: a triangle's Moeller-Trumbore t and the slab t of its own box are computed differently
// and may differ by a few ulps -- for a zero-thickness box (an axis-aligned floor) the slab interval is a single point -- and pruning on the bare box could drop the
// brute force's answer.  Ties: a node whose entry t EQUALS the best t is still entered (it may hold a lower index).  An axis with an
// infinite 1/d (d = +-0 or denormal) takes no part in the interval (0 * inf = NaN); the ray's coordinate on it is constant, so the node
// is entered only when that coordinate lies in the widened box, as in k_octree_trace.
// The widening covers Moeller-Trumbore's rounding only where that rounding is bounded: its error in the hit point grows like
// eps * |e1| |e2| / |e1 x e2|, without limit for slivers and (exactly or nearly) collinear triangles, whose t is rounding noise that
// may lie anywhere on the ray.  The build puts every triangle whose angle at v0 has a sine below kIllSin (2^-10) on a side list, and
// every ray tests that list before the descent, whatever the boxes say: the brute force's answer cannot be pruned away there either.
#include "vx_internal.h"
#include "vx_ray.h"
#include "vx_blas.h"

#include <cstring>

#pragma clang fp contract(off)

namespace vx {

namespace {

constexpr uint32_t kBuildBlock = 256;
constexpr uint32_t kBvhBlock = 128;       // lanes per trace workgroup; the stack is [level][lane] in LDS
constexpr double kIllSin = 1.0 / 1024.0;  // triangles thinner than this go on the side list every ray tests (see the head of the file)
constexpr float kBoxExt = 1.0f / 1024.0f; // box widening: relative to the mesh's extent (the size of its triangles' rounding terms)...
constexpr float kBoxPos = 1.0f / 262144.0f; // ... plus 2^-18 (~32 ulps) of its largest |coordinate| (the rounding of positions themselves)

// the triangle's three vertices; false (and zeros) when an index leaves [0, nv)
__device__ __forceinline__ bool load_tri(const float* __restrict__ v, const int32_t* __restrict__ idx, uint64_t nv, uint32_t t, float p[9])
{
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int32_t i = idx[3ull * t + k];
        const bool in = i >= 0 && (uint64_t)i < nv;
        ok &= in;
#pragma unroll
        for (int a = 0; a < 3; ++a) p[3 * k + a] = in ? v[3ull * (uint32_t)i + a] : 0.0f;
    }
    return ok;
}

}  // namespace

// Box of the bounds of all triangles (ordered uint encoding: 0..2 min, 3..5 max, initialised by the host to ~0 / 0), the index check
// (err bit 0) and the check for non-finite coordinates of referenced vertices (err bit 1).
__global__ __launch_bounds__(kBuildBlock) void k_bvh_prep(const float* __restrict__ v, const int32_t* __restrict__ idx, uint64_t nv, uint32_t ntri,
                                                          uint32_t* __restrict__ box6, uint32_t* __restrict__ err)
{
    __shared__ uint32_t sb[6];
    if (threadIdx.x < 6) sb[threadIdx.x] = threadIdx.x < 3 ? 0xFFFFFFFFu : 0u;
    __syncthreads();
    const uint32_t t = blockIdx.x * kBuildBlock + threadIdx.x;
    if (t < ntri) {
        float p[9];
        if (!load_tri(v, idx, nv, t, p)) atomicOr(err, 1u);
        bool fin = true;
#pragma unroll
        for (int k = 0; k < 9; ++k) fin &= isfinite(p[k]);
        if (!fin) atomicOr(err, 2u);  // a referenced vertex with a NaN or infinite coordinate: the build refuses the mesh
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            atomicMin(&sb[a], f2ord(fminf(fminf(p[a], p[3 + a]), p[6 + a])));
            atomicMax(&sb[3 + a], f2ord(fmaxf(fmaxf(p[a], p[3 + a]), p[6 + a])));
        }
    }
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(&box6[threadIdx.x], sb[threadIdx.x]);
    else if (threadIdx.x < 6) atomicMax(&box6[threadIdx.x], sb[threadIdx.x]);
}

__global__ __launch_bounds__(kBuildBlock) void k_bvh_keys(const float* __restrict__ v, const int32_t* __restrict__ idx, uint64_t nv, uint32_t ntri,
                                                          const uint32_t* __restrict__ box6, uint64_t* __restrict__ keys)
{
    const uint32_t t = blockIdx.x * kBuildBlock + threadIdx.x;
    if (t >= ntri) return;
    float p[9];
    (void)load_tri(v, idx, nv, t, p);
    uint32_t q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float lo = ord2f(box6[a]), hi = ord2f(box6[3 + a]);
        const float c = (fminf(fminf(p[a], p[3 + a]), p[6 + a]) + fmaxf(fmaxf(p[a], p[3 + a]), p[6 + a])) * 0.5f;
        const float ext = hi - lo;
        const float f = ext > 0.0f ? (c - lo) / ext * 1024.0f : 0.0f;
        q[a] = f >= 1023.0f ? 1023u : (f > 0.0f ? (uint32_t)f : 0u);  // (NaN -> 0)
    }
    const uint64_t code = (uint64_t)(spread10(q[0]) | (spread10(q[1]) << 1) | (spread10(q[2]) << 2));
    keys[t] = (code << 32) | t;
}

// Unified node numbering of the radix tree: internal i -> i (0 .. n-2, root 0), leaf j -> n-1+j.
__device__ __forceinline__ int kdelta(const uint64_t* __restrict__ k, int64_t n, int64_t i, int64_t j)
{
    if (j < 0 || j >= n) return -1;
    return __clzll(k[i] ^ k[j]);  // keys are unique: never 64
}

__global__ __launch_bounds__(kBuildBlock) void k_bvh_karras(const uint64_t* __restrict__ k, uint32_t n, uint32_t* __restrict__ child,
                                                            uint32_t* __restrict__ parent, uint32_t* __restrict__ range)
{
    const int64_t i = (int64_t)blockIdx.x * kBuildBlock + threadIdx.x;
    if (i >= (int64_t)n - 1) return;
    const int64_t N = n;
    const int d = kdelta(k, N, i, i + 1) - kdelta(k, N, i, i - 1) >= 0 ? 1 : -1;
    const int dmin = kdelta(k, N, i, i - d);
    int64_t lmax = 2;
    while (kdelta(k, N, i, i + lmax * d) > dmin) lmax *= 2;
    int64_t l = 0;
    for (int64_t t = lmax / 2; t >= 1; t /= 2)
        if (kdelta(k, N, i, i + (l + t) * d) > dmin) l += t;
    const int64_t j = i + l * d;
    const int dnode = kdelta(k, N, i, j);
    int64_t s = 0;
    for (int64_t div = 2;; div *= 2) {
        const int64_t t = (l + div - 1) / div;
        if (kdelta(k, N, i, i + (s + t) * d) > dnode) s += t;
        if (t <= 1) break;
    }
    const int64_t gamma = i + s * d + (d < 0 ? -1 : 0);
    const int64_t lo = i < j ? i : j, hi = i < j ? j : i;
    const uint32_t left = lo == gamma ? (uint32_t)(N - 1 + gamma) : (uint32_t)gamma;
    const uint32_t right = hi == gamma + 1 ? (uint32_t)(N - 1 + gamma + 1) : (uint32_t)(gamma + 1);
    child[2 * i] = left;
    child[2 * i + 1] = right;
    parent[left] = (uint32_t)i;
    parent[right] = (uint32_t)i;
    range[2 * i] = (uint32_t)lo;
    range[2 * i + 1] = (uint32_t)hi;
}

// kbox: per unified node {min xyz, height, max xyz, pad} (32 B).  tris: the de-indexed triangles in sorted (= leaf) order, 3 float4 each:
// (v0, triangle index), (v1, 1 when the triangle is on the side list, else 0), (v2, 0).
__global__ __launch_bounds__(kBuildBlock) void k_bvh_bounds(const float* __restrict__ v, const int32_t* __restrict__ idx, uint64_t nv, uint32_t n,
                                                            const uint64_t* __restrict__ keys, const uint32_t* __restrict__ child,
                                                            const uint32_t* __restrict__ parent, uint32_t* __restrict__ arrived, float4* kbox,
                                                            float4* __restrict__ tris, uint32_t* __restrict__ ill, uint32_t* __restrict__ nill)
{
    const uint32_t j = blockIdx.x * kBuildBlock + threadIdx.x;
    if (j >= n) return;
    const uint32_t tri = (uint32_t)(keys[j] & 0xFFFFFFFFull);
    float p[9];
    (void)load_tri(v, idx, nv, tri, p);
    bool on_side_list = false;
    {   // ill-conditioned (sin of the angle at v0 below kIllSin, collinear included): its MT t is rounding noise -> the side list
        const double e1[3] = {(double)p[3] - p[0], (double)p[4] - p[1], (double)p[5] - p[2]};
        const double e2[3] = {(double)p[6] - p[0], (double)p[7] - p[1], (double)p[8] - p[2]};
        const double c0 = e1[1] * e2[2] - e1[2] * e2[1], c1 = e1[2] * e2[0] - e1[0] * e2[2], c2 = e1[0] * e2[1] - e1[1] * e2[0];
        const double l1 = e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2], l2 = e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2];
        on_side_list = l1 > 0.0 && l2 > 0.0 && c0 * c0 + c1 * c1 + c2 * c2 <= kIllSin * kIllSin * l1 * l2;
        if (on_side_list) ill[atomicAdd(nill, 1u)] = j;
    }
    // the w of v1 marks a side-listed triangle for the multi-hit kernels (vx_meshmulti.hip), which must count it once; the first-hit
    // kernels do not read it
    tris[3ull * j] = make_float4(p[0], p[1], p[2], __uint_as_float(tri));
    tris[3ull * j + 1] = make_float4(p[3], p[4], p[5], __uint_as_float(on_side_list ? 1u : 0u));
    tris[3ull * j + 2] = make_float4(p[6], p[7], p[8], 0.0f);
    const uint32_t leaf = n - 1 + j;
    kbox[2ull * leaf] = make_float4(fminf(fminf(p[0], p[3]), p[6]), fminf(fminf(p[1], p[4]), p[7]), fminf(fminf(p[2], p[5]), p[8]), __uint_as_float(0u));
    kbox[2ull * leaf + 1] = make_float4(fmaxf(fmaxf(p[0], p[3]), p[6]), fmaxf(fmaxf(p[1], p[4]), p[7]), fmaxf(fmaxf(p[2], p[5]), p[8]), 0.0f);
    uint32_t node = parent[leaf];
    while (node != blas::kNone) {
        __threadfence();                                   // release this lane's box
        if (atomicAdd(&arrived[node], 1u) == 0u) return;   // the sibling's box is not there yet: its lane carries on
        __threadfence();                                   // acquire the sibling's
        const uint32_t a = child[2 * node], b = child[2 * node + 1];
        const float4 a0 = kbox[2ull * a], a1 = kbox[2ull * a + 1];  // (kbox is not __restrict__: these loads stay behind the fence)
        const float4 b0 = kbox[2ull * b], b1 = kbox[2ull * b + 1];
        const uint32_t ha = __float_as_uint(a0.w), hb = __float_as_uint(b0.w);
        kbox[2ull * node] = make_float4(fminf(a0.x, b0.x), fminf(a0.y, b0.y), fminf(a0.z, b0.z), __uint_as_float(1u + (ha > hb ? ha : hb)));
        kbox[2ull * node + 1] = make_float4(fmaxf(a1.x, b1.x), fmaxf(a1.y, b1.y), fmaxf(a1.z, b1.z), 0.0f);
        node = parent[node];
    }
}

// a node survives the collapse iff it is the root or its parent holds more than max_leaf triangles
__global__ __launch_bounds__(kBuildBlock) void k_bvh_alive(uint32_t n, const uint32_t* __restrict__ parent, const uint32_t* __restrict__ range,
                                                           uint32_t max_leaf, uint32_t* __restrict__ alive)
{
    const uint32_t u = blockIdx.x * kBuildBlock + threadIdx.x;
    if (u >= 2 * n - 1) return;
    const uint32_t p = parent[u];
    alive[u] = (p == blas::kNone || range[2 * p + 1] - range[2 * p] + 1u > max_leaf) ? 1u : 0u;
}

// the collapsed node array: {min xyz, a, max xyz, b}; interior: a, b = the children's new indices; leaf: a = first triangle (leaf order),
// b = kLeafBit | count
__global__ __launch_bounds__(kBuildBlock) void k_bvh_emit(uint32_t n, const uint32_t* __restrict__ alive, const uint32_t* __restrict__ newidx,
                                                          const uint32_t* __restrict__ child, const uint32_t* __restrict__ range, uint32_t max_leaf,
                                                          const float4* __restrict__ kbox, float4* __restrict__ nodes)
{
    const uint32_t u = blockIdx.x * kBuildBlock + threadIdx.x;
    if (u >= 2 * n - 1 || !alive[u]) return;
    const bool is_leaf = u >= n - 1;
    const uint32_t first = is_leaf ? u - (n - 1) : range[2 * u];
    const uint32_t cnt = is_leaf ? 1u : range[2 * u + 1] - range[2 * u] + 1u;
    uint32_t a, b;
    if (is_leaf || cnt <= max_leaf) { a = first; b = blas::kLeafBit | cnt; }
    else { a = newidx[child[2 * u]]; b = newidx[child[2 * u + 1]]; }
    const float4 m0 = kbox[2ull * u], m1 = kbox[2ull * u + 1];
    const uint32_t o = newidx[u];
    nodes[2ull * o] = make_float4(m0.x, m0.y, m0.z, __uint_as_float(a));
    nodes[2ull * o + 1] = make_float4(m1.x, m1.y, m1.z, __uint_as_float(b));
}

void launch_bvh_prep(const float* v, const int32_t* idx, uint64_t nv, uint32_t ntri, uint32_t* box6, uint32_t* err, uint64_t* keys, hipStream_t s)
{
    const dim3 g((ntri + kBuildBlock - 1) / kBuildBlock);
    VX_KL(k_bvh_prep, g, dim3(kBuildBlock), 0, s, v, idx, nv, ntri, box6, err);
    VX_KL(k_bvh_keys, g, dim3(kBuildBlock), 0, s, v, idx, nv, ntri, box6, keys);
}

void launch_bvh_tree(const float* v, const int32_t* idx, uint64_t nv, uint32_t n, const uint64_t* keys, uint32_t max_leaf, uint32_t* child,
                     uint32_t* parent, uint32_t* range, uint32_t* arrived, float* kbox, float* tris, uint32_t* alive, uint32_t* ill, uint32_t* nill,
                     hipStream_t s)
{
    (void)hipMemsetAsync(parent, 0xFF, (size_t)(2ull * n - 1) * 4, s);
    (void)hipMemsetAsync(arrived, 0, (size_t)n * 4, s);
    if (n > 1) VX_KL(k_bvh_karras, dim3((n - 1 + kBuildBlock - 1) / kBuildBlock), dim3(kBuildBlock), 0, s, keys, n, child, parent, range);
    VX_KL(k_bvh_bounds, dim3((n + kBuildBlock - 1) / kBuildBlock), dim3(kBuildBlock), 0, s, v, idx, nv, n, keys, child, parent, arrived,
          reinterpret_cast<float4*>(kbox), reinterpret_cast<float4*>(tris), ill, nill);
    VX_KL(k_bvh_alive, dim3((2 * n - 1 + kBuildBlock - 1) / kBuildBlock), dim3(kBuildBlock), 0, s, n, parent, range, max_leaf, alive);
}

// the traversal's absolute box widening of a BVH (launch_bvh_trace's), for the TLAS's per-BLAS table
float bvh_pad(float extent, float coord_max) { return kBoxExt * extent + kBoxPos * coord_max + 1e-30f; }

// the radix tree alone (the TLAS's build sorts its own keys; vx_tlas.hip): child / parent / range as in launch_bvh_tree, parent pre-filled
void launch_bvh_karras(const uint64_t* keys, uint32_t n, uint32_t* child, uint32_t* parent, uint32_t* range, hipStream_t s)
{
    if (n > 1) VX_KL(k_bvh_karras, dim3((n - 1 + kBuildBlock - 1) / kBuildBlock), dim3(kBuildBlock), 0, s, keys, n, child, parent, range);
}

void launch_bvh_emit(uint32_t n, const uint32_t* alive, const uint32_t* newidx, const uint32_t* child, const uint32_t* range, uint32_t max_leaf,
                     const float* kbox, float* nodes, hipStream_t s)
{
    VX_KL(k_bvh_emit, dim3((2 * n - 1 + kBuildBlock - 1) / kBuildBlock), dim3(kBuildBlock), 0, s, n, alive, newidx, child, range, max_leaf,
          reinterpret_cast<const float4*>(kbox), reinterpret_cast<float4*>(nodes));
}

// ---- trace ----------------------------------------------------------------------------------------------------------------------------
namespace {

struct BvhParams {
    const float4* nodes;
    const float4* tris;
    const uint32_t* ill;  // leaf-order positions of the ill-conditioned triangles: tested by every ray, whatever the boxes say
    uint32_t nill;
    uint32_t ntri;    // 0: every ray misses
    uint32_t levels;  // LDS stack entries per lane (>= the tree's height, >= 1)
    float pad;        // box widening (absolute)
    RayArgs io;
    float* bary_out;
};

// entry t of the widened box, or false when the ray cannot have an accepted hit in it at t in [tlow, best].  k_bvh_trace calls THIS one
// (unqualified); blas::box_enter in vx_blas.h is k_tlas_trace's copy of the same text.
__device__ __forceinline__ bool box_enter(const float4& m0, const float4& m1, const SlabRay& R, float pad, float tlow, float best, float& t0)
{
    const float lo[3] = {m0.x - pad, m0.y - pad, m0.z - pad}, hi[3] = {m1.x + pad, m1.y + pad, m1.z + pad};
    float a0 = -INFINITY, a1 = INFINITY;
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p = R.inv[a] * (lo[a] - R.o[a]), q = R.inv[a] * (hi[a] - R.o[a]);
        a0 = R.deg[a] ? a0 : fmaxf(a0, fminf(p, q));
        a1 = R.deg[a] ? a1 : fminf(a1, fmaxf(p, q));
        inside &= !R.deg[a] || (lo[a] <= R.o[a] && R.o[a] <= hi[a]);
    }
    t0 = a0 - blas::kTRel * fabsf(a0);
    const float t1 = a1 + blas::kTRel * fabsf(a1);
    return inside && t0 <= t1 && t1 >= tlow && t0 <= best;
}

}  // namespace

// vx_blas.h restates this descent for k_tlas_trace (box_enter, Moeller-Trumbore, the stack walk, the normal): the two copies must change
// together (tests/test_gpu_instances.py::test_tlas_identity_matches_bvh checks them against each other bit for bit).  This kernel keeps
// its own copy because on the template it was measured 1.5 to 3 % slower on every workload.  After a side-list hit with
// any_hit this kernel still descends (`alive` stays true: root to the first leaf, no box test), while k_tlas_trace does not enter the BLAS
// at all; the contract allows either (any_hit reports `shadowed` and an arbitrary accepted t).
__global__ __launch_bounds__(kBvhBlock) void k_bvh_trace(BvhParams P)
{
    extern __shared__ uint32_t bvh_lds[];  // [level][lane]: consecutive lanes on consecutive banks
    const uint32_t tid = threadIdx.x;
    const uint64_t r = (uint64_t)blockIdx.x * kBvhBlock + tid;
    const bool active = r < P.io.nrays;

    float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 0.f, dz = 0.f;
    float best = -1.0f, bu = 0.0f, bv = 0.0f;
    uint32_t bp = blas::kNone, bk = 0;
    bool found = false;
    if (active) {
        load_ray(P.io.rays == nullptr, r, P.io.rays, P.io.cam, ox, oy, oz, dx, dy, dz);
        SlabRay R;
        make_slab_ray(ox, oy, oz, dx, dy, dz, R);
        const float tmin = P.io.tmin, tlow = fmaxf(tmin, 0.0f);
        best = P.io.tmax_per_ray ? P.io.tmax_per_ray[r] : P.io.tmax;  // acceptance bound until the first hit
        const float pad = P.pad;

        // Moeller-Trumbore exactly as include/voxhip.h pins it, and the closest-hit / tie rule
        auto test_tri = [&](uint32_t k) {
            const float4 A = P.tris[3ull * k], B = P.tris[3ull * k + 1], Cc = P.tris[3ull * k + 2];
            // Moeller-Trumbore exactly as include/voxhip.h pins it
            const float e1x = B.x - A.x, e1y = B.y - A.y, e1z = B.z - A.z;
            const float e2x = Cc.x - A.x, e2y = Cc.y - A.y, e2z = Cc.z - A.z;
            const float px = dy * e2z - dz * e2y, py = dz * e2x - dx * e2z, pz = dx * e2y - dy * e2x;
            const float det = (e1x * px + e1y * py) + e1z * pz;
            const float inv = 1.0f / det;
            const float sx = ox - A.x, sy = oy - A.y, sz = oz - A.z;
            const float u = ((sx * px + sy * py) + sz * pz) * inv;
            const float qx = sy * e1z - sz * e1y, qy = sz * e1x - sx * e1z, qz = sx * e1y - sy * e1x;
            const float v = ((dx * qx + dy * qy) + dz * qz) * inv;
            const float t = ((e2x * qx + e2y * qy) + e2z * qz) * inv;
            const uint32_t id = __float_as_uint(A.w);
            if (u >= 0.0f && u <= 1.0f && v >= 0.0f && u + v <= 1.0f && t > 0.0f && t >= tmin &&
                (found ? (t < best || (t == best && id < bp)) : t <= best)) {
                best = t; bp = id; bk = k; bu = u; bv = v; found = true;
            }
        };
        bool alive = P.ntri != 0 && !ray_nonfinite(ox, oy, oz, dx, dy, dz);  // a non-finite ray is a miss: neither the side list nor a box sees it
        for (uint32_t i = 0; i < P.nill && alive; ++i) test_tri(P.ill[i]);
        if (alive && !(found && P.io.any_hit)) {
            float t0;
            alive = box_enter(P.nodes[0], P.nodes[1], R, pad, tlow, best, t0);
        }
        uint32_t cur = 0, sp = 0;
        while (alive) {
            const float4 n0 = P.nodes[2ull * cur], n1 = P.nodes[2ull * cur + 1];
            const uint32_t na = __float_as_uint(n0.w), nb = __float_as_uint(n1.w);
            if (nb & blas::kLeafBit) {
                const uint32_t end = na + (nb & ~blas::kLeafBit);
                for (uint32_t k = na; k < end; ++k) test_tri(k);
                if (found && P.io.any_hit) break;  // gl_RayFlagsTerminateOnFirstHitEXT (raytrace.rchit:113)
            } else {
                const float4 l0 = P.nodes[2ull * na], l1 = P.nodes[2ull * na + 1];
                const float4 r0 = P.nodes[2ull * nb], r1 = P.nodes[2ull * nb + 1];
                float tl, tr;
                const bool hl = box_enter(l0, l1, R, pad, tlow, best, tl);
                const bool hr = box_enter(r0, r1, R, pad, tlow, best, tr);
                if (hl && hr) {
                    const bool lnear = tl <= tr;
                    bvh_lds[sp * kBvhBlock + tid] = lnear ? nb : na;  // sp < height <= levels: one push per interior node of the path
                    ++sp;
                    cur = lnear ? na : nb;
                    continue;
                }
                if (hl || hr) { cur = hl ? na : nb; continue; }
            }
            // next: the nearest stacked node that can still hold a hit
            bool next = false;
            while (sp > 0) {
                --sp;
                const uint32_t c = bvh_lds[sp * kBvhBlock + tid];
                if (found) {  // best has moved since the node was pushed
                    float t0;
                    if (!box_enter(P.nodes[2ull * c], P.nodes[2ull * c + 1], R, pad, tlow, best, t0)) continue;
                }
                cur = c;
                next = true;
                break;
            }
            if (!next) break;
        }
    }
    const float tt = found ? best : -1.0f;
    const uint32_t prim = found ? bp : blas::kNone;
    if (active) {
        if (P.io.t_out) P.io.t_out[r] = tt;
        if (P.io.prim_out) P.io.prim_out[r] = prim;
        if (P.io.shadowed_out) P.io.shadowed_out[r] = found ? 1 : 0;
        if (P.bary_out) { P.bary_out[2 * r] = found ? bu : 0.0f; P.bary_out[2 * r + 1] = found ? bv : 0.0f; }
        if (P.io.normal_out) {
            float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
            if (found) {  // the geometric normal cross(e1, e2) / |.| of prim, not flipped
                const float4 A = P.tris[3ull * bk], B = P.tris[3ull * bk + 1], Cc = P.tris[3ull * bk + 2];
                const float e1x = B.x - A.x, e1y = B.y - A.y, e1z = B.z - A.z;
                const float e2x = Cc.x - A.x, e2y = Cc.y - A.y, e2z = Cc.z - A.z;
                const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
                const float il = 1.0f / sqrtf((cx * cx + cy * cy) + cz * cz);
                n0 = cx * il; n1 = cy * il; n2 = cz * il;
            }
            P.io.normal_out[3 * r] = n0; P.io.normal_out[3 * r + 1] = n1; P.io.normal_out[3 * r + 2] = n2;
        }
    }
    if (P.io.hits) compact_hit(found, r, prim, tt, P.io.hits, P.io.nhits);  // every lane of the workgroup gets here
}

void launch_bvh_trace(const float* nodes, const float* tris, const uint32_t* ill, uint32_t nill, uint32_t ntri, uint32_t height, float extent,
                      float coord_max, const TraceIO& io, float* bary_out, hipStream_t s)
{
    if (!io.nrays) return;
    BvhParams P;
    std::memset(&P, 0, sizeof(P));
    P.nodes = reinterpret_cast<const float4*>(nodes);
    P.tris = reinterpret_cast<const float4*>(tris);
    P.ntri = nodes ? ntri : 0;
    P.ill = ill;
    P.nill = nodes ? nill : 0;
    P.levels = height ? height : 1u;
    P.pad = bvh_pad(extent, coord_max);
    set_ray_args(P.io, io, s);
    P.bary_out = bary_out;
    const size_t shmem = (size_t)P.levels * kBvhBlock * 4u;
    const uint64_t nblk = (io.nrays + kBvhBlock - 1) / kBvhBlock;
    VX_KL(k_bvh_trace, dim3((unsigned)nblk), dim3(kBvhBlock), shmem, s, P);
}

}  // namespace vx
