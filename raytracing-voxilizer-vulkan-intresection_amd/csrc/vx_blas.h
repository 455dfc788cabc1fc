// vx_blas.h -- the descent of one triangle BVH (a BLAS) inside k_tlas_trace (vx_tlas.hip), restating k_bvh_trace's (vx_bvh.hip): the widened
// box test, Moeller-Trumbore in the order include/voxhip.h pins, and the front-to-back descent with its LDS stack.  The closest-hit tie
// rule is a template parameter: the triangle index alone for one BVH, (instance, triangle) lexicographically for a TLAS.  The reasoning
// behind the widening (kTRel, the per-BVH pad) is at the head of vx_bvh.hip.  k_bvh_trace keeps its own copy of this code (on this header it
// was measured slower): a change here must be made there too.  The constants below are the only copy.
#pragma once
#include "vx_internal.h"
#include "vx_ray.h"

#pragma clang fp contract(off)

namespace vx {
namespace blas {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kLeafBit = 0x80000000u;
constexpr float kTRel = 1.0f / 1024.0f;   // slab interval widening, relative to |t|

// entry t of the widened box, or false when the ray cannot have an accepted hit in it at t in [tlow, best]
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
    t0 = a0 - kTRel * fabsf(a0);
    const float t1 = a1 + kTRel * fabsf(a1);
    return inside && t0 <= t1 && t1 >= tlow && t0 <= best;
}

// the running closest hit of one ray: t, (u, v), triangle index, leaf-order position, instance (TLAS only)
struct Hit {
    float best = -1.0f, bu = 0.0f, bv = 0.0f;
    uint32_t bp = kNone, bk = 0, bi = kNone;
    bool found = false;
};

// tie rules on an equal t: a lower triangle index (one BVH) ...
struct TieTri {
    __device__ __forceinline__ static bool less(const Hit& h, uint32_t /*inst*/, uint32_t id) { return id < h.bp; }
    __device__ __forceinline__ static void take(Hit& /*h*/, uint32_t /*inst*/) {}
};
// ... or the lexicographically smaller (instance, triangle) pair (a TLAS; inst is the instance being descended)
struct TieInst {
    __device__ __forceinline__ static bool less(const Hit& h, uint32_t inst, uint32_t id) { return inst < h.bi || (inst == h.bi && id < h.bp); }
    __device__ __forceinline__ static void take(Hit& h, uint32_t inst) { h.bi = inst; }
};

// the ray of one BLAS: origin, direction, its slab form, the interval
struct Ray {
    float ox, oy, oz, dx, dy, dz;
    SlabRay R;
    float tmin, tlow;
};

// Moeller-Trumbore of the triangle at leaf-order position k, exactly as include/voxhip.h pins it, and the closest-hit / tie rule
template <class Tie>
__device__ __forceinline__ void test_tri(const float4* __restrict__ tris, uint32_t k, const Ray& y, uint32_t inst, Hit& h)
{
    const float ox = y.ox, oy = y.oy, oz = y.oz, dx = y.dx, dy = y.dy, dz = y.dz;
    const float4 A = tris[3ull * k], B = tris[3ull * k + 1], Cc = tris[3ull * k + 2];
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
    if (u >= 0.0f && u <= 1.0f && v >= 0.0f && u + v <= 1.0f && t > 0.0f && t >= y.tmin &&
        (h.found ? (t < h.best || (t == h.best && Tie::less(h, inst, id))) : t <= h.best)) {
        h.best = t; h.bp = id; h.bk = k; h.bu = u; h.bv = v; h.found = true;
        Tie::take(h, inst);
    }
}

// Front-to-back descent from the root when `alive` (the caller has entered the root's box): the nearer child first, the farther one on the
// LDS stack [level][lane] (entries sp0 .. sp0 + the BLAS's height - 1), a popped node re-tested against the best t found since.
template <class Tie, uint32_t kBlock>
__device__ __forceinline__ void descend(const float4* __restrict__ nodes, const float4* __restrict__ tris, const Ray& y, float pad, int any_hit,
                                        uint32_t* lds, uint32_t tid, uint32_t sp0, uint32_t inst, Hit& h, bool alive)
{
    uint32_t cur = 0, sp = sp0;
    while (alive) {
        const float4 n0 = nodes[2ull * cur], n1 = nodes[2ull * cur + 1];
        const uint32_t na = __float_as_uint(n0.w), nb = __float_as_uint(n1.w);
        if (nb & kLeafBit) {
            const uint32_t end = na + (nb & ~kLeafBit);
            for (uint32_t k = na; k < end; ++k) test_tri<Tie>(tris, k, y, inst, h);
            if (h.found && any_hit) break;  // gl_RayFlagsTerminateOnFirstHitEXT (raytrace.rchit:113)
        } else {
            const float4 l0 = nodes[2ull * na], l1 = nodes[2ull * na + 1];
            const float4 r0 = nodes[2ull * nb], r1 = nodes[2ull * nb + 1];
            float tl, tr;
            const bool hl = box_enter(l0, l1, y.R, pad, y.tlow, h.best, tl);
            const bool hr = box_enter(r0, r1, y.R, pad, y.tlow, h.best, tr);
            if (hl && hr) {
                const bool lnear = tl <= tr;
                lds[sp * kBlock + tid] = lnear ? nb : na;  // sp < sp0 + height <= levels: one push per interior node of the path
                ++sp;
                cur = lnear ? na : nb;
                continue;
            }
            if (hl || hr) { cur = hl ? na : nb; continue; }
        }
        // next: the nearest stacked node that can still hold a hit
        bool next = false;
        while (sp > sp0) {
            --sp;
            const uint32_t c = lds[sp * kBlock + tid];
            if (h.found) {  // best has moved since the node was pushed
                float t0;
                if (!box_enter(nodes[2ull * c], nodes[2ull * c + 1], y.R, pad, y.tlow, h.best, t0)) continue;
            }
            cur = c;
            next = true;
            break;
        }
        if (!next) break;
    }
}

// the unit geometric normal cross(e1, e2) / |.| of a triangle, not flipped
__device__ __forceinline__ void tri_normal(const float4& A, const float4& B, const float4& Cc, float& n0, float& n1, float& n2)
{
    const float e1x = B.x - A.x, e1y = B.y - A.y, e1z = B.z - A.z;
    const float e2x = Cc.x - A.x, e2y = Cc.y - A.y, e2z = Cc.z - A.z;
    const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
    const float il = 1.0f / sqrtf((cx * cx + cy * cy) + cz * cz);
    n0 = cx * il; n1 = cy * il; n2 = cz * il;
}

}  // namespace blas
}  // namespace vx
