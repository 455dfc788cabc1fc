// vx_poses.h -- pose queries on a vx_field (voxhip.h, "pose queries"): a body of P points with radii, N body-to-world transforms, and per
// pose the smallest clearance g = value(q) - radius over the body's points, the point that has it, the number of points within a margin,
// and the contact position and normal.  The contract is the float32 arithmetic below, in the order written, nothing fused
// (-ffp-contract=off plus the pragma); k_field_poses / k_field_poses_finish (vx_poses.hip) and the host driver of tests/test_poses_cpu.py
// both compile this file, and tests/poses_ref.py restates it in numpy.  Plain C++: no HIP header is needed.
#pragma once
#include "vx_field.h"

#pragma clang fp contract(off)

namespace vx {

constexpr uint64_t kPoseNone = ~0ull;          // the key of "no point": larger than every key of a point
constexpr uint32_t kPoseNoPoint = 0xFFFFFFFFu;  // `point` of a pose without one

// q = M p: row-major 3 x 4, the layout of vx_tlas_instance.transform
VX_HD void pose_point(const float* __restrict__ m, const float p[3], float q[3])
{
    for (int a = 0; a < 3; ++a) q[a] = ((m[4 * a] * p[0] + m[4 * a + 1] * p[1]) + m[4 * a + 2] * p[2]) + m[4 * a + 3];
}

// the clearance of one posed point; NaN: the point is skipped.  The + 0.0f turns -0 into +0, so equal values have equal bits.
VX_HD float pose_gap(const float* __restrict__ S, const FieldGeom& G, const float* __restrict__ m, const float p[3], float radius)
{
    float q[3];
    pose_point(m, p, q);
    const float v = field_value(S, G, q);
    return (v - radius) + 0.0f;
}

VX_HD uint32_t pose_float_bits(float x)
{
    union { float f; uint32_t u; } c;
    c.f = x;
    return c.u;
}

VX_HD float pose_bits_float(uint32_t u)
{
    union { float f; uint32_t u; } c;
    c.u = u;
    return c.f;
}

// the monotone map of float bits to u32: a < b as floats <=> orderable(a) < orderable(b).  No NaN reaches it, and no -0: the largest
// value, that of +inf, is 0xFF800000, so 0xFFFFFFFF never is one
VX_HD uint32_t pose_orderable(float g)
{
    const uint32_t u = pose_float_bits(g);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

VX_HD float pose_unorder(uint32_t o) { return pose_bits_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o); }

// orderable(g) << 32 | i: the smallest key is the smallest g, and among equal g the lowest index
VX_HD uint64_t pose_key(float g, uint32_t i) { return g != g ? kPoseNone : (((uint64_t)pose_orderable(g) << 32) | i); }

VX_HD bool pose_within(float g, float margin) { return g <= margin; }  // (false for a NaN g)

// A pose's outputs from its reduced key: the position is recomputed, the gradient is field_sample's there
VX_HD void pose_finish(const float* __restrict__ S, const FieldGeom& G, const float* __restrict__ m, const float* __restrict__ points, uint64_t key,
                       bool want_position, bool want_gradient, float* clearance, uint32_t* point, float position[3], float gradient[3])
{
    *clearance = INFINITY;
    *point = kPoseNoPoint;
    position[0] = position[1] = position[2] = 0.0f;
    gradient[0] = gradient[1] = gradient[2] = 0.0f;
    if (key == kPoseNone) return;
    const uint32_t i = (uint32_t)key;
    *clearance = pose_unorder((uint32_t)(key >> 32));
    *point = i;
    if (!want_position && !want_gradient) return;
    const float p[3] = {points[3 * (uint64_t)i], points[3 * (uint64_t)i + 1], points[3 * (uint64_t)i + 2]};
    pose_point(m, p, position);
    if (want_gradient) {
        float v;
        uint8_t occ;
        field_sample(S, G, position, true, false, &v, gradient, &occ);
    }
}

}  // namespace vx
