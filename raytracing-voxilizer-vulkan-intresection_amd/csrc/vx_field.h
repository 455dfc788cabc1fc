// vx_field.h -- the sampled signed field (vx_field, voxhip.h): the trilinear interpolant of the cell-centre values of a snapshot S of
// vx_grid_sdf, clamped to the box of cell centres, its exact gradient, the occupancy of a point's cell, and the conservative sphere cast
// along a ray.  The contract is the float32 arithmetic below, in the order written, nothing fused (-ffp-contract=off plus the pragma);
// k_field_sample / k_field_trace (vx_field.hip) and the host driver of tests/test_field_cpu.py both compile this file, and
// tests/field_ref.py restates it in numpy.  Plain C++: no HIP header is needed.
#pragma once
#include "vx_math.h"

#pragma clang fp contract(off)

namespace vx {

constexpr uint32_t kFieldFinite = 0, kFieldEmpty = 1, kFieldFull = 2;  // VX_FIELD_FINITE / _EMPTY / _FULL
constexpr uint8_t kFieldMiss = 0, kFieldHit = 1, kFieldStepLimit = 2;  // VX_FIELD_MISS / _HIT / _STEP_LIMIT

struct FieldGeom {
    float org[3];
    float vs;
    uint32_t dim[3];
    uint32_t state;
};

// One axis of a point: the two cell centres around it, the weight of the upper one, and whether the field is constant along the axis there
struct FieldAxis {
    uint32_t i0, i1;
    float f;
    bool out;
};

VX_HD FieldAxis field_axis(float p, float org, float vs, uint32_t dim)
{
    FieldAxis a;
    const float top = (float)(dim - 1u);
    const float u_raw = (p - org) / vs - 0.5f;
    a.out = (u_raw < 0.0f) || (u_raw > top) || dim == 1u;
    const float u = fminf(fmaxf(u_raw, 0.0f), top);
    const uint32_t iu = (uint32_t)u, cap = dim >= 2u ? dim - 2u : 0u;
    a.i0 = iu < cap ? iu : cap;
    a.i1 = a.i0 + 1u < dim - 1u ? a.i0 + 1u : dim - 1u;
    a.f = u - (float)a.i0;
    return a;
}

// x * 0 is NaN exactly for NaN and +-Inf (ray_nonfinite of vx_ray.h, for three and for six components)
VX_HD bool field_nonfinite3(float x, float y, float z)
{
    const float s = (x * 0.0f + y * 0.0f) + z * 0.0f;
    return s != s;
}

VX_HD bool field_ray_nonfinite(const float o[3], const float d[3])
{
    const float s = ((o[0] * 0.0f + o[1] * 0.0f) + o[2] * 0.0f) + ((d[0] * 0.0f + d[1] * 0.0f) + d[2] * 0.0f);
    return s != s;
}

VX_HD float field_nan()
{
    union { uint32_t u; float f; } q;
    q.u = 0x7FC00000u;
    return q.f;
}

// two x-neighbours: adjacent floats, 4-byte aligned -- one 8-byte load
struct alignas(4) FieldPair {
    float a, b;
};

// The eight corners c[x + 2 y + 4 z].  Every load is issued before the first use: they are independent.
VX_HD void field_corners(const float* __restrict__ S, const FieldGeom& G, const FieldAxis& ax, const FieldAxis& ay, const FieldAxis& az, float c[8])
{
    const uint64_t X = G.dim[0], XY = X * G.dim[1];
    const uint64_t r00 = X * ay.i0 + XY * az.i0, r10 = X * ay.i1 + XY * az.i0, r01 = X * ay.i0 + XY * az.i1, r11 = X * ay.i1 + XY * az.i1;
    if (G.dim[0] >= 2u) {  // (i1 == i0 + 1 on every point; uniform over a batch)
        const FieldPair p00 = *reinterpret_cast<const FieldPair*>(S + r00 + ax.i0), p10 = *reinterpret_cast<const FieldPair*>(S + r10 + ax.i0);
        const FieldPair p01 = *reinterpret_cast<const FieldPair*>(S + r01 + ax.i0), p11 = *reinterpret_cast<const FieldPair*>(S + r11 + ax.i0);
        c[0] = p00.a; c[1] = p00.b; c[2] = p10.a; c[3] = p10.b; c[4] = p01.a; c[5] = p01.b; c[6] = p11.a; c[7] = p11.b;
    } else {
        const float q00 = S[r00], q10 = S[r10], q01 = S[r01], q11 = S[r11];
        c[0] = c[1] = q00; c[2] = c[3] = q10; c[4] = c[5] = q01; c[6] = c[7] = q11;
    }
}

VX_HD float field_lerp(float a, float b, float f) { return a + f * (b - a); }

VX_HD float field_interp(const float c[8], float fx, float fy, float fz)
{
    return field_lerp(field_lerp(field_lerp(c[0], c[1], fx), field_lerp(c[2], c[3], fx), fy),
                      field_lerp(field_lerp(c[4], c[5], fx), field_lerp(c[6], c[7], fx), fy), fz);
}

// the exact gradient of the interpolant; 0 along an axis on which the point lies outside the box of centres
VX_HD void field_gradient(const float c[8], const FieldAxis& ax, const FieldAxis& ay, const FieldAxis& az, float vs, float g[3])
{
    const float fx = ax.f, fy = ay.f, fz = az.f;
    const float gx = field_lerp(field_lerp(c[1] - c[0], c[3] - c[2], fy), field_lerp(c[5] - c[4], c[7] - c[6], fy), fz) / vs;
    const float gy = field_lerp(field_lerp(c[2] - c[0], c[3] - c[1], fx), field_lerp(c[6] - c[4], c[7] - c[5], fx), fz) / vs;
    const float gz = field_lerp(field_lerp(c[4] - c[0], c[5] - c[1], fx), field_lerp(c[6] - c[2], c[7] - c[3], fx), fy) / vs;
    g[0] = ax.out ? 0.0f : gx;
    g[1] = ay.out ? 0.0f : gy;
    g[2] = az.out ? 0.0f : gz;
}

// the point's own cell, where it lies in the grid's box [org, org + dim * vs)
VX_HD bool field_cell(const FieldGeom& G, const float p[3], uint64_t* cell)
{
    const float qx = (p[0] - G.org[0]) / G.vs, qy = (p[1] - G.org[1]) / G.vs, qz = (p[2] - G.org[2]) / G.vs;
    const bool in = (qx >= 0.0f) && (qx < (float)G.dim[0]) && (qy >= 0.0f) && (qy < (float)G.dim[1]) && (qz >= 0.0f) && (qz < (float)G.dim[2]);
    if (!in) return false;
    *cell = (uint64_t)(uint32_t)qx + (uint64_t)G.dim[0] * ((uint64_t)(uint32_t)qy + (uint64_t)G.dim[1] * (uint64_t)(uint32_t)qz);
    return true;
}

// value alone, as the march reads it
VX_HD float field_value(const float* __restrict__ S, const FieldGeom& G, const float p[3])
{
    if (field_nonfinite3(p[0], p[1], p[2])) return field_nan();
    if (G.state == kFieldEmpty) return INFINITY;
    if (G.state == kFieldFull) return -INFINITY;
    const FieldAxis ax = field_axis(p[0], G.org[0], G.vs, G.dim[0]), ay = field_axis(p[1], G.org[1], G.vs, G.dim[1]),
                    az = field_axis(p[2], G.org[2], G.vs, G.dim[2]);
    float c[8];
    field_corners(S, G, ax, ay, az, c);
    return field_interp(c, ax.f, ay.f, az.f);
}

// value, gradient and occupancy of one point (grad / occ: whether they are wanted)
VX_HD void field_sample(const float* __restrict__ S, const FieldGeom& G, const float p[3], bool want_grad, bool want_occ, float* value, float g[3],
                        uint8_t* occupied)
{
    *value = field_nan();
    g[0] = g[1] = g[2] = 0.0f;
    *occupied = 0;
    if (field_nonfinite3(p[0], p[1], p[2])) return;
    uint64_t cell = 0;
    const bool in = want_occ && field_cell(G, p, &cell);
    if (G.state != kFieldFinite) {
        *value = G.state == kFieldEmpty ? INFINITY : -INFINITY;
        *occupied = (in && G.state == kFieldFull) ? 1 : 0;
        return;
    }
    const FieldAxis ax = field_axis(p[0], G.org[0], G.vs, G.dim[0]), ay = field_axis(p[1], G.org[1], G.vs, G.dim[1]),
                    az = field_axis(p[2], G.org[2], G.vs, G.dim[2]);
    float c[8];
    field_corners(S, G, ax, ay, az, c);
    const float own = in ? S[cell] : 0.0f;
    *value = field_interp(c, ax.f, ay.f, az.f);
    if (want_grad) field_gradient(c, ax, ay, az, G.vs, g);
    *occupied = (in && own < 0.0f) ? 1 : 0;
}

// The sphere cast of one ray: a sphere of `radius` (world units) moved along o + t d, t in [tmin, tmax] clipped to the grid's own box.
// eps = hit_eps * vs.  Steps of step_scale * (value - radius) / |d|: with step_scale <= 1 / (2 sqrt 3) no point of the clipped segment at
// which the field is <= radius is stepped over (|grad| <= 2 sqrt 3).
VX_HD void field_march(const float* __restrict__ S, const FieldGeom& G, const float o[3], const float d[3], float tmin, float tmax, float radius,
                       float step_scale, float eps, uint32_t max_steps, float* t_out, float* clearance, uint32_t* steps, uint8_t* status)
{
    *t_out = -1.0f;
    *clearance = INFINITY;
    *steps = 0;
    *status = kFieldMiss;
    if (field_ray_nonfinite(o, d)) return;
    if (!(radius >= 0.0f) || isinf(radius)) return;  // NaN, negative, infinite
    const float dn = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    if (!(dn > 0.0f) || isinf(dn)) return;
    float t0 = tmin, t1 = tmax;
    for (int a = 0; a < 3; ++a) {
        const float lo = G.org[a], hi = G.org[a] + (float)G.dim[a] * G.vs;
        const float inv = 1.0f / d[a];
        if (isinf(inv)) {
            if (!(lo <= o[a] && o[a] <= hi)) return;
        } else {
            const float ta = (lo - o[a]) * inv, tb = (hi - o[a]) * inv;
            t0 = fmaxf(t0, fminf(ta, tb));
            t1 = fminf(t1, fmaxf(ta, tb));
        }
    }
    if (!(t0 <= t1)) return;
    float t = t0, clr = INFINITY;
    uint8_t st = kFieldStepLimit;
    uint32_t k = 0;
    while (k < max_steps) {
        const float p[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
        const float f = field_value(S, G, p);
        ++k;
        clr = fminf(clr, f);
        const float g = f - radius;
        if (g <= eps) { st = kFieldHit; break; }
        t = t + (g * step_scale) / dn;
        if (t > t1) { st = kFieldMiss; break; }
    }
    *t_out = st == kFieldHit ? t : -1.0f;
    *clearance = clr;
    *steps = k;
    *status = st;
}

}  // namespace vx
