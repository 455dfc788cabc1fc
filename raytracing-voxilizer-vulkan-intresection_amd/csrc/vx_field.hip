// vx_field.hip -- batch queries on a vx_field: k_field_sample (trilinear value, gradient, occupancy of arbitrary points) and k_field_trace
// (the sphere cast).  The arithmetic is vx_field.h's, which a host driver compiles too.  One point / one ray per lane, 256-thread
// workgroups, no LDS: both kernels are bound by the latency of the eight-corner gather (four 8-byte loads, issued together), the field is
// read-only and shared by the whole batch, so L2 and the Infinity Cache do the reuse.
#include "vx_internal.h"
#include "vx_ray.h"
#include "vx_field.h"

#pragma clang fp contract(off)

namespace vx {

__global__ __launch_bounds__(256) void k_field_sample(const float* __restrict__ S, FieldGeom G, const float* __restrict__ points, uint64_t n,
                                                      float* __restrict__ value, float* __restrict__ gradient, uint8_t* __restrict__ occupied)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const float p[3] = {points[3 * r], points[3 * r + 1], points[3 * r + 2]};
    float v, g[3];
    uint8_t occ;
    field_sample(S, G, p, gradient != nullptr, occupied != nullptr, &v, g, &occ);
    if (value) value[r] = v;
    if (gradient) { gradient[3 * r] = g[0]; gradient[3 * r + 1] = g[1]; gradient[3 * r + 2] = g[2]; }
    if (occupied) occupied[r] = occ;
}

__global__ __launch_bounds__(256) void k_field_trace(const float* __restrict__ S, FieldGeom G, FieldTraceIO io)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= io.nrays) return;
    float o[3], d[3];
    load_ray(false, r, io.rays, nullptr, o[0], o[1], o[2], d[0], d[1], d[2]);
    const float tmax = io.tmax_per_ray ? io.tmax_per_ray[r] : io.tmax;
    const float radius = io.radius_per_ray ? io.radius_per_ray[r] : io.radius;
    float t, clr;
    uint32_t steps;
    uint8_t status;
    field_march(S, G, o, d, io.tmin, tmax, radius, io.step_scale, io.hit_eps * G.vs, io.max_steps, &t, &clr, &steps, &status);
    if (io.t) io.t[r] = t;
    if (io.clearance) io.clearance[r] = clr;
    if (io.steps) io.steps[r] = steps;
    if (io.status) io.status[r] = status;
}

void launch_field_sample(const float* S, const FieldGeom& G, const float* points, uint64_t n, float* value, float* gradient, uint8_t* occupied,
                         hipStream_t s)
{
    if (!n) return;
    VX_KL(k_field_sample, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, S, G, points, n, value, gradient, occupied);
}

void launch_field_trace(const float* S, const FieldGeom& G, const FieldTraceIO& io, hipStream_t s)
{
    if (!io.nrays) return;
    VX_KL(k_field_trace, dim3((unsigned)((io.nrays + 255) / 256)), dim3(256), 0, s, S, G, io);
}

}  // namespace vx
