// Host driver of csrc/vx_field.h for tests/test_field_cpu.py: the sample and the sphere cast of a field and a batch read from a file, as the
// kernels compile them.  g++ -O2 -ffp-contract=off -fno-fast-math -I csrc.
//   field_host IN OUT
// IN:  u32 dim[3], f32 vs, f32 org[3], u32 state, u64 npoints, u64 nrays, f32 tmin, tmax, radius, step_scale, hit_eps, u32 max_steps,
//      u32 has_tmax_per_ray, u32 has_radius_per_ray, then f32 S[X*Y*Z], points[3 n], rays[6 m], tmax_per_ray[m]?, radius_per_ray[m]?
// OUT: f32 value[n], gradient[3 n], u8 occupied[n], f32 t[m], clearance[m], u32 steps[m], u8 status[m]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vx_field.h"

struct Header {
    uint32_t dim[3];
    float vs;
    float org[3];
    uint32_t state;
    uint64_t npoints, nrays;
    float tmin, tmax, radius, step_scale, hit_eps;
    uint32_t max_steps, has_tmax, has_radius;
};

template <class T> static bool get(FILE* f, std::vector<T>& v, size_t n)
{
    v.resize(n);
    return !n || fread(v.data(), sizeof(T), n, f) == n;
}

template <class T> static bool put(FILE* f, const std::vector<T>& v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 3;
    Header h;
    if (fread(&h, sizeof(h), 1, in) != 1) return 4;
    std::vector<float> S, pts, rays, tmaxpr, radpr;
    const size_t N = (size_t)h.dim[0] * h.dim[1] * h.dim[2], n = (size_t)h.npoints, m = (size_t)h.nrays;
    if (!get(in, S, N) || !get(in, pts, 3 * n) || !get(in, rays, 6 * m) || !get(in, tmaxpr, h.has_tmax ? m : 0) || !get(in, radpr, h.has_radius ? m : 0)) return 5;
    fclose(in);
    vx::FieldGeom G;
    for (int a = 0; a < 3; ++a) { G.dim[a] = h.dim[a]; G.org[a] = h.org[a]; }
    G.vs = h.vs;
    G.state = h.state;
    std::vector<float> value(n), grad(3 * n), t(m), clr(m);
    std::vector<uint8_t> occ(n), status(m);
    std::vector<uint32_t> steps(m);
    for (size_t i = 0; i < n; ++i) vx::field_sample(S.data(), G, &pts[3 * i], true, true, &value[i], &grad[3 * i], &occ[i]);
    for (size_t i = 0; i < m; ++i)
        vx::field_march(S.data(), G, &rays[6 * i], &rays[6 * i + 3], h.tmin, h.has_tmax ? tmaxpr[i] : h.tmax, h.has_radius ? radpr[i] : h.radius, h.step_scale,
                        h.hit_eps * G.vs, h.max_steps, &t[i], &clr[i], &steps[i], &status[i]);
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 6;
    const bool ok = put(out, value) && put(out, grad) && put(out, occ) && put(out, t) && put(out, clr) && put(out, steps) && put(out, status);
    return fclose(out) == 0 && ok ? 0 : 7;
}
