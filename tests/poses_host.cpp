// Host driver of csrc/vx_poses.h for tests/test_poses_cpu.py: the pose query of a field, a body and a batch of transforms read from a file,
// reduced through the same keys as the kernels.  g++ -O2 -ffp-contract=off -fno-fast-math -I csrc.
//   poses_host IN OUT
// IN:  u32 dim[3], f32 vs, f32 org[3], u32 state, u64 npoints, u64 nposes, f32 margin, u32 has_radii, then f32 S[X*Y*Z], points[3 P],
//      radii[P]?, transforms[12 N]
// OUT: f32 clearance[N], u32 point[N], u32 count[N], f32 position[3 N], f32 gradient[3 N]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vx_poses.h"

struct Header {
    uint32_t dim[3];
    float vs;
    float org[3];
    uint32_t state;
    uint64_t npoints, nposes;
    float margin;
    uint32_t has_radii;
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
    std::vector<float> S, pts, radii, xf;
    const size_t cells = (size_t)h.dim[0] * h.dim[1] * h.dim[2], P = (size_t)h.npoints, N = (size_t)h.nposes;
    if (!get(in, S, cells) || !get(in, pts, 3 * P) || !get(in, radii, h.has_radii ? P : 0) || !get(in, xf, 12 * N)) return 5;
    fclose(in);
    vx::FieldGeom G;
    for (int a = 0; a < 3; ++a) { G.dim[a] = h.dim[a]; G.org[a] = h.org[a]; }
    G.vs = h.vs;
    G.state = h.state;
    std::vector<float> clearance(N), position(3 * N), gradient(3 * N);
    std::vector<uint32_t> point(N), count(N);
    for (size_t n = 0; n < N; ++n) {
        const float* m = &xf[12 * n];
        uint64_t key = vx::kPoseNone;
        uint32_t c = 0;
        for (size_t i = 0; i < P; ++i) {
            const float g = vx::pose_gap(S.data(), G, m, &pts[3 * i], h.has_radii ? radii[i] : 0.0f);
            const uint64_t k = vx::pose_key(g, (uint32_t)i);
            key = k < key ? k : key;
            c += vx::pose_within(g, h.margin) ? 1u : 0u;
        }
        count[n] = c;
        vx::pose_finish(S.data(), G, m, pts.data(), key, true, true, &clearance[n], &point[n], &position[3 * n], &gradient[3 * n]);
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 6;
    const bool ok = put(out, clearance) && put(out, point) && put(out, count) && put(out, position) && put(out, gradient);
    return fclose(out) == 0 && ok ? 0 : 7;
}
