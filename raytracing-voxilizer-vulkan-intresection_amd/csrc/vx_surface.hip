// vx_surface.hip -- the boundary mesh of the bitmask (vx_grid_surface*): one quad (two triangles) per face of an occupied cell whose
// neighbour is empty or outside the grid, over the shared lattice points those faces touch.  Three kernels around two scans:
//
//   k_surf_count   lanes over the mask words: the six exposed-face words of a word of 32 cells, from the word and its neighbours at bit
//                  offsets -1, +1, -X, +X, -XY, +XY (64-bit windows of two words: rows start at any bit), the neighbours of cells on the
//                  grid's faces masked off; 2 x the popcounts = the word's triangles.  The same lanes also cover the lattice words: a
//                  lattice point (X+1 by Y+1 by Z+1 of them) is used when the 2 x 2 x 2 cells around it are mixed (cells outside the grid
//                  count as empty), one bit per point.  Per run of points along one lattice row, the four cell rows around it are read
//                  as windows of 33 bits; OR and AND over them, then over neighbouring bits, give "some occupied" and "all occupied".
//   (scans)        launch_scan_u32 over the triangle counts and over the popcounts of the corner words: each word's first triangle and
//                  first vertex, and the totals for the host.
//   k_surf_verts   lanes over the lattice words: every used point's position at its rank, org + ((float)i + 0.5f) * vs - half per axis.
//   k_surf_emit    lanes over the mask words again: the face words recomputed, and per face (ascending cell, then d) the four corners'
//                  vertex indices by the corner prefix and a popcount, two triangles, and optionally the cell's material id twice.
//
// Surface nets (vx_grid_surface_smooth*) reuse the count, the scans and k_surf_emit; the positions come from
//   k_nets_init    lanes over the corner words: per used point the 2 x 2 x 2 configuration (from the four cell rows around its run) and
//                  the lattice index, at its rank;
//   k_nets_table   one lane per vertex: u0 from the configuration, the six neighbours' vertex indices through the corner prefix;
//   k_nets_relax   one lane per vertex and step: the Jacobi step between two offset buffers;
//   k_nets_finish  one lane per vertex: org + (((float)i + 0.5f) + u) * vs - half;
//   k_nets_normals one lane per vertex: the block's mixed internal faces from the final positions.
#include "vx_internal.h"
#include "vx_mask.h"

#pragma clang fp contract(off)

namespace vx {

namespace {

constexpr unsigned kSurfBlocks = 256 * 8;

// 64 bits of the mask from bit `bit` on (any sign): words outside [0, nwords) read as empty
__device__ __forceinline__ uint64_t window(const uint32_t* __restrict__ words, uint64_t nwords, int64_t bit)
{
    const int64_t wi = bit >> 5;  // (floor)
    const uint32_t sh = (uint32_t)bit & 31u;
    const uint64_t lo = (wi >= 0 && (uint64_t)wi < nwords) ? words[wi] : 0u;
    const uint64_t hi = (wi + 1 >= 0 && (uint64_t)(wi + 1) < nwords) ? words[wi + 1] : 0u;
    return (lo | (hi << 32)) >> sh;
}

// The exposed faces of the 32 cells of word w, f[d] for d = -X, +X, -Y, +Y, -Z, +Z; returns their union (0: nothing to do).
// (x, y, z) receive the coordinates of the word's first cell.
__device__ __forceinline__ uint32_t face_words(const uint32_t* __restrict__ words, const GridParams& g, uint64_t w, uint32_t f[6],
                                               uint32_t& x0, uint32_t& y0, uint32_t& z0)
{
    const uint32_t X = g.dim[0], Y = g.dim[1];
    const uint64_t c0 = w * 32u, xy = (uint64_t)X * Y;
    const uint64_t left = g.nvox - c0;
    const uint32_t valid = left >= 32u ? ~0u : ((1u << left) - 1u);
    const uint32_t occ = words[w] & valid;
    if (!occ) return 0u;
    // the cells of the word on each face of the grid, walked with carries
    const uint64_t r = c0 / X;
    x0 = (uint32_t)(c0 - r * X);
    y0 = (uint32_t)(r % Y);
    z0 = (uint32_t)(r / Y);
    uint32_t x = x0, y = y0, z = z0;
    uint32_t bx0 = 0, bx1 = 0, by0 = 0, by1 = 0, bz0 = 0, bz1 = 0;
    const uint32_t X1 = X - 1u, Y1 = Y - 1u, Z1 = g.dim[2] - 1u;
#pragma unroll
    for (uint32_t i = 0; i < 32u; ++i) {
        const uint32_t b = 1u << i;
        bx0 |= x == 0u ? b : 0u;
        bx1 |= x == X1 ? b : 0u;
        by0 |= y == 0u ? b : 0u;
        by1 |= y == Y1 ? b : 0u;
        bz0 |= z == 0u ? b : 0u;
        bz1 |= z == Z1 ? b : 0u;
        ++x;
        if (x == X) {
            x = 0u;
            ++y;
            if (y == Y) { y = 0u; ++z; }
        }
    }
    const int64_t c = (int64_t)c0;
    const uint64_t nw = g.nwords;
    f[0] = occ & ~((uint32_t)window(words, nw, c - 1) & ~bx0);
    f[1] = occ & ~((uint32_t)window(words, nw, c + 1) & ~bx1);
    f[2] = occ & ~((uint32_t)window(words, nw, c - (int64_t)X) & ~by0);
    f[3] = occ & ~((uint32_t)window(words, nw, c + (int64_t)X) & ~by1);
    f[4] = occ & ~((uint32_t)window(words, nw, c - (int64_t)xy) & ~bz0);
    f[5] = occ & ~((uint32_t)window(words, nw, c + (int64_t)xy) & ~bz1);
    return f[0] | f[1] | f[2] | f[3] | f[4] | f[5];
}

// cells x0 - 1 .. x0 - 1 + n (n <= 32) of the row (y, z): bit t = cell x0 - 1 + t; cells outside the grid are empty
__device__ __forceinline__ uint64_t cell_run(const uint32_t* __restrict__ words, const GridParams& g, int64_t y, int64_t z, uint32_t x0, uint32_t n)
{
    const uint32_t X = g.dim[0];
    if (y < 0 || z < 0 || y >= (int64_t)g.dim[1] || z >= (int64_t)g.dim[2]) return 0u;
    const int64_t row = (int64_t)X * (y + (int64_t)g.dim[1] * z);
    uint64_t r = window(words, g.nwords, row + (int64_t)x0 - 1);
    const uint32_t lo = x0 == 0u ? 1u : 0u;             // t = 0 is cell -1
    const uint32_t hi = X - x0 < n ? X - x0 : n;        // the last t inside the row: x0 - 1 + t <= X - 1
    const uint64_t keep = ((2ull << hi) - 1ull) & ~((1ull << lo) - 1ull);
    return r & keep;
}

// corner word lw: bit t = lattice point 32 lw + t is used
__device__ __forceinline__ uint32_t corner_word(const uint32_t* __restrict__ words, const GridParams& g, uint64_t lw, uint64_t npts)
{
    const uint32_t X1 = g.dim[0] + 1u, Y1 = g.dim[1] + 1u;
    const uint64_t p0 = lw * 32u;
    const uint32_t n = npts - p0 < 32u ? (uint32_t)(npts - p0) : 32u;
    const uint64_t r = p0 / X1;
    uint32_t i = (uint32_t)(p0 - r * X1), j = (uint32_t)(r % Y1), k = (uint32_t)(r / Y1);
    uint32_t out = 0u;
    for (uint32_t p = 0; p < n;) {  // one run of points along a lattice row per step
        const uint32_t len = X1 - i < n - p ? X1 - i : n - p;
        uint64_t o = 0u, a = ~0ull;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint64_t c = cell_run(words, g, (int64_t)j - 1 + (q & 1), (int64_t)k - 1 + (q >> 1), i, len);
            o |= c;
            a &= c;
        }
        const uint64_t any = o | (o >> 1), all = a & (a >> 1);  // point i + t: cells t and t + 1 of the runs
        const uint64_t used = any & ~all & ((1ull << len) - 1ull);
        out |= (uint32_t)used << p;
        p += len;
        i += len;
        if (i == X1) {
            i = 0u;
            if (++j == Y1) { j = 0u; ++k; }
        }
    }
    return out;
}

__global__ __launch_bounds__(256) void k_surf_count(const uint32_t* __restrict__ words, GridParams g, uint32_t* __restrict__ tcount,
                                                    uint32_t* __restrict__ cmask, uint64_t nlw, uint64_t npts)
{
    const uint64_t n = g.nwords > nlw ? g.nwords : nlw;
    for (uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x; w < n; w += (uint64_t)gridDim.x * 256u) {
        if (w < g.nwords) {
            uint32_t f[6], x, y, z;
            uint32_t t = 0u;
            if (face_words(words, g, w, f, x, y, z)) {
#pragma unroll
                for (int d = 0; d < 6; ++d) t += (uint32_t)__builtin_popcount(f[d]);
            }
            tcount[w] = 2u * t;
        }
        if (w < nlw) cmask[w] = corner_word(words, g, w, npts);
    }
}

__global__ __launch_bounds__(256) void k_surf_verts(const uint32_t* __restrict__ cmask, const uint32_t* __restrict__ vpre, GridParams g,
                                                    uint64_t nlw, float* __restrict__ xyz)
{
    const uint32_t X1 = g.dim[0] + 1u, Y1 = g.dim[1] + 1u;
    for (uint64_t lw = (uint64_t)blockIdx.x * 256u + threadIdx.x; lw < nlw; lw += (uint64_t)gridDim.x * 256u) {
        uint32_t m = cmask[lw];
        if (!m) continue;
        uint64_t v = vpre[lw];
        const uint64_t p0 = lw * 32u, r = p0 / X1;
        uint32_t i = (uint32_t)(p0 - r * X1), j = (uint32_t)(r % Y1), k = (uint32_t)(r / Y1), at = 0u;
        while (m) {
            const uint32_t t = (uint32_t)__builtin_ctz(m);
            m &= m - 1u;
            for (i += t - at; i >= X1;) {  // (step along the lattice to point t)
                i -= X1;
                if (++j == Y1) { j = 0u; ++k; }
            }
            at = t;
            float* o = xyz + 3u * v++;
            o[0] = cell_centre(g.org[0], g.vs, i) - g.half;
            o[1] = cell_centre(g.org[1], g.vs, j) - g.half;
            o[2] = cell_centre(g.org[2], g.vs, k) - g.half;
        }
    }
}

// the four corners of the face in direction d, as offsets dx | dy << 1 | dz << 2, counter-clockwise seen from the empty side
constexpr uint32_t kFace[6][4] = {{0, 4, 6, 2}, {1, 3, 7, 5}, {0, 1, 5, 4}, {2, 6, 7, 3}, {0, 2, 3, 1}, {4, 5, 7, 6}};

// lattice offset of corner c (dx | dy << 1 | dz << 2)
__device__ __forceinline__ uint64_t corner_off(uint32_t c, uint64_t X1, uint64_t XY1) { return (c & 1u) + ((c >> 1) & 1u) * X1 + (c >> 2) * XY1; }

// vertex index of lattice point p: its rank among the used points
__device__ __forceinline__ int32_t vertex_of(const uint32_t* __restrict__ cmask, const uint32_t* __restrict__ vpre, uint64_t p)
{
    const uint64_t lw = p >> 5;
    return (int32_t)(vpre[lw] + (uint32_t)__builtin_popcount(cmask[lw] & ((1u << (p & 31u)) - 1u)));
}

__global__ __launch_bounds__(256) void k_surf_emit(const uint32_t* __restrict__ words, GridParams g, const uint32_t* __restrict__ tpre,
                                                   const uint32_t* __restrict__ cmask, const uint32_t* __restrict__ vpre,
                                                   const uint32_t* __restrict__ wprefix, const int16_t* __restrict__ cell_mat,
                                                   int32_t* __restrict__ tri, int32_t* __restrict__ mat)
{
    const uint32_t X = g.dim[0], Y = g.dim[1];
    const uint64_t X1 = X + 1u, XY1 = X1 * (Y + 1u);
    for (uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x; w < g.nwords; w += (uint64_t)gridDim.x * 256u) {
        uint32_t f[6], x, y, z;
        uint32_t any = face_words(words, g, w, f, x, y, z);
        if (!any) continue;
        uint64_t t = tpre[w];
        const uint32_t occ = words[w];
        uint32_t at = 0u;
        while (any) {
            const uint32_t b = (uint32_t)__builtin_ctz(any);
            any &= any - 1u;
            for (x += b - at; x >= X;) {  // (step along the grid to cell b of the word)
                x -= X;
                if (++y == Y) { y = 0u; ++z; }
            }
            at = b;
            const uint64_t base = x + X1 * (y + (uint64_t)(Y + 1u) * z);
            int32_t id = 0;
            if (mat) id = cell_mat[wprefix[w] + (uint32_t)__builtin_popcount(occ & ((1u << b) - 1u))];
#pragma unroll
            for (int d = 0; d < 6; ++d) {
                if (!((f[d] >> b) & 1u)) continue;
                const int32_t v0 = vertex_of(cmask, vpre, base + corner_off(kFace[d][0], X1, XY1));
                const int32_t v1 = vertex_of(cmask, vpre, base + corner_off(kFace[d][1], X1, XY1));
                const int32_t v2 = vertex_of(cmask, vpre, base + corner_off(kFace[d][2], X1, XY1));
                const int32_t v3 = vertex_of(cmask, vpre, base + corner_off(kFace[d][3], X1, XY1));
                int32_t* o = tri + 3u * t;
                o[0] = v0; o[1] = v1; o[2] = v2;
                o[3] = v0; o[4] = v2; o[5] = v3;
                if (mat) { mat[t] = id; mat[t + 1] = id; }
                t += 2u;
            }
        }
    }
}

// ---- surface nets (vx_grid_surface_smooth*): the same vertices and triangles, other positions, and vertex normals ---------------------
// Block configuration of a lattice point: bit a | b << 1 | e << 2 = cell (i-1+a, j-1+b, k-1+e) is occupied.
// The block's crossing edges along axis A, one bit per edge at the position of its low cell.
__device__ __forceinline__ uint32_t nets_cross(uint32_t cfg, int A)
{
    const uint32_t lo = A == 0 ? 0x55u : (A == 1 ? 0x33u : 0x0Fu);
    return (cfg ^ (cfg >> (1u << A))) & lo;
}

// bit d: the lattice point has a neighbour in direction d (the four cells on that side are mixed)
__device__ __forceinline__ uint32_t nets_neighbours(uint32_t cfg)
{
    uint32_t out = 0u;
#pragma unroll
    for (int d = 0; d < 6; ++d) {
        const uint32_t hi = (d >> 1) == 0 ? 0xAAu : ((d >> 1) == 1 ? 0xCCu : 0xF0u);
        const uint32_t s = (uint32_t)__builtin_popcount(cfg & ((d & 1) ? hi : (~hi & 0xFFu)));
        out |= (s > 0u && s < 4u) ? (1u << d) : 0u;
    }
    return out;
}

// Lanes over the corner words.  Per used point: the configuration from the four cell rows around its run, and the lattice index.
__global__ __launch_bounds__(256) void k_nets_init(const uint32_t* __restrict__ words, GridParams g, const uint32_t* __restrict__ cmask,
                                                   const uint32_t* __restrict__ vpre, uint64_t nlw, uint64_t npts,
                                                   uint8_t* __restrict__ cfg_out, uint64_t* __restrict__ lat)
{
    const uint32_t X1 = g.dim[0] + 1u, Y1 = g.dim[1] + 1u;
    for (uint64_t lw = (uint64_t)blockIdx.x * 256u + threadIdx.x; lw < nlw; lw += (uint64_t)gridDim.x * 256u) {
        const uint32_t m = cmask[lw];
        if (!m) continue;
        uint64_t v = vpre[lw];
        const uint64_t p0 = lw * 32u;
        const uint32_t n = npts - p0 < 32u ? (uint32_t)(npts - p0) : 32u;
        const uint64_t r = p0 / X1;
        uint32_t i = (uint32_t)(p0 - r * X1), j = (uint32_t)(r % Y1), k = (uint32_t)(r / Y1);
        for (uint32_t p = 0; p < n;) {  // one run of points along a lattice row per step, as corner_word
            const uint32_t len = X1 - i < n - p ? X1 - i : n - p;
            uint32_t run = (uint32_t)(((uint64_t)m >> p) & ((1ull << len) - 1ull));
            if (run) {
                uint64_t c[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) c[q] = cell_run(words, g, (int64_t)j - 1 + (q & 1), (int64_t)k - 1 + (q >> 1), i, len);
                while (run) {
                    const uint32_t t = (uint32_t)__builtin_ctz(run);
                    run &= run - 1u;
                    uint32_t cfg = 0u;
#pragma unroll
                    for (int q = 0; q < 4; ++q) cfg |= (uint32_t)((c[q] >> t) & 3ull) << (2 * q);
                    cfg_out[v] = (uint8_t)cfg;
                    lat[v] = p0 + p + t;
                    ++v;
                }
            }
            p += len;
            i += len;
            if (i == X1) {
                i = 0u;
                if (++j == Y1) { j = 0u; ++k; }
            }
        }
    }
}

// One lane per vertex: u0 from the configuration, and the six neighbours' vertex indices (-1: none), nb[d * V + v].
__global__ __launch_bounds__(256) void k_nets_table(const uint8_t* __restrict__ cfgs, const uint64_t* __restrict__ lat,
                                                    const uint32_t* __restrict__ cmask, const uint32_t* __restrict__ vpre, GridParams g,
                                                    uint64_t V, int32_t* __restrict__ nb, float* __restrict__ u0)
{
    const int64_t X1 = (int64_t)g.dim[0] + 1;
    const int64_t step[3] = {1, X1, X1 * ((int64_t)g.dim[1] + 1)};
    for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < V; v += (uint64_t)gridDim.x * 256u) {
        const uint32_t cfg = cfgs[v];
        const uint64_t P = lat[v];
        const uint32_t cr[3] = {nets_cross(cfg, 0), nets_cross(cfg, 1), nets_cross(cfg, 2)};
        const int cn[3] = {__builtin_popcount(cr[0]), __builtin_popcount(cr[1]), __builtin_popcount(cr[2])};
        const float n2 = (float)(2 * (cn[0] + cn[1] + cn[2]));
#pragma unroll
        for (int B = 0; B < 3; ++B) {  // T_B: over the crossing edges not along B, +1 where the edge's B bit is set, -1 where not
            const uint32_t hi = B == 0 ? 0xAAu : (B == 1 ? 0xCCu : 0xF0u);
            const int A0 = (B + 1) % 3, A1 = (B + 2) % 3;
            const int T = 2 * (__builtin_popcount(cr[A0] & hi) + __builtin_popcount(cr[A1] & hi)) - (cn[A0] + cn[A1]);
            u0[3u * v + B] = (float)T / n2;
        }
        const uint32_t has = nets_neighbours(cfg);
#pragma unroll
        for (int d = 0; d < 6; ++d) {
            int32_t q = -1;
            if ((has >> d) & 1u) q = vertex_of(cmask, vpre, (uint64_t)((int64_t)P + ((d & 1) ? step[d >> 1] : -step[d >> 1])));
            nb[(uint64_t)d * V + v] = q;
        }
    }
}

// One Jacobi step with weight w, one lane per vertex: uout = clamp(uin + w * (mean of the neighbours' offsets - uin)).
__global__ __launch_bounds__(256) void k_nets_relax(const int32_t* __restrict__ nb, const float* __restrict__ uin, float* __restrict__ uout,
                                                    uint64_t V, float w)
{
    for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < V; v += (uint64_t)gridDim.x * 256u) {
        int32_t q[6];
#pragma unroll
        for (int d = 0; d < 6; ++d) q[d] = nb[(uint64_t)d * V + v];
        float s[3] = {0.0f, 0.0f, 0.0f};
        uint32_t m = 0u;
#pragma unroll
        for (int d = 0; d < 6; ++d) {
            if (q[d] < 0) continue;
            const float* uq = uin + 3u * (uint64_t)q[d];
            float r[3] = {uq[0], uq[1], uq[2]};
            r[d >> 1] = ((d & 1) ? 1.0f : -1.0f) + r[d >> 1];
            s[0] = s[0] + r[0];
            s[1] = s[1] + r[1];
            s[2] = s[2] + r[2];
            ++m;
        }
        const float fm = (float)m;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float u = uin[3u * v + a];
            const float mean = s[a] / fm;
            const float t = u + w * (mean - u);
            uout[3u * v + a] = fminf(fmaxf(t, -0.5f), 0.5f);
        }
    }
}

// world positions: org + (((float)i + 0.5f) + u) * vs - half per axis
__global__ __launch_bounds__(256) void k_nets_finish(const uint64_t* __restrict__ lat, const float* __restrict__ u, GridParams g, uint64_t V,
                                                     float* __restrict__ xyz)
{
    const uint32_t X1 = g.dim[0] + 1u, Y1 = g.dim[1] + 1u;
    for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < V; v += (uint64_t)gridDim.x * 256u) {
        const uint64_t p = lat[v], r = p / X1;
        const uint32_t ijk[3] = {(uint32_t)(p - r * X1), (uint32_t)(r % Y1), (uint32_t)(r / Y1)};
#pragma unroll
        for (int a = 0; a < 3; ++a) xyz[3u * v + a] = (g.org[a] + ((((float)ijk[a] + 0.5f) + u[3u * v + a]) * g.vs)) - g.half;
    }
}

// N += cross(P(c2) - P(c0), P(c3) - P(c1)) over the face in direction D of block cell CC of lattice point p (vertex v, position own)
template <uint32_t CC, uint32_t D>
__device__ __forceinline__ void nets_face(const uint32_t* __restrict__ cmask, const uint32_t* __restrict__ vpre, const float* __restrict__ xyz,
                                          uint64_t p, const float own[3], int64_t X1, int64_t XY1, float N[3])
{
    float c[4][3];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        constexpr uint32_t kf[4] = {kFace[D][0], kFace[D][1], kFace[D][2], kFace[D][3]};
        const int ox = (int)(CC & 1u) - 1 + (int)(kf[e] & 1u), oy = (int)((CC >> 1) & 1u) - 1 + (int)((kf[e] >> 1) & 1u),
                  oz = (int)(CC >> 2) - 1 + (int)(kf[e] >> 2);
        if (ox == 0 && oy == 0 && oz == 0) {
            c[e][0] = own[0]; c[e][1] = own[1]; c[e][2] = own[2];
        } else {
            const float* q = xyz + 3u * (uint64_t)vertex_of(cmask, vpre, (uint64_t)((int64_t)p + ox + oy * X1 + oz * XY1));
            c[e][0] = q[0]; c[e][1] = q[1]; c[e][2] = q[2];
        }
    }
    const float ax = c[2][0] - c[0][0], ay = c[2][1] - c[0][1], az = c[2][2] - c[0][2];
    const float bx = c[3][0] - c[1][0], by = c[3][1] - c[1][1], bz = c[3][2] - c[1][2];
    N[0] = N[0] + (ay * bz - az * by);
    N[1] = N[1] + (az * bx - ax * bz);
    N[2] = N[2] + (ax * by - ay * bx);
}

// internal face F (0..3) across axis A of the block: low cell LO = the other two bits with the first of the other axes fastest
template <int A, int F>
__device__ __forceinline__ void nets_axis_face(uint32_t cfg, const uint32_t* __restrict__ cmask, const uint32_t* __restrict__ vpre,
                                               const float* __restrict__ xyz, uint64_t p, const float own[3], int64_t X1, int64_t XY1, float N[3])
{
    constexpr int O0 = A == 0 ? 1 : 0, O1 = A == 2 ? 1 : 2;
    constexpr uint32_t LO = (uint32_t)(((F & 1) << O0) | ((F >> 1) << O1)), HI = LO | (1u << A);
    const uint32_t lo = (cfg >> LO) & 1u, hi = (cfg >> HI) & 1u;
    if (lo == hi) return;
    if (lo) nets_face<LO, 2 * A + 1>(cmask, vpre, xyz, p, own, X1, XY1, N);
    else nets_face<HI, 2 * A>(cmask, vpre, xyz, p, own, X1, XY1, N);
}

template <int A>
__device__ __forceinline__ void nets_axis(uint32_t cfg, const uint32_t* __restrict__ cmask, const uint32_t* __restrict__ vpre,
                                          const float* __restrict__ xyz, uint64_t p, const float own[3], int64_t X1, int64_t XY1, float N[3])
{
    nets_axis_face<A, 0>(cfg, cmask, vpre, xyz, p, own, X1, XY1, N);
    nets_axis_face<A, 1>(cfg, cmask, vpre, xyz, p, own, X1, XY1, N);
    nets_axis_face<A, 2>(cfg, cmask, vpre, xyz, p, own, X1, XY1, N);
    nets_axis_face<A, 3>(cfg, cmask, vpre, xyz, p, own, X1, XY1, N);
}

// vertex normals, one lane per vertex: the block's mixed internal faces in the contract's order, from the final positions
__global__ __launch_bounds__(256) void k_nets_normals(const uint8_t* __restrict__ cfgs, const uint64_t* __restrict__ lat,
                                                      const uint32_t* __restrict__ cmask, const uint32_t* __restrict__ vpre,
                                                      const float* __restrict__ xyz, GridParams g, uint64_t V, float* __restrict__ normals)
{
    const int64_t X1 = (int64_t)g.dim[0] + 1, XY1 = X1 * ((int64_t)g.dim[1] + 1);
    for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < V; v += (uint64_t)gridDim.x * 256u) {
        const uint32_t cfg = cfgs[v];
        const uint64_t p = lat[v];
        const float own[3] = {xyz[3u * v], xyz[3u * v + 1u], xyz[3u * v + 2u]};
        float N[3] = {0.0f, 0.0f, 0.0f};
        nets_axis<0>(cfg, cmask, vpre, xyz, p, own, X1, XY1, N);
        nets_axis<1>(cfg, cmask, vpre, xyz, p, own, X1, XY1, N);
        nets_axis<2>(cfg, cmask, vpre, xyz, p, own, X1, XY1, N);
        const float l = sqrtf((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]);
        const bool ok = l > 0.0f && l < INFINITY;
        normals[3u * v] = ok ? N[0] / l : 0.0f;
        normals[3u * v + 1u] = ok ? N[1] / l : 0.0f;
        normals[3u * v + 2u] = ok ? N[2] / l : 0.0f;
    }
}

}  // namespace

SurfacePlan surface_plan(const GridParams& g)
{
    SurfacePlan p;
    p.npts = ((uint64_t)g.dim[0] + 1u) * ((uint64_t)g.dim[1] + 1u) * ((uint64_t)g.dim[2] + 1u);
    p.nlw = (p.npts + 31u) / 32u;
    return p;
}

void launch_surface_count(const uint32_t* words, const GridParams& g, const SurfacePlan& p, uint32_t* tcount, uint32_t* cmask, hipStream_t s)
{
    const uint64_t n = g.nwords > p.nlw ? g.nwords : p.nlw;
    VX_KL(k_surf_count, dim3(blocks_for(n, kSurfBlocks)), dim3(256), 0, s, words, g, tcount, cmask, p.nlw, p.npts);
}

void launch_surface_emit(const uint32_t* words, const GridParams& g, const SurfacePlan& p, const uint32_t* tpre, const uint32_t* cmask,
                         const uint32_t* vpre, const uint32_t* wprefix, const int16_t* cell_mat, float* xyz, int32_t* tri, int32_t* mat,
                         hipStream_t s)
{
    VX_KL(k_surf_verts, dim3(blocks_for(p.nlw, kSurfBlocks)), dim3(256), 0, s, cmask, vpre, g, p.nlw, xyz);
    launch_surface_tris(words, g, tpre, cmask, vpre, wprefix, cell_mat, tri, mat, s);
}

void launch_surface_tris(const uint32_t* words, const GridParams& g, const uint32_t* tpre, const uint32_t* cmask, const uint32_t* vpre,
                         const uint32_t* wprefix, const int16_t* cell_mat, int32_t* tri, int32_t* mat, hipStream_t s)
{
    VX_KL(k_surf_emit, dim3(blocks_for(g.nwords, kSurfBlocks)), dim3(256), 0, s, words, g, tpre, cmask, vpre, wprefix, cell_mat, tri, mat);
}

size_t nets_bytes(uint64_t V, NetsBufs* b)
{
    // (each array starts on a multiple of 16 bytes)
    auto up = [](uint64_t n) { return (n + 15u) & ~(uint64_t)15u; };
    uint64_t at = 0;
    const uint64_t o_lat = at; at += up(V * 8u);
    const uint64_t o_nb = at; at += up(V * 24u);
    const uint64_t o_u0 = at; at += up(V * 12u);
    const uint64_t o_u1 = at; at += up(V * 12u);
    const uint64_t o_cfg = at; at += up(V);
    if (b && b->base) {
        char* c = static_cast<char*>(b->base);
        b->lat = reinterpret_cast<uint64_t*>(c + o_lat);
        b->nb = reinterpret_cast<int32_t*>(c + o_nb);
        b->u[0] = reinterpret_cast<float*>(c + o_u0);
        b->u[1] = reinterpret_cast<float*>(c + o_u1);
        b->cfg = reinterpret_cast<uint8_t*>(c + o_cfg);
    }
    return (size_t)at + 16u;
}

void launch_surface_nets(const uint32_t* words, const GridParams& g, const SurfacePlan& p, const uint32_t* cmask, const uint32_t* vpre,
                         uint64_t V, const NetsBufs& b, uint32_t iterations, float lambda, float mu, float* xyz, float* normals, hipStream_t s)
{
    VX_KL(k_nets_init, dim3(blocks_for(p.nlw, kSurfBlocks)), dim3(256), 0, s, words, g, cmask, vpre, p.nlw, p.npts, b.cfg, b.lat);
    const dim3 grid(blocks_for(V, kSurfBlocks));
    VX_KL(k_nets_table, grid, dim3(256), 0, s, b.cfg, b.lat, cmask, vpre, g, V, b.nb, b.u[0]);
    int cur = 0;  // (the buffer that holds the current offsets: the steps ping-pong, so an odd count ends in u[1])
    for (uint32_t it = 0; it < iterations; ++it) {
        VX_KL(k_nets_relax, grid, dim3(256), 0, s, b.nb, b.u[cur], b.u[cur ^ 1], V, lambda);
        cur ^= 1;
        if (mu != 0.0f) {
            VX_KL(k_nets_relax, grid, dim3(256), 0, s, b.nb, b.u[cur], b.u[cur ^ 1], V, mu);
            cur ^= 1;
        }
    }
    VX_KL(k_nets_finish, grid, dim3(256), 0, s, b.lat, b.u[cur], g, V, xyz);
    if (normals) VX_KL(k_nets_normals, grid, dim3(256), 0, s, b.cfg, b.lat, cmask, vpre, xyz, g, V, normals);
}
}  // namespace vx
