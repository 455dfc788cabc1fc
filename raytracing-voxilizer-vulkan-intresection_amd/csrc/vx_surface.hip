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
#include "vx_internal.h"

#pragma clang fp contract(off)

namespace vx {

namespace {

constexpr unsigned kSurfBlocks = 256 * 8;

inline unsigned surf_grid(uint64_t n)
{
    uint64_t b = (n + 255) / 256;
    if (b < 1) b = 1;
    if (b > kSurfBlocks) b = kSurfBlocks;
    return (unsigned)b;
}

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
    VX_KL(k_surf_count, dim3(surf_grid(n)), dim3(256), 0, s, words, g, tcount, cmask, p.nlw, p.npts);
}

void launch_surface_emit(const uint32_t* words, const GridParams& g, const SurfacePlan& p, const uint32_t* tpre, const uint32_t* cmask,
                         const uint32_t* vpre, const uint32_t* wprefix, const int16_t* cell_mat, float* xyz, int32_t* tri, int32_t* mat,
                         hipStream_t s)
{
    VX_KL(k_surf_verts, dim3(surf_grid(p.nlw)), dim3(256), 0, s, cmask, vpre, g, p.nlw, xyz);
    VX_KL(k_surf_emit, dim3(surf_grid(g.nwords)), dim3(256), 0, s, words, g, tpre, cmask, vpre, wprefix, cell_mat, tri, mat);
}

}  // namespace vx
