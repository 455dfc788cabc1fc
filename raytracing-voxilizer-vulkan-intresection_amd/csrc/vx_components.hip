// vx_components.hip -- connected-component labelling of the bitmask (vx_grid_components*, vx_grid_component_stats).  Union-find whose
// every root is the smallest cell index of its set, in four launches around one scan; the caller's label buffer is the parent array:
//
//   k_cc_local    one workgroup per brick of 32 x 16 x 16 cells (x word-aligned), one lane per row of 32 cells read through a 64-bit
//                 window of the mask (rows start at any bit) and masked with the row's valid bits.  Union-find in LDS: every occupied
//                 cell starts at the start of its run of set bits along x, then one join per run of touching cells for every backward
//                 row offset inside the brick.  The local root of a set is its smallest local index, which is also its smallest cell
//                 index; parent[i] = the global index of that root, for occupied cells only (coalesced, one brick row per 32 lanes).
//   k_cc_merge    one lane per brick row again: every adjacent occupied pair that crosses a brick border (a row offset into another
//                 brick, or an x offset past the brick's 32 cells) is joined in global memory, once per run of touching cells, unless
//                 joins that are always made already connect it (see the comments in place; they cut the joins of a solid ~16-fold).
//   k_cc_flatten  one wave per 64 mask words, one lane per occupied cell of them: parent[i] = the root of i, and the root words (bit i:
//                 parent[i] == i) from a ballot.
//   (scan)        launch_scan_u32 over the popcounts of the root words: each word's first rank, and K.
//   k_cc_label    one lane per four cells (one per cell where the buffer is not 16-byte aligned), in place: 1 + the rank of the cell's
//                 root for occupied cells, 0 for empty cells (a lane reads only its own slots; the ranks come from the root words and
//                 their scan).  K on the device, when asked for.
//   k_cc_stats    (vx_grid_component_stats only) one lane per cell over the labels: per label present in a wave a butterfly reduce, then
//                 one integer atomic per field from one lane.
//
// Invariant of the union-find: parent[i] <= i, and parents only ever decrease.  A link goes from the larger of two roots to the smaller by
// compare-and-swap on the larger root's slot (a lost race continues from the value the CAS saw); finds halve their path with atomic min.
// So the final root of every set is its minimum cell, whatever order the races resolve in, and the numbering comes out canonical.  Across
// workgroups every read of parent is an agent-scope atomic load and every write an agent-scope CAS or min (the CUs' L1s and the XCDs' L2s
// are not coherent with each other); no workgroup ever waits for another (a CAS fails only because another lane's link made progress).
// A read that is out of date still names an ancestor (an older parent), so finds stay correct and every decision is taken by the CAS.
#include "vx_internal.h"
#include "vx_mask.h"

namespace vx {

namespace {

constexpr uint32_t kBY = 16, kBZ = 16;    // brick rows: 16 along y by 16 along z, one lane each
constexpr uint32_t kRows = kBY * kBZ;     // 256 lanes
constexpr uint32_t kCells = 32u * kRows;  // 8192 cells, 32 KiB of LDS parents
constexpr unsigned kCellBlocks = 256 * 32;

struct CcDims {
    uint32_t X, Y, Z, nbx, nby;
    uint64_t n, nwords;
};

// cells x0 .. x0 + 31 (x0 % 32 == 0: bricks are word-aligned in x) of the row whose first cell is bit `rowbit`, masked to x < X (bits past a
// row, or past the last cell, are never trusted)
__device__ __forceinline__ uint32_t row_bits(const uint32_t* __restrict__ words, uint64_t rowbit, uint32_t X, uint32_t x0)
{
    uint32_t valid;
    return row_word(words, rowbit, X, x0 >> 5, valid) & valid;
}

// ---- union-find, in LDS (SCOPE = workgroup) or in global memory (SCOPE = agent) ---------------------------------------------------
constexpr int kLds = __HIP_MEMORY_SCOPE_WORKGROUP;
constexpr int kAgent = __HIP_MEMORY_SCOPE_AGENT;

template <int SCOPE>
__device__ __forceinline__ uint32_t uf_load(uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE); }

// the root of a, halving the path on the way (parent := grandparent by atomic min: a concurrent link or halving is never undone)
template <int SCOPE>
__device__ __forceinline__ uint32_t uf_find(uint32_t* par, uint32_t a)
{
    uint32_t p = uf_load<SCOPE>(par + a);
    while (p != a) {
        const uint32_t gp = uf_load<SCOPE>(par + p);
        if (gp != p) __hip_atomic_fetch_min(par + a, gp, __ATOMIC_RELAXED, SCOPE);
        a = p;
        p = gp;
    }
    return a;
}

// join the sets of a and b: the larger root is linked to the smaller one; a lost race continues from the value the CAS saw
template <int SCOPE>
__device__ __forceinline__ void uf_unite(uint32_t* par, uint32_t a, uint32_t b)
{
    a = uf_find<SCOPE>(par, a);
    b = uf_find<SCOPE>(par, b);
    while (a != b) {
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        uint32_t seen = a;
        if (__hip_atomic_compare_exchange_strong(par + a, &seen, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE)) return;
        a = uf_find<SCOPE>(par, seen);  // a was linked meanwhile (seen < a): continue from its new root
    }
}

// the row offsets (dy, dz) of the backward neighbours: 6-connectivity joins the first two with dx = 0 only; 26-connectivity joins all
// four with dx = -1, 0, +1 (the 13th backward offset, (-1, 0, 0), is the run along x)
constexpr int kRowOff[4][2] = {{-1, 0}, {0, -1}, {-1, -1}, {1, -1}};

template <int CONN>
__global__ __launch_bounds__(256) void k_cc_local(const uint32_t* __restrict__ words, CcDims d, uint32_t* __restrict__ par)
{
    __shared__ uint32_t lp[kCells];
    __shared__ uint32_t lrow[kRows];
    const uint32_t t = threadIdx.x, yl = t % kBY, zl = t / kBY;
    uint32_t b = blockIdx.x;
    const uint32_t x0 = (b % d.nbx) * 32u;
    b /= d.nbx;
    const uint32_t y0 = (b % d.nby) * kBY, z0 = (b / d.nby) * kBZ;
    const uint32_t y = y0 + yl, z = z0 + zl;
    const uint32_t m = (y < d.Y && z < d.Z) ? row_bits(words, (uint64_t)d.X * (y + (uint64_t)d.Y * z), d.X, x0) : 0u;
    lrow[t] = m;
    if (!__syncthreads_or(m != 0u)) return;  // an empty brick
    // every occupied cell starts at the start of its run along x (the slots of empty cells are never read)
    for (uint32_t l = t; l < kCells; l += kRows) {
        const uint32_t r = lrow[l >> 5], i = l & 31u;
        const uint32_t zeros = ~r & ((1u << i) - 1u);  // the empty cells below i
        if ((r >> i) & 1u) lp[l] = (l & ~31u) + (zeros ? 32u - (uint32_t)__builtin_clz(zeros) : 0u);
    }
    __syncthreads();
    if (m) {
        constexpr int nrows = CONN == 6 ? 2 : 4;
        for (int q = 0; q < nrows; ++q) {
            const int ny = (int)yl + kRowOff[q][0], nz = (int)zl + kRowOff[q][1];
            if (ny < 0 || ny >= (int)kBY || nz < 0) continue;  // a row of another brick: k_cc_merge
            const uint32_t u = (uint32_t)ny + kBY * (uint32_t)nz;
            const uint32_t r = lrow[u];
            for (int dx = (CONN == 6 ? 0 : -1); dx <= (CONN == 6 ? 0 : 1); ++dx) {
                const uint32_t sh = dx == 0 ? r : dx < 0 ? r << 1 : r >> 1;  // bit i: the partner x + dx is occupied
                uint32_t w = m & sh;
                if (dx) w &= ~r & ~(dx < 0 ? m << 1 : m >> 1);  // implied: through (x, partner row) or (x + dx, this row) and dx = 0
                w &= ~(w << 1);  // one join per run of touching pairs: the others follow through the runs along x
                while (w) {
                    const uint32_t i = (uint32_t)__builtin_ctz(w);
                    w &= w - 1u;
                    uf_unite<kLds>(lp, t * 32u + i, u * 32u + (uint32_t)((int)i + dx));
                }
            }
        }
    }
    __syncthreads();
    // parent = the global index of the local root, occupied cells only: 32 lanes per brick row, coalesced
    const uint64_t XY = (uint64_t)d.X * d.Y;
    for (uint32_t l = t; l < kCells; l += kRows) {
        const uint32_t row = l >> 5;
        if (!((lrow[row] >> (l & 31u)) & 1u)) continue;
        uint32_t r = l;
        for (uint32_t p; (p = lp[r]) != r;) r = p;
        const uint32_t rrow = r >> 5;
        const uint64_t gi = x0 + (l & 31u) + (uint64_t)d.X * (y0 + row % kBY) + XY * (z0 + row / kBY);
        const uint64_t gr = x0 + (r & 31u) + (uint64_t)d.X * (y0 + rrow % kBY) + XY * (z0 + rrow / kBY);
        par[gi] = (uint32_t)gr;
    }
}

template <int CONN>
__global__ __launch_bounds__(256) void k_cc_merge(const uint32_t* __restrict__ words, CcDims d, uint32_t* par)
{
    const uint64_t nrow = (uint64_t)d.nbx * d.Y * d.Z;
    for (uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x; k < nrow; k += (uint64_t)gridDim.x * 256u) {
        const uint32_t x0 = (uint32_t)(k % d.nbx) * 32u;
        const uint64_t yz = k / d.nbx;
        const uint32_t y = (uint32_t)(yz % d.Y), z = (uint32_t)(yz / d.Y);
        const uint64_t c0 = (uint64_t)d.X * yz + x0;  // the row's cell x0
        const uint32_t m = row_bits(words, c0 - x0, d.X, x0);
        if (!m) continue;
        const uint32_t self_l = x0 ? mask_bit(words, c0 - 1u) : 0u;                // this row's cell x0 - 1
        const uint32_t self_r = x0 + 32u < d.X ? mask_bit(words, c0 + 32u) : 0u;  // and x0 + 32
        // (-1, 0, 0) across the x border; implied when the row below in y, inside the brick, has both cells (then the join of that row,
        // and the dx = 0 joins of both bricks, connect these two)
        if ((m & 1u) && self_l && !(y % kBY && mask_bit(words, c0 - d.X) && mask_bit(words, c0 - d.X - 1u)))
            uf_unite<kAgent>(par, (uint32_t)c0, (uint32_t)(c0 - 1u));
        constexpr int nrows = CONN == 6 ? 2 : 4;
        for (int q = 0; q < nrows; ++q) {
            const int64_t ny = (int64_t)y + kRowOff[q][0], nz = (int64_t)z + kRowOff[q][1];
            if (ny < 0 || ny >= (int64_t)d.Y || nz < 0) continue;
            const bool cross = (uint32_t)ny / kBY != y / kBY || (uint32_t)nz / kBZ != z / kBZ;
            const uint64_t n0 = (uint64_t)d.X * ((uint64_t)ny + (uint64_t)d.Y * (uint64_t)nz) + x0;  // the partner row's cell x0
            if (CONN == 6) {
                if (!cross) continue;
                uint32_t w = m & row_bits(words, n0 - x0, d.X, x0);
                w &= ~(w << 1);
                while (w) {
                    const uint32_t i = (uint32_t)__builtin_ctz(w);
                    w &= w - 1u;
                    uf_unite<kAgent>(par, (uint32_t)(c0 + i), (uint32_t)(n0 + i));
                }
                continue;
            }
            const uint32_t left = x0 ? mask_bit(words, n0 - 1u) : 0u;                // the partner row's cell x0 - 1
            const uint32_t right = x0 + 32u < d.X ? mask_bit(words, n0 + 32u) : 0u;  // and x0 + 32
            const uint32_t r = row_bits(words, n0 - x0, d.X, x0);
            if (!cross) {  // a row of the same brick: only the x offsets past the brick's 32 cells, unless implied as in k_cc_local
                if ((m & 1u) && left && !(r & 1u) && !self_l) uf_unite<kAgent>(par, (uint32_t)c0, (uint32_t)(n0 - 1u));
                if ((m >> 31) && right && !(r >> 31) && !self_r) uf_unite<kAgent>(par, (uint32_t)(c0 + 31u), (uint32_t)(n0 + 32u));
                continue;
            }
            for (int dx = -1; dx <= 1; ++dx) {
                const uint32_t sh = dx == 0 ? r : dx < 0 ? (r << 1) | left : (r >> 1) | (right << 31);
                uint32_t w = m & sh;
                if (dx) w &= ~r & ~(dx < 0 ? (m << 1) | self_l : (m >> 1) | (self_r << 31));
                w &= ~(w << 1);
                while (w) {
                    const uint32_t i = (uint32_t)__builtin_ctz(w);
                    w &= w - 1u;
                    uf_unite<kAgent>(par, (uint32_t)(c0 + i), (uint32_t)((int64_t)n0 + i + dx));
                }
            }
        }
    }
}

// one wave per 64 mask words: each lane loads one word, then the wave walks the non-empty words two at a time, one lane per cell (a
// sparse grid costs one load and one store per word; a dense one keeps 64 finds in flight per wave).  The loop bounds are wave-uniform, so
// every ballot sees the whole wave.  The roots are final once k_cc_merge has ended; here only halvings write, so every find ends at the
// true root.
__global__ __launch_bounds__(256) void k_cc_flatten(const uint32_t* __restrict__ words, uint64_t n, uint64_t nwords, uint32_t* par,
                                                    uint32_t* __restrict__ roots)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t wb = ((uint64_t)blockIdx.x * 256u + threadIdx.x - lane); wb < nwords; wb += (uint64_t)gridDim.x * 256u) {
        const uint64_t w = wb + lane;
        const uint64_t left = w < nwords ? n - 32u * w : 0u;
        const uint32_t mw = w < nwords ? words[w] & (left >= 32u ? ~0u : ((1u << left) - 1u)) : 0u;
        uint32_t rw = 0u;
        unsigned long long nz = __ballot(mw != 0u);
        while (nz) {
            const uint32_t j0 = (uint32_t)__builtin_ctzll(nz);
            nz &= nz - 1ull;
            const uint32_t j1 = nz ? (uint32_t)__builtin_ctzll(nz) : 64u;
            if (nz) nz &= nz - 1ull;
            const uint32_t j = lane < 32u ? j0 : j1, b = lane & 31u;
            const uint32_t mj = (uint32_t)__shfl((int)mw, (int)(j & 63u), 64);
            bool root = false;
            if (j < 64u && ((mj >> b) & 1u)) {
                const uint32_t i = (uint32_t)(32u * (wb + j) + b);
                const uint32_t p = uf_load<kAgent>(par + i);
                const uint32_t r = p == i ? i : uf_find<kAgent>(par, i);
                if (r != p) __hip_atomic_fetch_min(par + i, r, __ATOMIC_RELAXED, kAgent);
                root = r == i;
            }
            const unsigned long long bits = __ballot(root);
            if (lane == j0) rw = (uint32_t)bits;
            if (lane == j1) rw = (uint32_t)(bits >> 32);
        }
        if (w < nwords) roots[w] = rw;
    }
}

__device__ __forceinline__ uint32_t rank_label(const uint32_t* __restrict__ roots, const uint32_t* __restrict__ rpre, uint32_t r)
{
    return 1u + rpre[r >> 5] + (uint32_t)__builtin_popcount(roots[r >> 5] & ((1u << (r & 31u)) - 1u));
}

// VEC4: X*Y*Z % 4 == 0 and a 16-byte aligned buffer: four cells per lane, one 16-byte store (no parent read where all four are empty)
template <bool VEC4>
__global__ __launch_bounds__(256) void k_cc_label(const uint32_t* __restrict__ words, uint64_t n, uint64_t nwords, uint32_t* __restrict__ par,
                                                  const uint32_t* __restrict__ roots, const uint32_t* __restrict__ rpre, uint32_t* __restrict__ count)
{
    if (count && blockIdx.x == 0 && threadIdx.x == 0) *count = rpre[nwords - 1] + (uint32_t)__builtin_popcount(roots[nwords - 1]);
    if (VEC4) {
        for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < n / 4u; q += (uint64_t)gridDim.x * 256u) {
            const uint32_t nib = (words[q >> 3] >> ((q & 7u) * 4u)) & 15u;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (nib) {
                const uint4 p = reinterpret_cast<const uint4*>(par)[q];
                if (nib & 1u) v.x = rank_label(roots, rpre, p.x);
                if (nib & 2u) v.y = rank_label(roots, rpre, p.y);
                if (nib & 4u) v.z = rank_label(roots, rpre, p.z);
                if (nib & 8u) v.w = rank_label(roots, rpre, p.w);
            }
            reinterpret_cast<uint4*>(par)[q] = v;
        }
        return;
    }
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u)
        par[i] = mask_bit(words, i) ? rank_label(roots, rpre, par[i]) : 0u;
}

// rec: 8 words per component (vx_component: cells as two words, min[3], max[3])
__global__ __launch_bounds__(256) void k_cc_stats_init(uint32_t* __restrict__ rec, uint64_t k)
{
    for (uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x; j < k * 8u; j += (uint64_t)gridDim.x * 256u)
        rec[j] = ((j & 7u) >= 2u && (j & 7u) < 5u) ? ~0u : 0u;
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
#pragma unroll
    for (int s = 32; s; s >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, s, 64); v = o < v ? o : v; }
    return v;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
#pragma unroll
    for (int s = 32; s; s >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, s, 64); v = o > v ? o : v; }
    return v;
}

__global__ __launch_bounds__(256) void k_cc_stats(const uint32_t* __restrict__ labels, CcDims d, uint32_t* __restrict__ rec)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t XY = (uint64_t)d.X * d.Y;
    for (uint64_t base = ((uint64_t)blockIdx.x * 256u + threadIdx.x) & ~63ull; base < d.n; base += (uint64_t)gridDim.x * 256u) {
        const uint64_t i = base + lane;
        const uint32_t lab = i < d.n ? labels[i] : 0u;
        const uint32_t z = (uint32_t)(i / XY), y = (uint32_t)((i - z * XY) / d.X), x = (uint32_t)(i - z * XY - (uint64_t)y * d.X);
        unsigned long long act = __ballot(lab != 0u);
        while (act) {  // one label of the wave per step
            const int leader = __ffsll((long long)act) - 1;
            const uint32_t L = (uint32_t)__shfl((int)lab, leader, 64);
            const bool mine = lab == L;
            const unsigned long long mm = __ballot(mine);
            act &= ~mm;
            const uint32_t v[6] = {wave_min(mine ? x : ~0u), wave_min(mine ? y : ~0u), wave_min(mine ? z : ~0u),
                                   wave_max(mine ? x : 0u),  wave_max(mine ? y : 0u),  wave_max(mine ? z : 0u)};
            if ((int)lane == leader) {
                uint32_t* r = rec + 8ull * (L - 1u);
                atomicAdd(reinterpret_cast<unsigned long long*>(r), (unsigned long long)__popcll(mm));
                for (int a = 0; a < 3; ++a) {
                    atomicMin(r + 2 + a, v[a]);
                    atomicMax(r + 5 + a, v[3 + a]);
                }
            }
        }
    }
}

CcDims cc_dims(const GridParams& g)
{
    CcDims d;
    d.X = g.dim[0];
    d.Y = g.dim[1];
    d.Z = g.dim[2];
    d.nbx = (d.X + 31u) / 32u;
    d.nby = (d.Y + kBY - 1u) / kBY;
    d.n = g.nvox;
    d.nwords = g.nwords;
    return d;
}

}  // namespace

void launch_components(const uint32_t* words, const GridParams& g, bool conn26, uint32_t* labels, uint32_t* roots, hipStream_t s)
{
    const CcDims d = cc_dims(g);
    const uint64_t nbricks = (uint64_t)d.nbx * d.nby * ((d.Z + kBZ - 1u) / kBZ);
    const uint64_t nrow = (uint64_t)d.nbx * d.Y * d.Z;
    if (conn26) {
        VX_KL(k_cc_local<26>, dim3((unsigned)nbricks), dim3(256), 0, s, words, d, labels);
        VX_KL(k_cc_merge<26>, dim3(blocks_for(nrow, kCellBlocks)), dim3(256), 0, s, words, d, labels);
    } else {
        VX_KL(k_cc_local<6>, dim3((unsigned)nbricks), dim3(256), 0, s, words, d, labels);
        VX_KL(k_cc_merge<6>, dim3(blocks_for(nrow, kCellBlocks)), dim3(256), 0, s, words, d, labels);
    }
    VX_KL(k_cc_flatten, dim3(blocks_for(d.nwords, kCellBlocks)), dim3(256), 0, s, words, d.n, d.nwords, labels, roots);  // (one lane per word)
}

void launch_components_label(const uint32_t* words, const GridParams& g, uint32_t* labels, const uint32_t* roots, const uint32_t* rpre,
                             uint32_t* dev_count, hipStream_t s)
{
    if (g.nvox % 4u == 0u && (reinterpret_cast<uintptr_t>(labels) & 15u) == 0u)
        VX_KL(k_cc_label<true>, dim3(blocks_for(g.nvox / 4u, kCellBlocks)), dim3(256), 0, s, words, g.nvox, g.nwords, labels, roots, rpre, dev_count);
    else
        VX_KL(k_cc_label<false>, dim3(blocks_for(g.nvox, kCellBlocks)), dim3(256), 0, s, words, g.nvox, g.nwords, labels, roots, rpre, dev_count);
}

void launch_component_stats(const uint32_t* labels, const GridParams& g, uint64_t k, uint32_t* rec, hipStream_t s)
{
    VX_KL(k_cc_stats_init, dim3(blocks_for(k * 8u, kCellBlocks)), dim3(256), 0, s, rec, k);
    VX_KL(k_cc_stats, dim3(blocks_for(g.nvox, kCellBlocks)), dim3(256), 0, s, labels, cc_dims(g), rec);
}

}  // namespace vx
