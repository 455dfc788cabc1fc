// vx_solid.hip -- solid voxelization (VX_VOXELIZE_SOLID, vx_grid_fill_interior): the empty cells that no 6-connected path of empty
// cells joins to the grid's boundary are filled.  A flood fill on bits of the EXTERIOR, grown from the empty boundary cells in rounds:
//
//   layout   a padded, row-aligned copy: W = ceil(X / 32) words per (y, z) row, word (r = y + Y z, w) at r W + w; bits past X are solid.
//            With X % 32 == 0 this IS the reference's bitmask, which is then read in place.
//   seed     k_solid_seed     mask -> padded mask (X % 32 != 0), exterior = the empty cells of the boundary
//   round    k_solid_x        per row: carry fill forward and backward (the add trick; v_bfrev_b32 for the backward direction), the carry
//                             handed from word to word along the row
//            k_solid_col_agg  per chunk of 8 / 16 steps of a word column along y, then z: its (pass, gen) words for both directions
//            k_solid_col_carry one wave per column: the scan of those words, every chunk's exclusive forward / backward carry
//            k_solid_col      per chunk: from its two carries, the runs of empty cells closed (F | B)
//   finish   k_solid_finish   H = empty & ~exterior, back into the reference layout; the mask becomes S | H
//
// Round control: every kernel of a round ORs 1 into its round's flag word when it grows the exterior; every kernel of a round first
// reads the flag of the round before and exits at once when that round was quiet (the fixpoint).  The host queues rounds in batches and
// reads one word per batch through the handle's mailbox (k_solid_report); there is no grid-wide barrier and no cap on the rounds.
// Nothing is exchanged between workgroups inside a launch: every thread owns the words it writes, kernel boundaries order the rest.
#include "vx_internal.h"
#include "vx_mask.h"

#pragma clang fp contract(off)

namespace vx {

namespace {

constexpr unsigned kSolidBlocks = 256 * 8;

// V consecutive words: one 16-byte access for V == 4
template <int V> struct Words { uint32_t w[V]; };
template <int V> __device__ __forceinline__ Words<V> ld(const uint32_t* p)
{
    Words<V> r;
    if constexpr (V == 4) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        r.w[0] = q.x; r.w[1] = q.y; r.w[2] = q.z; r.w[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) r.w[j] = p[j];
    }
    return r;
}
template <int V> __device__ __forceinline__ void st(uint32_t* p, const Words<V>& r)
{
    if constexpr (V == 4) {
        *reinterpret_cast<uint4*>(p) = make_uint4(r.w[0], r.w[1], r.w[2], r.w[3]);
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) p[j] = r.w[j];
    }
}

// The bits of `p` (empty cells) reachable from a bit of `g` (exterior, g within p) by steps towards higher bits inside p.  Adding the
// lowest bit of every run of p to the run's non-exterior cells ripples a carry up to the first exterior cell of the run and leaves the
// cells above it alone; a run without an exterior cell is cleared completely (its carry dies in the solid bit behind it).
__device__ __forceinline__ uint32_t fill_up(uint32_t p, uint32_t g)
{
    const uint32_t r = (p & ~g) + (p & ~(p << 1));
    return p & (g | r);
}
__device__ __forceinline__ uint32_t fill_down(uint32_t p, uint32_t g)
{
    return __builtin_bitreverse32(fill_up(__builtin_bitreverse32(p), __builtin_bitreverse32(g)));
}

__device__ __forceinline__ void mark_changed(bool changed, uint32_t* flag)
{
    if (__any(changed) && (threadIdx.x & 63u) == 0u) *flag = 1u;
}

// ---- seed: padded mask (pad != 0) and the boundary's empty cells ----
__global__ __launch_bounds__(256) void k_solid_seed(const uint32_t* __restrict__ words, uint32_t* __restrict__ mp /*null: words is the padded mask*/,
                                                    uint32_t* __restrict__ ext, uint32_t X, uint32_t Y, uint32_t Z, uint32_t W, uint32_t* __restrict__ flag)
{
    const uint64_t n = (uint64_t)W * Y * Z;
    if (blockIdx.x == 0 && threadIdx.x == 0) *flag = 1u;  // "the round before the first one changed something"
    const uint32_t hi_bit = 1u << ((X - 1u) & 31u);
    for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < n; q += (uint64_t)gridDim.x * 256u) {
        const uint64_t r = q / W;
        const uint32_t w = (uint32_t)(q - r * W);
        const uint32_t z = (uint32_t)(r / Y);
        const uint32_t y = (uint32_t)(r - (uint64_t)z * Y);
        uint32_t m;
        if (mp) {
            uint32_t valid;  // this padded word's cells in the reference's bit order
            m = (row_word(words, r * X, X, w, valid) & valid) | ~valid;
            mp[q] = m;
        } else {
            m = words[q];
        }
        const uint32_t p = ~m;
        uint32_t e;
        if (y == 0u || y == Y - 1u || z == 0u || z == Z - 1u) e = p;
        else e = p & ((w == 0u ? 1u : 0u) | (w == W - 1u ? hi_bit : 0u));
        ext[q] = e;
    }
}

// ---- along x: one row per thread, forward then backward, the carry handed across the row's words ----
template <int V>
__global__ __launch_bounds__(256) void k_solid_x(const uint32_t* __restrict__ m, uint32_t* __restrict__ ext, uint64_t rows, uint32_t W,
                                                 const uint32_t* __restrict__ prev_flag, uint32_t* __restrict__ flag)
{
    if (*prev_flag == 0u) return;  // the round before was quiet: the fixpoint is reached
    bool changed = false;
    for (uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x; r < rows; r += (uint64_t)gridDim.x * 256u) {
        const uint64_t base = r * W;
        uint32_t c = 0u;
        for (uint32_t w = 0; w < W; w += V) {
            const Words<V> mm = ld<V>(m + base + w);
            Words<V> e = ld<V>(ext + base + w);
            bool ch = false;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const uint32_t p = ~mm.w[j];
                const uint32_t f = fill_up(p, e.w[j] | (c & p));
                c = f >> 31;
                ch |= f != e.w[j];
                e.w[j] = f;
            }
            if (ch) st<V>(ext + base + w, e);
            changed |= ch;
        }
        c = 0u;
        for (uint32_t w = W; w > 0; w -= V) {
            const Words<V> mm = ld<V>(m + base + w - V);
            Words<V> e = ld<V>(ext + base + w - V);
            bool ch = false;
#pragma unroll
            for (int j = V - 1; j >= 0; --j) {
                const uint32_t p = ~mm.w[j];
                const uint32_t f = fill_down(p, e.w[j] | (c & p));
                c = (f & 1u) << 31;
                ch |= f != e.w[j];
                e.w[j] = f;
            }
            if (ch) st<V>(ext + base + w - V, e);
            changed |= ch;
        }
    }
    mark_changed(changed, flag);
}

// ---- along y (outer = z, step = one row) or z (outer = y, step = one slice): a two-pass scan over chunks of kChunk<V> steps ----
// Along a line the closure is exact in one go: a cell is exterior when its run of empty cells holds an exterior cell, i.e. the forward fill
// F(i) = e(i) | (p(i) & F(i-1)) OR the backward fill, both of the ORIGINAL e.  Each step is the map r -> e | (p & r); a chunk of them composes to
// r -> g | (q & r) with q = AND of the p's: the (pass, gen) operator (p2 & p1, (g1 & p2) | g2).  Pass 1 (k_solid_col_agg) writes q and the
// forward / backward g of every chunk of V-word columns; pass 2 (k_solid_col_carry), one wave per column, scans those in both directions, 64
// chunks per step, and leaves every chunk its exclusive forward / backward carry in place of its g words; pass 3 (k_solid_col) re-runs its
// chunk from the two carries and stores what grew.  Linear work: every pass reads each of its words once.  Units: chunk-major within a column (o, c, g), the V-word column group g fastest, so that neighbouring lanes read
// neighbouring 16-byte pieces of a row.
// (steps per chunk: 8 for 16-byte columns, 16 for single words -- the chunk's mask, exterior and result words stay in registers)
template <int V> constexpr uint32_t kChunk = V == 4 ? 8u : 16u;

template <int V>
__device__ __forceinline__ void col_unit(uint64_t u, uint32_t groups, uint32_t nch, uint64_t outer_stride, uint64_t step, uint32_t nsteps,
                                         uint64_t& base, uint32_t& c, uint32_t& i0, uint32_t& i1)
{
    const uint64_t oc = u / groups;
    const uint32_t g = (uint32_t)(u - oc * groups);
    const uint64_t o = oc / nch;
    c = (uint32_t)(oc - o * nch);
    base = o * outer_stride + (uint64_t)g * V;
    i0 = c * kChunk<V>;
    i1 = i0 + kChunk<V> < nsteps ? i0 + kChunk<V> : nsteps;
}

template <int V>
__global__ __launch_bounds__(256) void k_solid_col_agg(const uint32_t* __restrict__ m, const uint32_t* __restrict__ ext, uint32_t* __restrict__ agg,
                                                       uint64_t nouter, uint64_t outer_stride, uint32_t groups, uint64_t step, uint32_t nsteps, uint32_t nch,
                                                       const uint32_t* __restrict__ prev_flag)
{
    if (*prev_flag == 0u) return;
    const uint64_t units = nouter * nch * groups;
    for (uint64_t u = (uint64_t)blockIdx.x * 256u + threadIdx.x; u < units; u += (uint64_t)gridDim.x * 256u) {
        uint64_t base;
        uint32_t c, i0, i1;
        col_unit<V>(u, groups, nch, outer_stride, step, nsteps, base, c, i0, i1);
        Words<V> mm[kChunk<V>], e[kChunk<V>];
#pragma unroll
        for (uint32_t k = 0; k < kChunk<V>; ++k)
            if (i0 + k < i1) { mm[k] = ld<V>(m + base + (uint64_t)(i0 + k) * step); e[k] = ld<V>(ext + base + (uint64_t)(i0 + k) * step); }
        Words<V> q, gf, gb;
#pragma unroll
        for (int j = 0; j < V; ++j) { q.w[j] = ~0u; gf.w[j] = 0u; gb.w[j] = 0u; }
#pragma unroll
        for (uint32_t k = 0; k < kChunk<V>; ++k)
            if (i0 + k < i1) {
#pragma unroll
                for (int j = 0; j < V; ++j) { q.w[j] &= ~mm[k].w[j]; gf.w[j] = e[k].w[j] | (~mm[k].w[j] & gf.w[j]); }
            }
#pragma unroll
        for (int k = (int)kChunk<V> - 1; k >= 0; --k)
            if (i0 + (uint32_t)k < i1) {
#pragma unroll
                for (int j = 0; j < V; ++j) gb.w[j] = e[k].w[j] | (~mm[k].w[j] & gb.w[j]);
            }
        uint32_t* a = agg + u * (3u * V);
        st<V>(a, q);
        st<V>(a + V, gf);
        st<V>(a + 2 * V, gb);
    }
}

// one wave per column (o, g); its chunks k at agg unit (o nch + k) groups + g.  dir 0: forward over k, dir 1: backward (lane order = descending
// k).  A Kogge-Stone scan of the (pass, gen) operator over the wave's 64 chunks, applied to the carry coming from the previous 64; the lane
// stores the carry INTO its chunk (the exclusive value) over the g words it read.  Lanes past the column's end carry the identity (~0, 0).
template <int V>
__global__ __launch_bounds__(256) void k_solid_col_carry(uint32_t* __restrict__ agg, uint64_t ncols, uint32_t groups, uint32_t nch,
                                                         const uint32_t* __restrict__ prev_flag)
{
    if (*prev_flag == 0u) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nwaves = ((uint64_t)gridDim.x * 256u) >> 6;
    for (uint64_t cidx = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 6; cidx < ncols; cidx += nwaves) {  // (wave-uniform)
        const uint64_t o = cidx / groups;
        const uint64_t unit0 = o * nch * groups + (cidx - o * groups);
        for (uint32_t dir = 0; dir < 2; ++dir) {
            Words<V> carry;
#pragma unroll
            for (int j = 0; j < V; ++j) carry.w[j] = 0u;
            for (uint32_t b = 0; b < nch; b += 64u) {
                const uint32_t i = b + lane;
                const bool valid = i < nch;
                const uint32_t k = dir == 0 ? i : nch - 1u - i;
                uint32_t* a = agg + (unit0 + (uint64_t)(valid ? k : 0u) * groups) * (3u * V);
                Words<V> q, g;
#pragma unroll
                for (int j = 0; j < V; ++j) { q.w[j] = ~0u; g.w[j] = 0u; }
                if (valid) { q = ld<V>(a); g = ld<V>(a + V + dir * V); }
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        const uint32_t oq = __shfl_up(q.w[j], d, 64), og = __shfl_up(g.w[j], d, 64);
                        if (lane >= (uint32_t)d) { g.w[j] = (og & q.w[j]) | g.w[j]; q.w[j] &= oq; }
                    }
                }
                Words<V> ex;
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const uint32_t incl = g.w[j] | (q.w[j] & carry.w[j]);
                    const uint32_t prev = __shfl_up(incl, 1, 64);
                    ex.w[j] = lane == 0u ? carry.w[j] : prev;
                    carry.w[j] = __shfl(incl, 63, 64);
                }
                if (valid) st<V>(a + V + dir * V, ex);
            }
        }
    }
}

template <int V>
__global__ __launch_bounds__(256) void k_solid_col(const uint32_t* __restrict__ m, uint32_t* __restrict__ ext, const uint32_t* __restrict__ agg,
                                                   uint64_t nouter, uint64_t outer_stride, uint32_t groups, uint64_t step, uint32_t nsteps, uint32_t nch,
                                                   const uint32_t* __restrict__ prev_flag, uint32_t* __restrict__ flag)
{
    if (*prev_flag == 0u) return;
    bool changed = false;
    const uint64_t units = nouter * nch * groups;
    for (uint64_t u = (uint64_t)blockIdx.x * 256u + threadIdx.x; u < units; u += (uint64_t)gridDim.x * 256u) {
        uint64_t base;
        uint32_t c, i0, i1;
        col_unit<V>(u, groups, nch, outer_stride, step, nsteps, base, c, i0, i1);
        // the chunk's own words, then its carries (k_solid_col_carry)
        Words<V> mm[kChunk<V>], e[kChunk<V>];
#pragma unroll
        for (uint32_t k = 0; k < kChunk<V>; ++k)
            if (i0 + k < i1) { mm[k] = ld<V>(m + base + (uint64_t)(i0 + k) * step); e[k] = ld<V>(ext + base + (uint64_t)(i0 + k) * step); }
        Words<V> cf = ld<V>(agg + u * (3u * V) + V), cb = ld<V>(agg + u * (3u * V) + 2 * V);
        Words<V> f[kChunk<V>];
#pragma unroll
        for (uint32_t k = 0; k < kChunk<V>; ++k)
            if (i0 + k < i1) {
#pragma unroll
                for (int j = 0; j < V; ++j) { cf.w[j] = e[k].w[j] | (~mm[k].w[j] & cf.w[j]); f[k].w[j] = cf.w[j]; }
            }
#pragma unroll
        for (int k = (int)kChunk<V> - 1; k >= 0; --k)
            if (i0 + (uint32_t)k < i1) {
                bool ch = false;
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    cb.w[j] = e[k].w[j] | (~mm[k].w[j] & cb.w[j]);
                    f[k].w[j] |= cb.w[j];
                    ch |= f[k].w[j] != e[k].w[j];
                }
                if (ch) st<V>(ext + base + (uint64_t)(i0 + (uint32_t)k) * step, f[k]);
                changed |= ch;
            }
    }
    mark_changed(changed, flag);
}

// ---- one thread: the batch's rounds that changed something, into the host's mailbox word ----
__global__ void k_solid_report(const uint32_t* __restrict__ flags, uint32_t nrounds, unsigned long long* out, unsigned long long tag)
{
    uint32_t n = 0;
    for (uint32_t k = 0; k < nrounds; ++k) n += flags[k] ? 1u : 0u;
    *out = tag | n;
}

// ---- H = empty & ~exterior, OR-ed into the reference's bitmask; h receives H in the reference layout ----
// aligned (X % 32 == 0): m == words, h == ext (H replaces the exterior in place)
__global__ __launch_bounds__(256) void k_solid_finish_aligned(uint32_t* __restrict__ words, uint32_t* __restrict__ ext, uint64_t nwords)
{
    for (uint64_t i = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 4u; i < nwords; i += (uint64_t)gridDim.x * 1024u) {
        if (i + 4u <= nwords) {
            Words<4> w = ld<4>(words + i), e = ld<4>(ext + i);
            bool any = false;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                e.w[j] = ~(w.w[j] | e.w[j]);
                any |= e.w[j] != 0u;
                w.w[j] |= e.w[j];
            }
            st<4>(ext + i, e);
            if (any) st<4>(words + i, w);
        } else {
            for (uint64_t k = i; k < nwords; ++k) {
                const uint32_t h = ~(words[k] | ext[k]);
                ext[k] = h;
                if (h) words[k] |= h;
            }
        }
    }
}
// padded: every reference word gathers its bits from the padded words of the rows it covers (two for X >= 32, up to 32 for narrow rows)
__global__ __launch_bounds__(256) void k_solid_finish_padded(uint32_t* __restrict__ words, const uint32_t* __restrict__ mp, const uint32_t* __restrict__ ext,
                                                             uint32_t* __restrict__ h, uint64_t nwords, uint64_t nvox, uint32_t X, uint32_t W)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nwords; i += (uint64_t)gridDim.x * 256u) {
        const uint64_t b0 = i * 32u;
        const uint64_t end = b0 + 32u < nvox ? b0 + 32u : nvox;
        uint32_t out = 0u;
        uint64_t b = b0;
        uint64_t r = b / X;
        uint32_t x = (uint32_t)(b - r * X);
        while (b < end) {
            const uint32_t off = x & 31u;
            uint32_t n = 32u - off;
            if (X - x < n) n = X - x;
            if (end - b < n) n = (uint32_t)(end - b);
            const uint64_t q = r * W + (x >> 5);
            const uint32_t hv = ~(mp[q] | ext[q]) >> off;
            out |= (n == 32u ? hv : (hv & ((1u << n) - 1u))) << (uint32_t)(b - b0);
            b += n;
            x += n;
            if (x == X) { x = 0u; ++r; }
        }
        h[i] = out;
        if (out) words[i] |= out;
    }
}

__global__ __launch_bounds__(256) void k_solid_ids(int16_t* __restrict__ ids, uint64_t n, int16_t v, int only_unset)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u)
        if (!only_unset || ids[i] < 0) ids[i] = v;
}

}  // namespace

SolidPlan solid_plan(const uint32_t dim[3])
{
    SolidPlan p;
    p.W = (dim[0] + 31u) / 32u;
    p.padded = (dim[0] % 32u) != 0u;
    p.pwords = (uint64_t)p.W * dim[1] * dim[2];
    return p;
}

void launch_solid_seed(const uint32_t* words, uint32_t* mp, uint32_t* ext, const uint32_t dim[3], uint32_t* flag, hipStream_t s)
{
    const SolidPlan p = solid_plan(dim);
    VX_KL(k_solid_seed, dim3(blocks_for(p.pwords, kSolidBlocks)), dim3(256), 0, s, words, p.padded ? mp : nullptr, ext, dim[0], dim[1], dim[2], p.W, flag);
}

template <int V>
static void solid_col(const uint32_t* m, uint32_t* ext, uint32_t* agg, uint64_t nouter, uint64_t outer_stride, uint32_t groups, uint64_t step,
                      uint32_t nsteps, const uint32_t* prev_flag, uint32_t* flag, hipStream_t s)
{
    const uint32_t nch = (nsteps + kChunk<V> - 1) / kChunk<V>;
    const uint64_t units = nouter * nch * groups;
    VX_KL(k_solid_col_agg<V>, dim3(blocks_for(units, kSolidBlocks)), dim3(256), 0, s, m, ext, agg, nouter, outer_stride, groups, step, nsteps, nch, prev_flag);
    const uint64_t ncols = nouter * groups;
    VX_KL(k_solid_col_carry<V>, dim3(blocks_for(ncols * 64, kSolidBlocks)), dim3(256), 0, s, agg, ncols, groups, nch, prev_flag);
    VX_KL(k_solid_col<V>, dim3(blocks_for(units, kSolidBlocks)), dim3(256), 0, s, m, ext, agg, nouter, outer_stride, groups, step, nsteps, nch, prev_flag, flag);
}

uint64_t solid_agg_words(const uint32_t dim[3])
{
    const SolidPlan p = solid_plan(dim);
    const uint64_t y = (uint64_t)dim[2] * p.W * ((dim[1] + kChunk<4> - 1) / kChunk<4>), z = (uint64_t)dim[1] * p.W * ((dim[2] + kChunk<4> - 1) / kChunk<4>);
    return 3ull * (y > z ? y : z);
}

void launch_solid_round(const uint32_t* m, uint32_t* ext, uint32_t* agg, const uint32_t dim[3], const uint32_t* prev_flag, uint32_t* flag, hipStream_t s)
{
    const SolidPlan p = solid_plan(dim);
    const uint64_t rows = (uint64_t)dim[1] * dim[2];
    const uint64_t yw = (uint64_t)dim[1] * p.W;
    if (p.W % 4u == 0u) {
        VX_KL(k_solid_x<4>, dim3(blocks_for(rows, kSolidBlocks)), dim3(256), 0, s, m, ext, rows, p.W, prev_flag, flag);
        solid_col<4>(m, ext, agg, dim[2], yw, p.W / 4u, p.W, dim[1], prev_flag, flag, s);
        solid_col<4>(m, ext, agg, dim[1], p.W, p.W / 4u, yw, dim[2], prev_flag, flag, s);
    } else {
        VX_KL(k_solid_x<1>, dim3(blocks_for(rows, kSolidBlocks)), dim3(256), 0, s, m, ext, rows, p.W, prev_flag, flag);
        solid_col<1>(m, ext, agg, dim[2], yw, p.W, p.W, dim[1], prev_flag, flag, s);
        solid_col<1>(m, ext, agg, dim[1], p.W, p.W, yw, dim[2], prev_flag, flag, s);
    }
}

void launch_solid_report(const uint32_t* flags, uint32_t nrounds, unsigned long long* out, unsigned long long tag, hipStream_t s)
{
    VX_KL(k_solid_report, dim3(1), dim3(1), 0, s, flags, nrounds, out, tag);
}

void launch_solid_finish(uint32_t* words, const uint32_t* mp, uint32_t* ext, uint32_t* h, const uint32_t dim[3], uint64_t nwords, hipStream_t s)
{
    const SolidPlan p = solid_plan(dim);
    if (!p.padded) {
        VX_KL(k_solid_finish_aligned, dim3(blocks_for((nwords + 3) / 4, kSolidBlocks)), dim3(256), 0, s, words, ext, nwords);
    } else {
        const uint64_t nvox = (uint64_t)dim[0] * dim[1] * dim[2];
        VX_KL(k_solid_finish_padded, dim3(blocks_for(nwords, kSolidBlocks)), dim3(256), 0, s, words, mp, ext, h, nwords, nvox, dim[0], p.W);
    }
}

void launch_solid_ids(int16_t* ids, uint64_t n, int16_t v, bool only_unset, hipStream_t s)
{
    if (!n) return;
    VX_KL(k_solid_ids, dim3(blocks_for(n, kSolidBlocks)), dim3(256), 0, s, ids, n, v, only_unset ? 1 : 0);
}

}  // namespace vx
