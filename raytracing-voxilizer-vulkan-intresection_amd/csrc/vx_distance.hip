// vx_distance.hip -- exact squared Euclidean distance fields of the bitmask (vx_grid_distance_sq*, vx_grid_sdf*).  Separable, one pass per
// axis, integer arithmetic only until the signed field's final conversion:
//
//   x pass   k_dist_x     one row (y, z) per thread, straight from the reference's bitmask (rows start at any bit: X % 32 != 0 is read as
//                         vx_solid.hip reads it, through a 64-bit window of two words).  Per word of the row, the nearest target cell to the
//                         left and right of every cell comes from clz / ctz of the masked word, with the last target of the words before
//                         (carried) and the first target of the words after (a look-ahead pointer that only moves forward): every word is
//                         read at most twice per target kind, linear in the row.  Out: dx^2, or the sentinel when the row has no target.
//   y, z     k_dist_col   one column per thread, adjacent threads on adjacent x (the loads and stores of a step coalesce): Meijster's exact
//                         1-D lower envelope of the parabolas (q - u)^2 + g(u) in two sweeps, sentinels skipped, separators in 64-bit
//                         integers.  The envelope's stack (s | t << 16, g(s)) lives in global scratch laid out [k][column] (8 bytes an
//                         entry, column length entries per column): columns of any length up to 65536.  Phase 1 reads the whole column
//                         before phase 2 writes it, and the stack keeps g(s): the pass runs in place.
//
// Modes: OUT (targets = occupied cells; 0 on M), IN (targets = empty cells; 0 off M) and SIGNED: each cell carries the transform it needs
// (D_in on M, D_out off M) in the one 32-bit intermediate -- the other transform is 0 there, known from the mask -- and the column passes run
// both envelopes over the one buffer, g_out(u) = m(u) ? 0 : v(u), g_in(u) = m(u) ? v(u) : 0.  The z pass of SIGNED converts to f32 in place.
//
// The feature transform (vx_grid_nearest*: the INDEX of the nearest target, smallest index on ties) runs the same passes and carries WHICH
// target wins instead of how far it is: k_near_x and k_near_col are the same row sweep and the same envelope with another expression per cell
// and another second word in the stack entry (NearCell, FeatureWord).
#include "vx_internal.h"
#include "vx_mask.h"

#pragma clang fp contract(off)

namespace vx {

namespace {

constexpr uint32_t kInf = 0xFFFFFFFFu;  // no target in reach (the contract's sentinel)
constexpr uint32_t kNone = 0xFFFFFFFFu; // no target position, no feature
constexpr unsigned kDistBlocks = 256 * 8;

enum : int { kOut = 0, kIn = 1, kSigned = 2 };

// ---- x pass: the row sweep ---------------------------------------------------------------------------------------------------------------
// The nearest target of a row at or after word w + 1: `lw` the word it lies in (W: none), `pos` its cell.  Moves forward only.
struct Ahead {
    uint32_t lw, pos;
};
template <bool OCC>
__device__ __forceinline__ void ahead_from(Ahead& a, const uint32_t* __restrict__ words, uint64_t rowbit, uint32_t X, uint32_t W, uint32_t w)
{
    for (a.lw = w; a.lw < W; ++a.lw) {
        uint32_t valid;
        const uint32_t m = row_word(words, rowbit, X, a.lw, valid);
        const uint32_t t = (OCC ? m : ~m) & valid;
        if (t) { a.pos = 32u * a.lw + (uint32_t)__builtin_ctz(t); return; }
    }
    a.pos = kNone;
}

// distance along the row from cell x (bit i of word w) to the nearest target: t = the word's targets, prev / next = the carried ones
__device__ __forceinline__ uint32_t row_dist(uint32_t t, uint32_t i, uint32_t x, uint32_t prev, uint32_t next)
{
    const uint32_t lo = t & ((2u << i) - 1u);  // targets at or below i (i = 31: 2u << 31 == 0, all bits)
    const uint32_t hi = t >> i;                 // targets at or above i
    const uint32_t dl = lo ? i - (31u - (uint32_t)__builtin_clz(lo)) : (prev != kNone ? x - prev : kInf);
    const uint32_t dr = hi ? (uint32_t)__builtin_ctz(hi) : (next != kNone ? next - x : kInf);
    const uint32_t d = dl < dr ? dl : dr;
    return d == kInf ? kInf : d * d;  // d <= 65535: d^2 < 2^32 - 1
}

// position along the row of the nearest target of cell x (bit i of word w), the left one on a tie; kNone: the row has none
__device__ __forceinline__ uint32_t row_near(uint32_t t, uint32_t i, uint32_t x, uint32_t prev, uint32_t next)
{
    const uint32_t lo = t & ((2u << i) - 1u);
    const uint32_t hi = t >> i;
    const uint32_t pl = lo ? x - i + (31u - (uint32_t)__builtin_clz(lo)) : prev;
    const uint32_t pr = hi ? x + (uint32_t)__builtin_ctz(hi) : next;
    const uint32_t dl = pl != kNone ? x - pl : kInf;
    const uint32_t dr = pr != kNone ? pr - x : kInf;
    return dl <= dr ? pl : pr;
}

// What the sweep writes per cell: which target kinds it follows (kOcc, kEmp), and the value of cell x = bit i of the word m from the word's
// occupied and empty targets to / te, the last target of either kind before the word (po, pe) and the first after it (no, ne).
template <int MODE>
struct DistCell {  // dx^2, or the sentinel when the row has no target; SIGNED: to the empty cells on M, to the occupied ones off M
    static constexpr bool kOcc = MODE != kIn, kEmp = MODE != kOut;
    static __device__ __forceinline__ uint32_t at(uint32_t m, uint32_t i, uint32_t x, uint32_t to, uint32_t te, uint32_t po, uint32_t pe,
                                                  uint32_t no, uint32_t ne)
    {
        if (MODE == kOut) return row_dist(to, i, x, po, no);
        if (MODE == kIn) return row_dist(te, i, x, pe, ne);
        return (m >> i) & 1u ? row_dist(te, i, x, pe, ne) : row_dist(to, i, x, po, no);
    }
};
template <bool OCC>
struct NearCell {  // x' of the nearest target
    static constexpr bool kOcc = OCC, kEmp = !OCC;
    static __device__ __forceinline__ uint32_t at(uint32_t, uint32_t i, uint32_t x, uint32_t to, uint32_t te, uint32_t po, uint32_t pe,
                                                  uint32_t no, uint32_t ne)
    {
        return OCC ? row_near(to, i, x, po, no) : row_near(te, i, x, pe, ne);
    }
};

// One row (y, z) per thread.  VEC4: X % 4 == 0 and `out` is 16-byte aligned, so rows start on 16-byte boundaries.
// (The state stays in plain locals: packed into one struct per target kind, k_near_x came out 3-6 % slower)
template <class CELL, bool VEC4>
__device__ __forceinline__ void row_sweep(const uint32_t* __restrict__ words, uint32_t* __restrict__ out, uint32_t X, uint64_t rows)
{
    const uint32_t W = (X + 31u) / 32u;
    for (uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x; r < rows; r += (uint64_t)gridDim.x * 256u) {
        const uint64_t rowbit = r * X;
        uint32_t* o = out + rowbit;
        uint32_t prev_occ = kNone, prev_emp = kNone;  // last target of the words before
        Ahead ao{0u, kNone}, ae{0u, kNone};           // first target of the words after
        if (CELL::kOcc) ahead_from<true>(ao, words, rowbit, X, W, 1u);
        if (CELL::kEmp) ahead_from<false>(ae, words, rowbit, X, W, 1u);
        for (uint32_t w = 0; w < W; ++w) {
            if (CELL::kOcc && ao.lw == w) ahead_from<true>(ao, words, rowbit, X, W, w + 1u);
            if (CELL::kEmp && ae.lw == w) ahead_from<false>(ae, words, rowbit, X, W, w + 1u);
            uint32_t valid;
            const uint32_t m = row_word(words, rowbit, X, w, valid);
            const uint32_t to = m & valid, te = ~m & valid;  // padding bits are neither occupied nor empty
            const uint32_t nb = (uint32_t)__builtin_popcount(valid);
            uint32_t v[32];
#pragma unroll
            for (uint32_t i = 0; i < 32u; ++i) v[i] = CELL::at(m, i, 32u * w + i, to, te, prev_occ, prev_emp, ao.pos, ae.pos);
            if (VEC4) {  // the row and nb are multiples of four cells
#pragma unroll
                for (uint32_t i = 0; i < 32u; i += 4u)
                    if (i < nb) *reinterpret_cast<uint4*>(o + 32u * w + i) = make_uint4(v[i], v[i + 1], v[i + 2], v[i + 3]);
            } else {
#pragma unroll
                for (uint32_t i = 0; i < 32u; ++i)
                    if (i < nb) o[32u * w + i] = v[i];
            }
            if (CELL::kOcc && to) prev_occ = 32u * w + 31u - (uint32_t)__builtin_clz(to);
            if (CELL::kEmp && te) prev_emp = 32u * w + 31u - (uint32_t)__builtin_clz(te);
        }
    }
}

template <int MODE, bool VEC4>
__global__ __launch_bounds__(256) void k_dist_x(const uint32_t* __restrict__ words, uint32_t* __restrict__ out, uint32_t X, uint64_t rows)
{
    row_sweep<DistCell<MODE>, VEC4>(words, out, X, rows);
}

template <bool OCC, bool VEC4>
__global__ __launch_bounds__(256) void k_near_x(const uint32_t* __restrict__ words, uint32_t* __restrict__ out, uint32_t X, uint64_t rows)
{
    row_sweep<NearCell<OCC>, VEC4>(words, out, X, rows);
}

// ---- y and z passes: the envelope --------------------------------------------------------------------------------------------------------
// What the second word of a stack entry is: how g(s) comes out of it, and what the pass writes to a cell u where s wins with the value d.
// The distance fields keep g itself and write d.  The feature transform keeps the packed feature x' | y' << 16 of the cell's nearest target
// so far, the one 32-bit intermediate it has per cell, and recomputes g from it and the column's own position on every load: (x - x')^2
// after the x pass, (x - x')^2 + (y - y')^2 after the y pass (y pass: f >> 16 == 0).  It writes the feature extended by s.
// x' | y' << 16 == kNone would need X = Y = 65536, which the distance fields' limit excludes.
struct DistWord {
    __device__ __forceinline__ uint32_t g(uint32_t word) const { return word; }
    __device__ __forceinline__ uint32_t result(uint32_t, uint32_t, uint32_t d) const { return d; }
};
template <bool ZPASS>
struct FeatureWord {
    uint32_t x, y, X, Y;  // the column's position, the grid's size
    __device__ __forceinline__ uint32_t g(uint32_t f) const
    {
        const uint32_t dx = x - (f & 0xFFFFu);  // (the square of a wrapped difference is the square of the difference: below 2^32)
        uint32_t g = dx * dx;
        if (ZPASS) {
            const uint32_t dy = y - (f >> 16);
            g += dy * dy;
        }
        return g;
    }
    // y pass: x' | y' << 16 with y' = s.  z pass: the cell index x' + X (y' + Y z') with z' = s.
    // (the value d is not used: env_take computes it for every policy, and the compiler drops it here)
    __device__ __forceinline__ uint32_t result(uint32_t s, uint32_t f, uint32_t) const
    {
        return ZPASS ? (f & 0xFFFFu) + X * ((f >> 16) + Y * s) : f | (s << 16);
    }
};

// One lower envelope of a column (Meijster): entries k = 0..q, parabola s_k with value g_k, winning from t_k on; the top in registers,
// every entry also at stk[k * ld] (s | t << 16, word) -- s, t < 65536.  g(s) is kept for the top only, through G.
template <class G>
struct Env {
    uint2* stk;
    uint64_t ld;
    int q;
    uint32_t s, t, word, g;
    G of;
};

template <class G>
__device__ __forceinline__ void env_init(Env<G>& e, uint2* stk, uint64_t ld, G of = G())
{
    e.stk = stk;
    e.ld = ld;
    e.q = -1;
    e.s = e.t = e.word = e.g = 0u;
    e.of = of;
}
template <class G>
__device__ __forceinline__ void env_load(Env<G>& e)
{
    const uint2 v = e.stk[(uint64_t)e.q * e.ld];
    e.s = v.x & 0xFFFFu;
    e.t = v.x >> 16;
    e.word = v.y;
    e.g = e.of.g(v.y);
}
template <class G>
__device__ __forceinline__ void env_push(Env<G>& e, uint32_t s, uint32_t t, uint32_t word, uint32_t g)
{
    ++e.q;
    e.s = s;
    e.t = t;
    e.word = word;
    e.g = g;
    e.stk[(uint64_t)e.q * e.ld] = make_uint2(s | (t << 16), word);
}
__device__ __forceinline__ uint64_t para(uint32_t x, uint32_t s, uint32_t g)
{
    const int64_t d = (int64_t)x - (int64_t)s;
    return (uint64_t)(d * d) + g;
}

// phase 1, one cell u of a column of n with its word (kInf / kNone: skipped, never pushed): the parabolas u now beats at their start are
// dropped -- only by a strictly better newcomer -- then u starts where it first beats the top.  Ties so keep the smaller s.
template <class G>
__device__ __forceinline__ void env_add(Env<G>& e, uint32_t u, uint32_t word, uint32_t n)
{
    if (word == kInf) return;
    const uint32_t gu = e.of.g(word);
    while (e.q >= 0 && para(e.t, e.s, e.g) > para(e.t, u, gu)) {
        if (--e.q >= 0) env_load(e);
    }
    if (e.q < 0) { env_push(e, u, 0u, word, gu); return; }
    // Sep(s, u) = floor((u^2 - s^2 + g_u - g_s) / (2 (u - s))); not popped: the crossing lies at or past t >= 0, the numerator is >= 0
    const int64_t num = (int64_t)u * u - (int64_t)e.s * e.s + (int64_t)gu - (int64_t)e.g;
    const int64_t den = 2 * ((int64_t)u - (int64_t)e.s);
    const int64_t w = (num >= 0 ? num / den : -((-num + den - 1) / den)) + 1;
    if (w < (int64_t)n) env_push(e, u, (uint32_t)w, word, gu);
}

// phase 2, cells u = n-1 down to 0: the result at u of the parabola that wins there (kInf / kNone: the envelope is empty), its value being
// the exact minimum, within the grid's 32-bit limit; then the entry that starts at u is dropped
template <class G>
__device__ __forceinline__ uint32_t env_take(Env<G>& e, uint32_t u)
{
    if (e.q < 0) return kInf;
    const uint32_t v = e.of.result(e.s, e.word, (uint32_t)para(u, e.s, e.g));
    if (u == e.t && --e.q >= 0) env_load(e);
    return v;
}

// Columns c < ncols of n cells: cell j of column c at base(c) + j * stride with base(c) = c % X + (c / X) * outer.
// y pass: ncols = X Z, outer = X Y, stride = X.  z pass: ncols = X Y, outer = X, stride = X Y.
// stk: n * ncols entries per envelope.  Phase 1 reads the whole column before phase 2 writes it: the passes run in place.

// SIGNED: two envelopes over the one buffer (stk: the in-envelope's entries follow the out-envelope's); TO_F32: the z pass converts in place.
template <int MODE, bool TO_F32>
__global__ __launch_bounds__(256) void k_dist_col(const uint32_t* __restrict__ words, uint32_t* __restrict__ buf, uint2* __restrict__ stk,
                                                  uint32_t X, uint64_t ncols, uint64_t outer, uint64_t stride, uint32_t n, float vs)
{
    for (uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x; c < ncols; c += (uint64_t)gridDim.x * 256u) {
        const uint64_t base = c % X + (c / X) * outer;
        Env<DistWord> eo, ei;
        env_init(eo, stk + c, ncols);
        env_init(ei, stk + (uint64_t)n * ncols + c, ncols);
        uint32_t v = buf[base];
        for (uint32_t u = 0; u < n; ++u) {
            const uint64_t i = base + (uint64_t)u * stride;
            const uint32_t vn = u + 1u < n ? buf[i + stride] : 0u;  // the next step's load, issued ahead
            if (MODE == kSigned) {
                const uint32_t b = mask_bit(words, i);
                env_add(eo, u, b ? 0u : v, n);
                env_add(ei, u, b ? v : 0u, n);
            } else {
                env_add(eo, u, v, n);
            }
            v = vn;
        }
        for (uint32_t u = n; u-- > 0;) {
            const uint64_t i = base + (uint64_t)u * stride;
            uint32_t r;
            uint32_t b = 0u;
            if (MODE == kSigned) {
                b = mask_bit(words, i);
                const uint32_t ro = env_take(eo, u), ri = env_take(ei, u);
                r = b ? ri : ro;
            } else {
                r = env_take(eo, u);
            }
            if (TO_F32) {
                // s = vs * sqrtf((float)D) off M, -(vs * sqrtf((float)D)) on M; the sentinel gives +-inf
                const float f = r == kInf ? __builtin_inff() : vs * sqrtf((float)r);
                reinterpret_cast<float*>(buf)[i] = b ? -f : f;
            } else {
                buf[i] = r;
            }
        }
    }
}

// y pass (ZPASS false): buf holds x' (or kNone) and leaves as x' | y' << 16.  z pass: buf leaves as the cell index x' + X (y' + Y z') of
// the nearest target; GATHER: as values[that index] instead, `fill` for kNone (values is not buf: every thread reads and writes its own
// column of buf only, after phase 1 has read all of it).  With the x pass keeping the left target and the envelope the smaller s, the
// index is the smallest among the nearest targets.
template <bool ZPASS, bool GATHER>
__global__ __launch_bounds__(256) void k_near_col(uint32_t* __restrict__ buf, uint2* __restrict__ stk, uint32_t X, uint32_t Y, uint64_t ncols,
                                                  uint64_t outer, uint64_t stride, uint32_t n, const uint32_t* __restrict__ values, uint32_t fill)
{
    for (uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x; c < ncols; c += (uint64_t)gridDim.x * 256u) {
        const uint64_t base = c % X + (c / X) * outer;
        Env<FeatureWord<ZPASS>> e;  // (y pass: y is the column's z, and unused)
        env_init(e, stk + c, ncols, FeatureWord<ZPASS>{(uint32_t)(c % X), (uint32_t)(c / X), X, Y});
        uint32_t v = buf[base];
        for (uint32_t u = 0; u < n; ++u) {
            const uint64_t i = base + (uint64_t)u * stride;
            const uint32_t vn = u + 1u < n ? buf[i + stride] : 0u;  // the next step's load, issued ahead
            env_add(e, u, v, n);
            v = vn;
        }
        for (uint32_t u = n; u-- > 0;) {
            uint32_t r = env_take(e, u);
            if (GATHER) r = r == kNone ? fill : values[r];
            buf[base + (uint64_t)u * stride] = r;
        }
    }
}

// ---- the three launches of a transform ---------------------------------------------------------------------------------------------------
struct Passes {
    uint32_t X, Y, Z;
    uint64_t rows, xy, xz;  // rows of the x pass, columns of the z pass, columns of the y pass
    unsigned gx, gy, gz;
    bool v4;  // the x pass may store 16 bytes at a time: rows start on 16-byte boundaries
    Passes(const uint32_t dim[3], const uint32_t* buf)
        : X(dim[0]), Y(dim[1]), Z(dim[2]), rows((uint64_t)Y * Z), xy((uint64_t)X * Y), xz((uint64_t)X * Z), gx(blocks_for(rows, kDistBlocks)),
          gy(blocks_for(xz, kDistBlocks)), gz(blocks_for(xy, kDistBlocks)), v4(X % 4u == 0u && ((uintptr_t)buf & 15u) == 0u)
    {
    }
};

template <int MODE>
void distance_passes(const uint32_t* words, const uint32_t dim[3], float vs, uint32_t* buf, uint2* stk, hipStream_t s)
{
    const Passes p(dim, buf);
    if (p.v4) VX_KL((k_dist_x<MODE, true>), dim3(p.gx), dim3(256), 0, s, words, buf, p.X, p.rows);
    else VX_KL((k_dist_x<MODE, false>), dim3(p.gx), dim3(256), 0, s, words, buf, p.X, p.rows);
    VX_KL((k_dist_col<MODE, false>), dim3(p.gy), dim3(256), 0, s, words, buf, stk, p.X, p.xz, p.xy, (uint64_t)p.X, p.Y, vs);
    VX_KL((k_dist_col<MODE, MODE == kSigned>), dim3(p.gz), dim3(256), 0, s, words, buf, stk, p.X, p.xy, (uint64_t)p.X, p.xy, p.Z, vs);
}

template <bool OCC>
void nearest_passes(const uint32_t* words, const uint32_t dim[3], const uint32_t* values, uint32_t fill, uint32_t* buf, uint2* stk, hipStream_t s)
{
    const Passes p(dim, buf);
    if (p.v4) VX_KL((k_near_x<OCC, true>), dim3(p.gx), dim3(256), 0, s, words, buf, p.X, p.rows);
    else VX_KL((k_near_x<OCC, false>), dim3(p.gx), dim3(256), 0, s, words, buf, p.X, p.rows);
    VX_KL((k_near_col<false, false>), dim3(p.gy), dim3(256), 0, s, buf, stk, p.X, p.Y, p.xz, p.xy, (uint64_t)p.X, p.Y, values, fill);
    if (values) VX_KL((k_near_col<true, true>), dim3(p.gz), dim3(256), 0, s, buf, stk, p.X, p.Y, p.xy, (uint64_t)p.X, p.xy, p.Z, values, fill);
    else VX_KL((k_near_col<true, false>), dim3(p.gz), dim3(256), 0, s, buf, stk, p.X, p.Y, p.xy, (uint64_t)p.X, p.xy, p.Z, values, fill);
}

}  // namespace

void launch_nearest(const uint32_t* words, const uint32_t dim[3], bool inside, const uint32_t* values, uint32_t fill, uint32_t* buf, uint2* stk,
                    hipStream_t s)
{
    if (inside) nearest_passes<false>(words, dim, values, fill, buf, stk, s);
    else nearest_passes<true>(words, dim, values, fill, buf, stk, s);
}

uint64_t distance_stack_entries(const uint32_t dim[3], bool is_signed)
{
    const uint64_t n = (uint64_t)dim[0] * dim[1] * dim[2];
    return is_signed ? 2 * n : n;
}

void launch_distance(const uint32_t* words, const uint32_t dim[3], int mode, float vs, uint32_t* buf, uint2* stk, hipStream_t s)
{
    switch (mode) {
    case kOut: distance_passes<kOut>(words, dim, vs, buf, stk, s); break;
    case kIn: distance_passes<kIn>(words, dim, vs, buf, stk, s); break;
    default: distance_passes<kSigned>(words, dim, vs, buf, stk, s); break;
    }
}

}  // namespace vx
