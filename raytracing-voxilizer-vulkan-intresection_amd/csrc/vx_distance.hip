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
// The feature transform (vx_grid_nearest*: the INDEX of the nearest target, smallest index on ties) runs the same passes with kernels of its
// own, k_near_x and k_near_col, below the distance kernels.
#include "vx_internal.h"

#pragma clang fp contract(off)

namespace vx {

namespace {

constexpr uint32_t kInf = 0xFFFFFFFFu;  // no target in reach (the contract's sentinel)
constexpr uint32_t kNone = 0xFFFFFFFFu; // no target position
constexpr unsigned kDistBlocks = 256 * 8;

inline unsigned dist_grid(uint64_t n)
{
    uint64_t b = (n + 255) / 256;
    if (b < 1) b = 1;
    if (b > kDistBlocks) b = kDistBlocks;
    return (unsigned)b;
}

enum : int { kOut = 0, kIn = 1, kSigned = 2 };

// word w of the row whose first cell is bit `rowbit` of the mask: cells x = 32 w .. 32 w + 31, `valid` marks those with x < X (the mask has
// two spare words past nwords, so the second word of the window always exists)
__device__ __forceinline__ uint32_t row_word(const uint32_t* __restrict__ words, uint64_t rowbit, uint32_t X, uint32_t w, uint32_t& valid)
{
    const uint64_t s = rowbit + 32ull * w;
    const uint64_t two = (uint64_t)words[s >> 5] | ((uint64_t)words[(s >> 5) + 1] << 32);
    const uint32_t nb = X - 32u * w < 32u ? X - 32u * w : 32u;
    valid = nb == 32u ? ~0u : ((1u << nb) - 1u);
    return (uint32_t)(two >> (s & 31u));
}

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

template <int MODE, bool VEC4>
__global__ __launch_bounds__(256) void k_dist_x(const uint32_t* __restrict__ words, uint32_t* __restrict__ out, uint32_t X, uint64_t rows)
{
    const uint32_t W = (X + 31u) / 32u;
    for (uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x; r < rows; r += (uint64_t)gridDim.x * 256u) {
        const uint64_t rowbit = r * X;
        uint32_t* o = out + rowbit;
        uint32_t prev_occ = kNone, prev_emp = kNone;  // last target of the words before
        Ahead ao{0u, kNone}, ae{0u, kNone};           // first target of the words after
        if (MODE != kIn) ahead_from<true>(ao, words, rowbit, X, W, 1u);
        if (MODE != kOut) ahead_from<false>(ae, words, rowbit, X, W, 1u);
        for (uint32_t w = 0; w < W; ++w) {
            if (MODE != kIn && ao.lw == w) ahead_from<true>(ao, words, rowbit, X, W, w + 1u);
            if (MODE != kOut && ae.lw == w) ahead_from<false>(ae, words, rowbit, X, W, w + 1u);
            uint32_t valid;
            const uint32_t m = row_word(words, rowbit, X, w, valid);
            const uint32_t to = m & valid, te = ~m & valid;  // padding bits are neither occupied nor empty
            const uint32_t nb = (uint32_t)__builtin_popcount(valid);
            uint32_t v[32];
#pragma unroll
            for (uint32_t i = 0; i < 32u; ++i) {
                const uint32_t x = 32u * w + i;
                if (MODE == kOut) v[i] = row_dist(to, i, x, prev_occ, ao.pos);
                else if (MODE == kIn) v[i] = row_dist(te, i, x, prev_emp, ae.pos);
                else v[i] = (m >> i) & 1u ? row_dist(te, i, x, prev_emp, ae.pos) : row_dist(to, i, x, prev_occ, ao.pos);
            }
            if (VEC4) {  // X % 4 == 0: the row and nb are multiples of four cells
#pragma unroll
                for (uint32_t i = 0; i < 32u; i += 4u)
                    if (i < nb) *reinterpret_cast<uint4*>(o + 32u * w + i) = make_uint4(v[i], v[i + 1], v[i + 2], v[i + 3]);
            } else {
#pragma unroll
                for (uint32_t i = 0; i < 32u; ++i)
                    if (i < nb) o[32u * w + i] = v[i];
            }
            if (to) prev_occ = 32u * w + 31u - (uint32_t)__builtin_clz(to);
            if (te) prev_emp = 32u * w + 31u - (uint32_t)__builtin_clz(te);
        }
    }
}

// One lower envelope of a column (Meijster): entries k = 0..q, parabola s_k with value g_k, winning from t_k on; the top in registers,
// every entry also at stk[k * ld] (s | t << 16, g) -- s, t < 65536.
struct Env {
    uint2* stk;
    uint64_t ld;
    int q;
    uint32_t s, t, g;
};

__device__ __forceinline__ void env_init(Env& e, uint2* stk, uint64_t ld)
{
    e.stk = stk;
    e.ld = ld;
    e.q = -1;
    e.s = e.t = e.g = 0u;
}
__device__ __forceinline__ void env_load(Env& e)
{
    const uint2 v = e.stk[(uint64_t)e.q * e.ld];
    e.s = v.x & 0xFFFFu;
    e.t = v.x >> 16;
    e.g = v.y;
}
__device__ __forceinline__ void env_push(Env& e, uint32_t s, uint32_t t, uint32_t g)
{
    ++e.q;
    e.s = s;
    e.t = t;
    e.g = g;
    e.stk[(uint64_t)e.q * e.ld] = make_uint2(s | (t << 16), g);
}
__device__ __forceinline__ uint64_t para(uint32_t x, uint32_t s, uint32_t g)
{
    const int64_t d = (int64_t)x - (int64_t)s;
    return (uint64_t)(d * d) + g;
}

// phase 1, one cell u of a column of n: the parabolas u now beats at their start are dropped, then u starts where it first beats the top
__device__ __forceinline__ void env_add(Env& e, uint32_t u, uint32_t gu, uint32_t n)
{
    if (gu == kInf) return;  // sentinels are skipped, never pushed
    while (e.q >= 0 && para(e.t, e.s, e.g) > para(e.t, u, gu)) {
        if (--e.q >= 0) env_load(e);
    }
    if (e.q < 0) { env_push(e, u, 0u, gu); return; }
    // Sep(s, u) = floor((u^2 - s^2 + g_u - g_s) / (2 (u - s))); not popped: the crossing lies at or past t >= 0, the numerator is >= 0
    const int64_t num = (int64_t)u * u - (int64_t)e.s * e.s + (int64_t)gu - (int64_t)e.g;
    const int64_t den = 2 * ((int64_t)u - (int64_t)e.s);
    const int64_t w = (num >= 0 ? num / den : -((-num + den - 1) / den)) + 1;
    if (w < (int64_t)n) env_push(e, u, (uint32_t)w, gu);
}

// phase 2, cells u = n-1 down to 0: the envelope's value at u, then the entry that starts at u is dropped
__device__ __forceinline__ uint32_t env_take(Env& e, uint32_t u)
{
    if (e.q < 0) return kInf;
    const uint32_t v = (uint32_t)para(u, e.s, e.g);  // the exact minimum: within the grid's 32-bit limit
    if (u == e.t && --e.q >= 0) env_load(e);
    return v;
}

__device__ __forceinline__ uint32_t mask_bit(const uint32_t* __restrict__ words, uint64_t i) { return (words[i >> 5] >> (i & 31u)) & 1u; }

// Columns c < ncols of n cells: cell j of column c at base(c) + j * stride with base(c) = c % X + (c / X) * outer.
// y pass: ncols = X Z, outer = X Y, stride = X.  z pass: ncols = X Y, outer = X, stride = X Y.
// stk: n * ncols entries per envelope (SIGNED: the in-envelope's follow the out-envelope's).
template <int MODE, bool TO_F32>
__global__ __launch_bounds__(256) void k_dist_col(const uint32_t* __restrict__ words, uint32_t* __restrict__ buf, uint2* __restrict__ stk,
                                                  uint32_t X, uint64_t ncols, uint64_t outer, uint64_t stride, uint32_t n, float vs)
{
    for (uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x; c < ncols; c += (uint64_t)gridDim.x * 256u) {
        const uint64_t base = c % X + (c / X) * outer;
        Env eo, ei;
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

// ---- the feature transform (vx_grid_nearest*): the same three passes, carrying WHICH target wins instead of how far it is ------------------
// The one 32-bit intermediate per cell is the packed feature x' | y' << 16 of the cell's nearest target so far (kNone: none); every g the
// envelope needs is recomputed from it and the column's own position: (x - x')^2 after the x pass, (x - x')^2 + (y - y')^2 after the y pass.
// The stack entry stays 8 bytes, (s | t << 16, feature of s).  Ties: the x pass keeps the left target, the envelope keeps the smaller s
// (a parabola is popped only by a strictly better newcomer, and a newcomer starts where it is strictly better) -- together the smallest
// cell index among the nearest targets.  x' | y' << 16 == kNone would need X = Y = 65536, which the distance fields' limit excludes.

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

template <bool OCC, bool VEC4>
__global__ __launch_bounds__(256) void k_near_x(const uint32_t* __restrict__ words, uint32_t* __restrict__ out, uint32_t X, uint64_t rows)
{
    const uint32_t W = (X + 31u) / 32u;
    for (uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x; r < rows; r += (uint64_t)gridDim.x * 256u) {
        const uint64_t rowbit = r * X;
        uint32_t* o = out + rowbit;
        uint32_t prev = kNone;
        Ahead a{0u, kNone};
        ahead_from<OCC>(a, words, rowbit, X, W, 1u);
        for (uint32_t w = 0; w < W; ++w) {
            if (a.lw == w) ahead_from<OCC>(a, words, rowbit, X, W, w + 1u);
            uint32_t valid;
            const uint32_t m = row_word(words, rowbit, X, w, valid);
            const uint32_t t = (OCC ? m : ~m) & valid;
            const uint32_t nb = (uint32_t)__builtin_popcount(valid);
            uint32_t v[32];
#pragma unroll
            for (uint32_t i = 0; i < 32u; ++i) v[i] = row_near(t, i, 32u * w + i, prev, a.pos);
            if (VEC4) {
#pragma unroll
                for (uint32_t i = 0; i < 32u; i += 4u)
                    if (i < nb) *reinterpret_cast<uint4*>(o + 32u * w + i) = make_uint4(v[i], v[i + 1], v[i + 2], v[i + 3]);
            } else {
#pragma unroll
                for (uint32_t i = 0; i < 32u; ++i)
                    if (i < nb) o[32u * w + i] = v[i];
            }
            if (t) prev = 32u * w + 31u - (uint32_t)__builtin_clz(t);
        }
    }
}

// g of a packed feature seen from the column at (x, y): the squared distance within the axes already passed (y pass: x only, f >> 16 == 0)
template <bool ZPASS>
__device__ __forceinline__ uint32_t near_g(uint32_t f, uint32_t x, uint32_t y)
{
    const uint32_t dx = x - (f & 0xFFFFu);  // (the square of a wrapped difference is the square of the difference: below 2^32)
    uint32_t g = dx * dx;
    if (ZPASS) {
        const uint32_t dy = y - (f >> 16);
        g += dy * dy;
    }
    return g;
}

// Env with the feature of s in the entry's second word; g(s) is kept for the top only, recomputed on every load
struct NearEnv {
    uint2* stk;
    uint64_t ld;
    int q;
    uint32_t s, t, f, g;
};

template <bool ZPASS>
__device__ __forceinline__ void near_load(NearEnv& e, uint32_t x, uint32_t y)
{
    const uint2 v = e.stk[(uint64_t)e.q * e.ld];
    e.s = v.x & 0xFFFFu;
    e.t = v.x >> 16;
    e.f = v.y;
    e.g = near_g<ZPASS>(v.y, x, y);
}
__device__ __forceinline__ void near_push(NearEnv& e, uint32_t s, uint32_t t, uint32_t f, uint32_t g)
{
    ++e.q;
    e.s = s;
    e.t = t;
    e.f = f;
    e.g = g;
    e.stk[(uint64_t)e.q * e.ld] = make_uint2(s | (t << 16), f);
}

// env_add with the feature fu of cell u (kNone: skipped)
template <bool ZPASS>
__device__ __forceinline__ void near_add(NearEnv& e, uint32_t u, uint32_t fu, uint32_t n, uint32_t x, uint32_t y)
{
    if (fu == kNone) return;
    const uint32_t gu = near_g<ZPASS>(fu, x, y);
    while (e.q >= 0 && para(e.t, e.s, e.g) > para(e.t, u, gu)) {
        if (--e.q >= 0) near_load<ZPASS>(e, x, y);
    }
    if (e.q < 0) { near_push(e, u, 0u, fu, gu); return; }
    const int64_t num = (int64_t)u * u - (int64_t)e.s * e.s + (int64_t)gu - (int64_t)e.g;
    const int64_t den = 2 * ((int64_t)u - (int64_t)e.s);
    const int64_t w = (num >= 0 ? num / den : -((-num + den - 1) / den)) + 1;
    if (w < (int64_t)n) near_push(e, u, (uint32_t)w, fu, gu);
}

// Columns as for k_dist_col.  y pass (ZPASS false): buf holds x' (or kNone) and leaves as x' | y' << 16.  z pass: buf leaves as the cell
// index x' + X (y' + Y z') of the nearest target; GATHER: as values[that index] instead, `fill` for kNone (values is not buf: every thread
// reads and writes its own column of buf only, after phase 1 has read all of it).
template <bool ZPASS, bool GATHER>
__global__ __launch_bounds__(256) void k_near_col(uint32_t* __restrict__ buf, uint2* __restrict__ stk, uint32_t X, uint32_t Y, uint64_t ncols,
                                                  uint64_t outer, uint64_t stride, uint32_t n, const uint32_t* __restrict__ values, uint32_t fill)
{
    for (uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x; c < ncols; c += (uint64_t)gridDim.x * 256u) {
        const uint32_t x = (uint32_t)(c % X), y = (uint32_t)(c / X);  // (y pass: y is the column's z, and unused)
        const uint64_t base = x + (c / X) * outer;
        NearEnv e;
        e.stk = stk + c;
        e.ld = ncols;
        e.q = -1;
        e.s = e.t = e.f = e.g = 0u;
        uint32_t v = buf[base];
        for (uint32_t u = 0; u < n; ++u) {
            const uint64_t i = base + (uint64_t)u * stride;
            const uint32_t vn = u + 1u < n ? buf[i + stride] : 0u;  // the next step's load, issued ahead
            near_add<ZPASS>(e, u, v, n, x, y);
            v = vn;
        }
        for (uint32_t u = n; u-- > 0;) {
            const uint64_t i = base + (uint64_t)u * stride;
            uint32_t r = kNone;
            if (e.q >= 0) {
                r = ZPASS ? (e.f & 0xFFFFu) + X * ((e.f >> 16) + Y * e.s) : e.f | (e.s << 16);
                if (u == e.t && --e.q >= 0) near_load<ZPASS>(e, x, y);
            }
            if (GATHER) r = r == kNone ? fill : values[r];
            buf[i] = r;
        }
    }
}

}  // namespace

void launch_nearest(const uint32_t* words, const uint32_t dim[3], bool inside, const uint32_t* values, uint32_t fill, uint32_t* buf, uint2* stk,
                    hipStream_t s)
{
    const uint32_t X = dim[0], Y = dim[1], Z = dim[2];
    const uint64_t rows = (uint64_t)Y * Z, xy = (uint64_t)X * Y, xz = (uint64_t)X * Z;
    const unsigned gx = dist_grid(rows), gy = dist_grid(xz), gz = dist_grid(xy);
    const bool v4 = X % 4u == 0u && ((uintptr_t)buf & 15u) == 0u;
    if (inside) {
        if (v4) VX_KL((k_near_x<false, true>), dim3(gx), dim3(256), 0, s, words, buf, X, rows);
        else VX_KL((k_near_x<false, false>), dim3(gx), dim3(256), 0, s, words, buf, X, rows);
    } else {
        if (v4) VX_KL((k_near_x<true, true>), dim3(gx), dim3(256), 0, s, words, buf, X, rows);
        else VX_KL((k_near_x<true, false>), dim3(gx), dim3(256), 0, s, words, buf, X, rows);
    }
    VX_KL((k_near_col<false, false>), dim3(gy), dim3(256), 0, s, buf, stk, X, Y, xz, xy, (uint64_t)X, Y, values, fill);
    if (values) VX_KL((k_near_col<true, true>), dim3(gz), dim3(256), 0, s, buf, stk, X, Y, xy, (uint64_t)X, xy, Z, values, fill);
    else VX_KL((k_near_col<true, false>), dim3(gz), dim3(256), 0, s, buf, stk, X, Y, xy, (uint64_t)X, xy, Z, values, fill);
}

uint64_t distance_stack_entries(const uint32_t dim[3], bool is_signed)
{
    const uint64_t n = (uint64_t)dim[0] * dim[1] * dim[2];
    return is_signed ? 2 * n : n;
}

void launch_distance(const uint32_t* words, const uint32_t dim[3], int mode, float vs, uint32_t* buf, uint2* stk, hipStream_t s)
{
    const uint32_t X = dim[0], Y = dim[1], Z = dim[2];
    const uint64_t rows = (uint64_t)Y * Z, xy = (uint64_t)X * Y, xz = (uint64_t)X * Z;
    const unsigned gx = dist_grid(rows), gy = dist_grid(xz), gz = dist_grid(xy);
    const bool v4 = X % 4u == 0u && ((uintptr_t)buf & 15u) == 0u;  // (rows start on 16-byte boundaries)
    switch (mode) {
    case kOut:
        if (v4) VX_KL((k_dist_x<kOut, true>), dim3(gx), dim3(256), 0, s, words, buf, X, rows);
        else VX_KL((k_dist_x<kOut, false>), dim3(gx), dim3(256), 0, s, words, buf, X, rows);
        VX_KL((k_dist_col<kOut, false>), dim3(gy), dim3(256), 0, s, words, buf, stk, X, xz, xy, (uint64_t)X, Y, vs);
        VX_KL((k_dist_col<kOut, false>), dim3(gz), dim3(256), 0, s, words, buf, stk, X, xy, (uint64_t)X, xy, Z, vs);
        break;
    case kIn:
        if (v4) VX_KL((k_dist_x<kIn, true>), dim3(gx), dim3(256), 0, s, words, buf, X, rows);
        else VX_KL((k_dist_x<kIn, false>), dim3(gx), dim3(256), 0, s, words, buf, X, rows);
        VX_KL((k_dist_col<kIn, false>), dim3(gy), dim3(256), 0, s, words, buf, stk, X, xz, xy, (uint64_t)X, Y, vs);
        VX_KL((k_dist_col<kIn, false>), dim3(gz), dim3(256), 0, s, words, buf, stk, X, xy, (uint64_t)X, xy, Z, vs);
        break;
    default:
        if (v4) VX_KL((k_dist_x<kSigned, true>), dim3(gx), dim3(256), 0, s, words, buf, X, rows);
        else VX_KL((k_dist_x<kSigned, false>), dim3(gx), dim3(256), 0, s, words, buf, X, rows);
        VX_KL((k_dist_col<kSigned, false>), dim3(gy), dim3(256), 0, s, words, buf, stk, X, xz, xy, (uint64_t)X, Y, vs);
        VX_KL((k_dist_col<kSigned, true>), dim3(gz), dim3(256), 0, s, words, buf, stk, X, xy, (uint64_t)X, xy, Z, vs);
        break;
    }
}

}  // namespace vx
