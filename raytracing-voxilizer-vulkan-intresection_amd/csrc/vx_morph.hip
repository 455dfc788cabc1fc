// vx_morph.hip -- binary morphology of the bitmask with the digital Euclidean ball B(r2) = {b : bx^2 + by^2 + bz^2 <= r2} (vx_grid_morph*,
// vx_grid_seal).  Integer bit operations only: bit-exact by construction.
//
//   k_morph_ball    the bit-level dilation, 32 cells a word.  The ball decomposes by rows,
//                       delta(M)(y, z) = OR over (dy, dz), dy^2 + dz^2 <= r2, of xdil(M(y + dy, z + dz), h(dy, dz)),  h = isqrt(r2 - dy^2 - dz^2),
//                   xdil(row, h) = OR of the row shifted by -h..+h; shifts distribute over OR, so with A_h = the OR of the rows whose
//                   h(dy, dz) >= h (A_R, then one ring of (dy, dz) more per step down)
//                       delta(M)(y, z) = OR over h = R..0 of (A_h << h | A_h >> h):
//                   one pass over the ~pi R^2 rows of the disc and 2 R + 1 funnel shifts, whatever the row lengths.  A workgroup owns a
//                   tile of TY x TZ rows for a run of TXW words; it stages the source rows with a halo of R rows and one word into LDS
//                   once, every lane then gathers its output word from LDS.  The source is read through a 64-bit window (rows start at any
//                   bit; a row-aligned source is the same thing with another row stride), cells outside the source domain are empty.  The
//                   output is ROW-ALIGNED: W = ceil(X / 32) words per (y, z) row, padding bits zero.  Input and output domains differ: input
//                   cell = output cell + shift on every axis (negative: the output is a padded domain; positive: a crop).
//                   Erosion is the same kernel on the complement: kMorphInvIn complements the source over the whole lattice (so every cell
//                   outside the source domain is a target: the box rule, with no reads), kMorphInvOut complements the result.
//                   r2 = 0 is a bit copy with an offset: the pad and the crop.
//   k_morph_pack    row-aligned -> the reference's bitmask (x + X (y + Y z), rows at any bit), optionally OR-ed with another bitmask
//   k_morph_thresh  the distance-field path: cell i is linear in the field, so a wave64 ballot of D[i] <= r2 (erosion: D[i] > r2 and the
//                   box rule) yields two mask words; the tail bits of the last word stay clear
#include "vx_internal.h"
#include "vx_mask.h"

#pragma clang fp contract(off)

namespace vx {

namespace {

constexpr unsigned kMorphBlocks = 1u << 16;
constexpr uint32_t kMorphLdsBytes = 65536u - 2304u;  // per workgroup, beside the static disc table

// up to 32 cells of a row starting at bit `bitpos` of `w` (n = 1..32 of them, the rest of the result is zero); the second word of the
// window is read only when the cells reach into it
__device__ __forceinline__ uint32_t bit_window(const uint32_t* __restrict__ w, uint64_t bitpos, uint32_t n)
{
    const uint32_t sh = (uint32_t)(bitpos & 31u);
    uint64_t two = w[bitpos >> 5];
    if (sh + n > 32u) two |= (uint64_t)w[(bitpos >> 5) + 1] << 32;
    const uint32_t v = (uint32_t)(two >> sh);
    return n >= 32u ? v : v & ((1u << n) - 1u);
}

// cells xs .. xs + 31 of source row (y, z), bit i = cell xs + i; cells outside the domain read as 0
__device__ __forceinline__ uint32_t src_bits(const uint32_t* __restrict__ w, const MorphDom& d, int64_t xs, int64_t y, int64_t z)
{
    if (y < 0 || z < 0 || y >= (int64_t)d.dim[1] || z >= (int64_t)d.dim[2]) return 0u;
    const int64_t lo = xs < 0 ? 0 : xs;
    const int64_t hi = xs + 32 < (int64_t)d.dim[0] ? xs + 32 : (int64_t)d.dim[0];
    if (lo >= hi) return 0u;
    const uint64_t rowbit = ((uint64_t)z * d.dim[1] + (uint64_t)y) * d.stride;
    return bit_window(w, rowbit + (uint64_t)lo, (uint32_t)(hi - lo)) << (uint32_t)(lo - xs);
}

__global__ __launch_bounds__(256) void k_morph_ball(const uint32_t* __restrict__ src, MorphDom in, uint32_t* __restrict__ dst, MorphDom out, int32_t shift,
                                                    uint32_t r2, uint32_t R, uint32_t flags, uint32_t TXW, uint32_t TY, uint32_t TZ, uint64_t ntx, uint64_t nty,
                                                    uint64_t ntiles)
{
    extern __shared__ uint32_t rows[];    // [TZ + 2R][TY + 2R][TXW + 2] source words
    __shared__ short disc[33 * 33];       // disc[h * (R + 1) + |dz|] = isqrt(r2 - h^2 - dz^2), -1 when negative: the |dy| reach of A_h at dz
    const uint32_t tid = threadIdx.x, R1 = R + 1u;
    for (uint32_t i = tid; i < R1 * R1; i += 256u) {
        const int64_t h = i / R1, dz = i % R1, rem = (int64_t)r2 - h * h - dz * dz;
        int s = -1;
        if (rem >= 0) {
            s = (int)sqrtf((float)rem);
            while ((int64_t)s * s > rem) --s;
            while ((int64_t)(s + 1) * (s + 1) <= rem) ++s;
        }
        disc[i] = (short)s;
    }
    const uint32_t PX = TXW + 2u, PY = TY + 2u * R, PZ = TZ + 2u * R;
    const uint32_t Wo = (uint32_t)(out.stride >> 5);
    const bool inv_in = flags & kMorphInvIn, inv_out = flags & kMorphInvOut;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t xw0 = (t % ntx) * TXW, y0 = (t / ntx % nty) * TY, z0 = (t / (ntx * nty)) * TZ;
        __syncthreads();  // the tile before has been gathered (first tile: the disc table is complete)
        for (uint32_t i = tid; i < PX * PY * PZ; i += 256u) {
            const uint32_t lx = i % PX, ly = i / PX % PY, lz = i / (PX * PY);
            const uint32_t v = src_bits(src, in, 32 * ((int64_t)xw0 + lx - 1) + shift, (int64_t)y0 + ly - R + shift, (int64_t)z0 + lz - R + shift);
            rows[i] = inv_in ? ~v : v;
        }
        __syncthreads();
        for (uint32_t o = tid; o < TXW * TY * TZ; o += 256u) {
            const uint32_t ox = o % TXW, oy = o / TXW % TY, oz = o / (TXW * TY);
            const uint64_t xw = xw0 + ox, y = y0 + oy, z = z0 + oz;
            if (xw >= Wo || y >= out.dim[1] || z >= out.dim[2]) continue;
            const int base = (int)(((oz + R) * PY + (oy + R)) * PX + ox + 1u);
            uint32_t al = 0u, ac = 0u, ar = 0u, res = 0u;  // A_h: the words left of, at and right of the output word
            for (int h = (int)R; h >= 0; --h) {
                const short* th = disc + h * (int)R1;
                for (int dz = -(int)R; dz <= (int)R; ++dz) {
                    const int adz = dz < 0 ? -dz : dz;
                    const int a1 = th[adz];
                    if (a1 < 0) continue;
                    const int a0 = h < (int)R ? th[(int)R1 + adz] : -1;  // |dy| <= a0 joined at a larger h
                    for (int dy = a0 + 1; dy <= a1; ++dy) {
                        const int p = base + (dz * (int)PY + dy) * (int)PX;
                        al |= rows[p - 1]; ac |= rows[p]; ar |= rows[p + 1];
                        if (dy) {
                            const int q = base + (dz * (int)PY - dy) * (int)PX;
                            al |= rows[q - 1]; ac |= rows[q]; ar |= rows[q + 1];
                        }
                    }
                }
                if (h == 0) res |= ac;
                else if (h < 32) res |= (ac << h) | (al >> (32 - h)) | (ac >> h) | (ar << (32 - h));
                else res |= al | ar;
            }
            if (inv_out) res = ~res;
            const uint64_t left = (uint64_t)out.dim[0] - 32ull * xw;  // cells of the row from this word on: padding bits stay zero
            if (left < 32u) res &= (1u << left) - 1u;
            dst[(z * out.dim[1] + y) * Wo + xw] = res;
        }
    }
}

__global__ __launch_bounds__(256) void k_morph_pack(const uint32_t* __restrict__ src, uint64_t stride, uint32_t X, uint64_t nvox, uint64_t nwords,
                                                    const uint32_t* __restrict__ orw, uint32_t* __restrict__ dst)
{
    for (uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x; w < nwords; w += (uint64_t)gridDim.x * 256u) {
        uint64_t i = 32ull * w;
        const uint64_t end = i + 32u < nvox ? i + 32u : nvox;
        uint32_t acc = orw ? orw[w] : 0u;
        while (i < end) {
            const uint64_t row = i / X;
            const uint32_t x = (uint32_t)(i - row * X);
            const uint32_t n = (uint32_t)((uint64_t)(X - x) < end - i ? (uint64_t)(X - x) : end - i);
            acc |= bit_window(src, row * stride + x, n) << (uint32_t)(i - 32ull * w);
            i += n;
        }
        dst[w] = acc;
    }
}

template <bool ERODE>
__global__ __launch_bounds__(256) void k_morph_thresh(const uint32_t* __restrict__ field, uint32_t X, uint32_t Y, uint32_t Z, uint64_t nvox, uint32_t r2, uint32_t R,
                                                      uint32_t* __restrict__ dst)
{
    const uint64_t span = ((nvox + 255u) / 256u) * 256u;  // whole workgroups: every lane of a wave reaches the ballot
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < span; i += (uint64_t)gridDim.x * 256u) {
        bool in = false;
        if (i < nvox) {
            const uint32_t d = field[i];
            if (ERODE) {
                const uint64_t r = i / X;
                const uint32_t x = (uint32_t)(i - r * X), y = (uint32_t)(r % Y), z = (uint32_t)(r / Y);
                // the ball reaches R cells along every axis: a cell nearer than R to the border meets an outside (empty) cell
                in = d > r2 && x >= R && (uint64_t)x + R < X && y >= R && (uint64_t)y + R < Y && z >= R && (uint64_t)z + R < Z;
            } else {
                in = d <= r2;
            }
        }
        const unsigned long long b = __ballot(in);
        const uint32_t lane = threadIdx.x & 63u;
        const uint64_t w = (i >> 5);
        if ((lane == 0u || lane == 32u) && 32ull * w < nvox) dst[w] = lane ? (uint32_t)(b >> 32) : (uint32_t)b;
    }
}

}  // namespace

void launch_morph_ball(const uint32_t* src, const MorphDom& in, uint32_t* dst, const uint32_t odim[3], int32_t shift, uint32_t r2, uint32_t flags, hipStream_t s)
{
    uint32_t R = 0;
    while ((uint64_t)(R + 1) * (R + 1) <= r2) ++R;  // (callers keep R <= 32: a shift reaches only the neighbouring word)
    MorphDom out;
    for (int a = 0; a < 3; ++a) out.dim[a] = odim[a];
    const uint32_t Wo = (odim[0] + 31u) / 32u;
    out.stride = 32ull * Wo;
    // the tile: 8 words x 16 x 16 rows where the halo leaves room, rows before words
    uint32_t TXW = Wo < 8u ? Wo : 8u, TY = odim[1] < 16u ? odim[1] : 16u, TZ = odim[2] < 16u ? odim[2] : 16u;
    auto lds = [&]() { return (uint64_t)(TXW + 2u) * (TY + 2u * R) * (TZ + 2u * R) * 4u; };
    while (lds() > kMorphLdsBytes) {
        if (TY > 8u && TY >= TZ) TY = (TY + 1u) / 2u;
        else if (TZ > 8u) TZ = (TZ + 1u) / 2u;
        else if (TXW > 1u) TXW = (TXW + 1u) / 2u;
        else if (TY > 1u && TY >= TZ) TY = (TY + 1u) / 2u;
        else if (TZ > 1u) TZ = (TZ + 1u) / 2u;
        else break;  // (R = 32 fits with 8 x 8 rows of one word)
    }
    const uint64_t ntx = (Wo + TXW - 1u) / TXW, nty = (odim[1] + TY - 1u) / TY, ntz = (odim[2] + TZ - 1u) / TZ, ntiles = ntx * nty * ntz;
    if (!ntiles) return;
    const unsigned grid = (unsigned)(ntiles < kMorphBlocks ? ntiles : kMorphBlocks);
    VX_KL(k_morph_ball, dim3(grid), dim3(256), (size_t)lds(), s, src, in, dst, out, shift, r2, R, flags, TXW, TY, TZ, ntx, nty, ntiles);
}

uint64_t morph_aligned_words(const uint32_t dim[3]) { return (uint64_t)((dim[0] + 31u) / 32u) * dim[1] * dim[2]; }

void launch_morph_pack(const uint32_t* aligned, const uint32_t dim[3], const uint32_t* orw, uint32_t* dst, hipStream_t s)
{
    const uint64_t nvox = (uint64_t)dim[0] * dim[1] * dim[2], nwords = (nvox + 31u) / 32u;
    if (!nwords) return;
    VX_KL(k_morph_pack, dim3(blocks_for(nwords, kMorphBlocks)), dim3(256), 0, s, aligned, 32ull * ((dim[0] + 31u) / 32u), dim[0], nvox, nwords, orw, dst);
}

void launch_morph_thresh(const uint32_t* field, const uint32_t dim[3], uint32_t r2, bool erode, uint32_t* dst, hipStream_t s)
{
    const uint64_t nvox = (uint64_t)dim[0] * dim[1] * dim[2];
    if (!nvox) return;
    uint32_t R = 0;
    while ((uint64_t)(R + 1) * (R + 1) <= r2) ++R;
    if (erode) VX_KL((k_morph_thresh<true>), dim3(blocks_for(nvox, kMorphBlocks)), dim3(256), 0, s, field, dim[0], dim[1], dim[2], nvox, r2, R, dst);
    else VX_KL((k_morph_thresh<false>), dim3(blocks_for(nvox, kMorphBlocks)), dim3(256), 0, s, field, dim[0], dim[1], dim[2], nvox, r2, R, dst);
}

}  // namespace vx
