// vx_mask.h -- what the grid-analysis files (vx_solid.hip, vx_distance.hip, vx_morph.hip, vx_surface.hip, vx_components.hip) share: the
// launch clamp of their grid-stride kernels and the two readers of the reference's bitmask, cell i at bit i & 31 of word i >> 5 and rows
// starting at any bit (X % 32 != 0).  Three readers stay with their files on purpose: bit_window (vx_morph.hip) reads its second word only
// when the cells reach into it -- its sources are scratch masks without spare words; window (vx_surface.hip) reads words out of range as
// empty; vx_multihit.hip keeps its own text.
#pragma once
#include "vx_internal.h"

namespace vx {

// blocks of 256 threads for n items, at least one and at most `cap`: the kernels stride over the rest
inline unsigned blocks_for(uint64_t n, unsigned cap)
{
    uint64_t b = (n + 255) / 256;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (unsigned)b;
}

__device__ __forceinline__ uint32_t mask_bit(const uint32_t* __restrict__ words, uint64_t i) { return (words[i >> 5] >> (i & 31u)) & 1u; }

// Word w of the row of X cells whose first cell is bit `rowbit` of the mask: cells x = 32 w .. 32 w + 31, 32 w < X; `valid` marks those with
// x < X, the bits returned outside it are not the row's.  Both words of the 64-bit window are read whatever s & 31 is: `words` must be a
// grid's mask, which has two spare words past nwords.
__device__ __forceinline__ uint32_t row_word(const uint32_t* __restrict__ words, uint64_t rowbit, uint32_t X, uint32_t w, uint32_t& valid)
{
    const uint64_t s = rowbit + 32ull * w;
    const uint64_t two = (uint64_t)words[s >> 5] | ((uint64_t)words[(s >> 5) + 1] << 32);
    const uint32_t nb = X - 32u * w < 32u ? X - 32u * w : 32u;
    valid = nb == 32u ? ~0u : ((1u << nb) - 1u);
    return (uint32_t)(two >> (s & 31u));
}

}  // namespace vx
