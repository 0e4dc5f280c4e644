// K24's rule (k24_hamming_index.hip): the block index behind "every pair of d-bit codes that differ in at most hmax bits".  Cut the d
// bits into m = hmax + 1 blocks; two codes within hmax cannot differ in every block (pigeonhole), so they agree completely on at
// least one.  Only codes with the same bits in some block need their distance computed, and the filter is exact.
//
//   blocks      block b covers the row's bits [b d / m, (b + 1) d / m) (floors), bit k of a row being bit 7 - k % 8 of byte k / 8
//               (np.packbits order).  Widths differ by at most one.
//   indexable   1 <= m <= min(d, 256) for a width d in [1, 2^24); the call adds its own limits on the rows (k24_rows_indexable).
//   block key   the first min(width, 32) bits of the block as an unsigned integer, first bit most significant.  Agreement on a block
//               implies agreement on its key, so "same key in some block" is necessary for h <= hmax whatever the width.
//   candidate   (from i, to j) in block b iff the two keys of block b are equal; in a self-join only j > i.
//   hit         a candidate in block b whose full distance is <= hmax and whose keys differ in every block b' < b: each pair is
//               reported once, in the first block it agrees on, without a de-duplication pass.
//   sort key    block << 56 | key << 24 | position: 8 + 32 + 24 bits, where the limits come from.
//
// Plain integer C++, compiled for the device and for a host program that holds it to a numpy restatement (tests/k24_core_host.cpp).
// The cut of a probe's run of partners into work items is K17's: pair_item_count / pair_item_slice of k17_core.h.
#pragma once

#include <stdint.h>

#include "k17_core.h"

namespace pfz {

constexpr int32_t kK24MaxBlocks = 256;
constexpr int64_t kK24MaxRows = (int64_t)1 << 24;      // positions have 24 bits in a sort key
// The cost of one indexed check in tile pairs, rounded up to a power of two: PFZ_HAMMING_INDEX_AUTO runs the index iff
// checks * kK24AutoRatio <= all pairs.  Measured (docs/HAMMING_INDEX_MEASURED.md): the largest ratio of (index time / checks) to
// (K23 time / all pairs) over the sweep's points where the index call was not faster than K23's is 34.7.
constexpr int64_t kK24AutoRatio = 64;

// (d, hmax) has a block index
K16_HD bool k24_indexable(int64_t d, int64_t hmax)
{
    if (d < 1 || d >= ((int64_t)1 << 24) || hmax < 0) return false;
    const int64_t m = hmax + 1;
    return m <= d && m <= kK24MaxBlocks;
}

// ... and two lists of n_from and n_to rows fit its sort keys and the 32-bit positions of the sorted keys and of the probes
K16_HD bool k24_rows_indexable(int64_t n_from, int64_t n_to, int64_t m)
{
    return n_from < kK24MaxRows && n_to < kK24MaxRows && m * n_to < ((int64_t)1 << 31) && m * n_from < ((int64_t)1 << 31);
}

// the first bit of block b (b == m: d)
K16_HD int32_t k24_block_lo(int64_t d, int64_t m, int64_t b) { return (int32_t)(b * d / m); }

// the narrowest and the widest block: d / m and its ceiling
K16_HD int32_t k24_block_min(int64_t d, int64_t m) { return (int32_t)(d / m); }
K16_HD int32_t k24_block_max(int64_t d, int64_t m) { return (int32_t)((d + m - 1) / m); }

// the key of the block [lo, hi) of a packed row: only the bytes that hold one of its first min(hi - lo, 32) bits are read
K16_HD uint32_t k24_block_key(const uint8_t *row, int32_t lo, int32_t hi)
{
    const int32_t nb = hi - lo < 32 ? hi - lo : 32;
    if (nb <= 0) return 0;
    const int32_t first = lo >> 3, last = (lo + nb - 1) >> 3;      // at most five bytes
    uint64_t v = 0;
    for (int32_t k = first; k <= last; ++k) v = v << 8 | row[k];
    const int32_t have = 8 * (last - first + 1), skip = lo & 7;
    v >>= have - skip - nb;
    return (uint32_t)(v & (((uint64_t)1 << nb) - 1));
}

K16_HD uint64_t k24_sort_key(int32_t block, uint32_t key, int32_t pos) { return (uint64_t)block << 56 | (uint64_t)key << 24 | (uint32_t)pos; }
K16_HD int32_t k24_sort_key_block(uint64_t s) { return (int32_t)(s >> 56); }
K16_HD int32_t k24_sort_key_pos(uint64_t s) { return (int32_t)(s & 0xffffff); }

// the first-block rule: a pair that agrees on block b is reported there iff its key rows differ in every block before b
K16_HD bool k24_first_block(const uint32_t *ka, const uint32_t *kb, int32_t b)
{
    for (int32_t q = 0; q < b; ++q)
        if (ka[q] == kb[q]) return false;
    return true;
}

// the first position in the ascending keys[p0, p1) that is >= x (p1: none)
K16_HD int64_t k24_lower_bound(const uint64_t *keys, int64_t p0, int64_t p1, uint64_t x)
{
    while (p0 < p1) {
        const int64_t mid = p0 + (p1 - p0) / 2;
        if (keys[mid] < x) p0 = mid + 1;
        else p1 = mid;
    }
    return p0;
}

// The run of partners of the probe (from-row i, block b, key) in the sorted keys of n_to rows and m blocks: block b's keys are
// the positions [b n_to, (b + 1) n_to), ordered by key, then position.  Two lists: every to-row with the key; self: those behind i.
K16_HD void k24_probe_run(const uint64_t *skeys, int64_t n_to, int32_t b, uint32_t key, int32_t i, bool self, int64_t *p0, int64_t *p1)
{
    const int64_t s0 = (int64_t)b * n_to, s1 = s0 + n_to;
    *p0 = k24_lower_bound(skeys, s0, s1, k24_sort_key(b, key, self ? i + 1 : 0));
    *p1 = k24_lower_bound(skeys, *p0, s1, k24_sort_key(b, key, 0xffffff));      // (no to-row has position 2^24 - 1)
}

}  // namespace pfz
