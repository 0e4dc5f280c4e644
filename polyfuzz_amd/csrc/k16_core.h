// K16's candidate pairs as sortable keys (k16_pairs_join.hip): one 64-bit key per cell of the candidate table, the rule that makes
// a pair listed twice count once, and the row pointers over the sorted keys.  Plain integer C++, compiled for the device and for a
// host program that holds it to a set-based model on the CPU (tests/k16_core_host.cpp).
//
//   two lists   cell (row i, to-index j)  ->  i << 32 | j
//   self-join   cell (row i, index j)     ->  min(i, j) << 32 | max(i, j): the two directions of an unordered pair get ONE key, and
//               the lower position is the key's row -- the from-string of the pair's score
//   no pair     j outside [0, n_to), or a row's own index in a self-join  ->  all ones, which sorts behind every real key (a real
//               key's row is below 2^31)
// Sorted ascending, equal keys are adjacent -- a cell listed twice in its row, or the two directions of a self-join pair -- so "this
// key differs from its predecessor" picks each distinct pair once, in (row, to-index) order: CSR order.
#pragma once

#include "k11_core.h"

#include <stdint.h>

#if defined(__HIPCC__)
#define K16_HD __host__ __device__ inline
#else
#define K16_HD inline
#endif

namespace pfz {

constexpr uint64_t kPairKeyNone = ~0ull;

K16_HD uint64_t pair_key(int64_t row, int32_t j, int64_t n_to, bool self)
{
    if (j < 0 || (int64_t)j >= n_to || (self && (int64_t)j == row)) return kPairKeyNone;
    const uint32_t a = (uint32_t)row, b = (uint32_t)j;
    return self && b < a ? (uint64_t)b << 32 | a : (uint64_t)a << 32 | b;
}

K16_HD int32_t pair_key_to(uint64_t key) { return (int32_t)(uint32_t)key; }

// the row a sorted key belongs to; the keys that are no pair belong to "row n_rows", behind the last
K16_HD int64_t pair_key_row(uint64_t key, int64_t n_rows) { return key == kPairKeyNone ? n_rows : (int64_t)(key >> 32); }

// is sorted key p the first of its pair?  (the first key of a row has a predecessor of another row, or none)
K16_HD bool pair_key_first(const uint64_t *keys, int64_t p) { return p == 0 || keys[p - 1] != keys[p]; }

// Position p's share of the row pointers over n sorted keys (k11_core.h rows_fill): seg[r] = the first position whose row is >= r.
// Every seg[0 .. n_rows] is written exactly once over p = 0 .. n - 1 (n >= 1); seg[n_rows] = the number of keys that are a pair.
K16_HD void pair_rows_fill(const uint64_t *keys, int64_t p, int64_t n, int64_t n_rows, int32_t *seg)
{
    rows_fill(p > 0 ? pair_key_row(keys[p - 1], n_rows) : -1, pair_key_row(keys[p], n_rows), p, n, n_rows, seg);
}

}  // namespace pfz
