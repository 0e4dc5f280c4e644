// K17's work items (k16_pairs_join.hip, the key entries): the arithmetic that cuts a from-row's range of sorted pair keys into slices
// of at most S partners.  Plain integer C++, compiled for the device and for a host program that holds it to a numpy restatement
// (tests/k17_core_host.cpp).
//
// Behind a threshold join (K15) a row's range has no bound: the fullest row of the 100 000 company names has 1 860 partners at
// cosine 0.8 where the mean row has a handful.  One wave per row would leave that wave 29 chunks of 64 lanes behind the others, so
// the key entries deal (row, slice) ITEMS instead: row r with the range [p0, p1) gives pair_item_count(p1 - p0, S) items, the k-th
// of them [p0 + k S, min(p0 + (k + 1) S, p1)).  An empty row gives none.  S <= 0 stands for "whole rows": one item per row that
// has a pair (what-if builds only, see kPairSlice).
#pragma once

#include <stdint.h>

#include "k16_core.h"

// what-if builds only (tools/build_variant.sh -DPFZ_PAIR_SLICE=n, 0: whole rows): the slice's worth in time; results are the same
#ifndef PFZ_PAIR_SLICE
#define PFZ_PAIR_SLICE 64
#endif

namespace pfz {

constexpr int32_t kPairSlice = PFZ_PAIR_SLICE;      // S: partners per item (measured: DESIGN.md, K17)

struct PairItem {
    int32_t row, p0, p1;      // the from-row and its slice [p0, p1) of the sorted keys
};

// the items of a row with `len` partners
K16_HD int32_t pair_item_count(int64_t len, int32_t S)
{
    if (len <= 0) return 0;
    return S <= 0 ? 1 : (int32_t)((len + S - 1) / S);
}

// the k-th item (0 <= k < pair_item_count(p1 - p0, S)) of row `row` with the range [p0, p1)
K16_HD PairItem pair_item_slice(int32_t row, int64_t p0, int64_t p1, int32_t k, int32_t S)
{
    if (S <= 0) return PairItem{row, (int32_t)p0, (int32_t)p1};
    const int64_t q0 = p0 + (int64_t)k * S, q1 = q0 + S < p1 ? q0 + S : p1;
    return PairItem{row, (int32_t)q0, (int32_t)q1};
}

// an upper bound of the items of `n_rows` rows that share `n_keys` keys: every row's last item may be short, the others are full
K16_HD int64_t pair_item_bound(int64_t n_rows, int64_t n_keys, int32_t S)
{
    const int64_t rows = n_rows < n_keys ? n_rows : n_keys;
    return S <= 0 ? rows : rows + n_keys / S;
}

}  // namespace pfz
