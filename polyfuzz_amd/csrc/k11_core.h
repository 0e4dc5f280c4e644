// K11's per-pair logic on top of K9's (k9_core.h: the recurrence, the distance, the float64 similarity -- used unchanged): what a
// known threshold t lets a lane leave out, exactly.  Plain integer C++ and K9's one float64 formula, shared by the HIP kernels
// (k11_join.hip) and a host program that checks it exhaustively on the CPU (tests/k11_core_host.cpp).
//
// Pair (a, b) is a hit iff lev_similarity(d, |a|, |b|) >= t, float64 against float64 (rapidfuzz's score_cutoff: equal is a hit).
// The similarity falls strictly as d rises (tests/test_levenshtein_cpu.py), so the hits of a pair of lengths are d = 0 .. kmax:
//   join_kmax(t, la, lb) = the largest d in 0 .. max(la, lb) with lev_similarity(d, la, lb) >= t, -1 if there is none.
// It is found by EVALUATING that formula around a guess, never by floor((1 - t) * M) alone, which rounding puts off by one.
// Two lower bounds of d are held against it:
//   the lengths:   d >= | |a| - |b| |                      (join_in_window; the same test as lev_length_bound(la, lb) >= t)
//   the walk:      d >= dist_j - (lb - j) after j of the lb to-characters -- the bottom cell of the column moves by at most 1 per
//                  to-character, under OSA too (checked exhaustively by the host program)       (join_abandon)
// A pair is left out only where a lower bound of d exceeds kmax, i.e. where the formula on that bound is < t.
//
// The packed hit, one 64-bit key that sorts by (row, to-index):  row << 40 | to-index << 16 | d.
// Limits it implies (pfz_lev_join refuses beyond them, PFZ_ERR_UNSUPPORTED): lists of at most 2^24 strings, strings of at most
// 65 535 characters (d <= max(|a|, |b|)).
#pragma once

#include "k9_core.h"

namespace pfz {

constexpr int64_t kJoinMaxStrings = (int64_t)1 << 24;
constexpr int64_t kJoinMaxLength = 65535;

K9_HD int join_kmax(double t, int la, int lb)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int m = la > lb ? la : lb;
    if (m == 0) return lev_similarity(0, 0, 0) >= t ? 0 : -1;
    double guess = (1.0 - t) * (double)m;           // a starting point only: the two loops below decide
    int k = guess >= (double)m ? m : (guess <= 0.0 ? 0 : (int)guess);
    while (k < m && lev_similarity(k + 1, la, lb) >= t) ++k;
    while (k >= 0 && !(lev_similarity(k, la, lb) >= t)) --k;
    return k;
}

// the length bound passes: some distance these two lengths allow is a hit
K9_HD bool join_in_window(int kmax, int la, int lb) { return kmax >= (la > lb ? la - lb : lb - la); }

// after j (<= lb) to-characters with the column's bottom cell at `dist`: no continuation reaches d <= kmax
K9_HD bool join_abandon(int dist, int j, int lb, int kmax) { return dist - (lb - j) > kmax; }

K9_HD uint64_t join_pack(int row, int to, int d) { return (uint64_t)(uint32_t)row << 40 | (uint64_t)(uint32_t)to << 16 | (uint64_t)(uint32_t)d; }
K9_HD int join_key_row(uint64_t key) { return (int)(key >> 40); }
K9_HD int join_key_to(uint64_t key) { return (int)((key >> 16) & 0xffffffu); }
K9_HD int join_key_dist(uint64_t key) { return (int)(key & 0xffffu); }

// The row pointers over `total` (>= 1) hits sorted by row, position p's share: hit p belongs to `row`, hit p - 1 to `prev` (-1 for
// p = 0), and every row that begins between the two begins at p -- row_ptr[r] = p for prev < r <= row; the last position also closes
// the rows behind its own, up to row_ptr[n_rows] = total.  Over p = 0 .. total - 1 every row_ptr[0 .. n_rows] is written exactly
// once.  PTR: int64_t (K11, K13, K14 / K15's unpack) or int32_t (K16's segments); `row` may be n_rows itself (K16's keys that are
// no pair).
template <typename PTR> K9_HD void rows_fill(int64_t prev, int64_t row, int64_t p, int64_t total, int64_t n_rows, PTR *row_ptr)
{
    for (int64_t r = prev + 1; r <= row; ++r) row_ptr[r] = (PTR)p;
    if (p == total - 1)
        for (int64_t r = row + 1; r <= n_rows; ++r) row_ptr[r] = (PTR)total;
}

}  // namespace pfz
