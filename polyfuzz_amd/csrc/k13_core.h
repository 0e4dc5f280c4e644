// K13's per-pair logic on top of K10's (k10_core.h: the bit-parallel LCS, lcs_step_reg / lcs_step_word -- used unchanged): the
// Indel similarity on the 0..1 scale (rapidfuzz.distance.Indel.normalized_similarity; fuzz.ratio is this value times 100) and
// what a known threshold t lets a lane leave out, exactly.  Plain integer C++ and one float64 formula, shared by the HIP kernels
// (k13_indel_join.hip) and a host program that checks it exhaustively on the CPU (tests/k13_core_host.cpp).
//
// The definition, on code points:  lcs = the length of the longest common subsequence, S = |a| + |b|, d = S - 2 lcs;
//   indel_similarity = 1.0 - (double)d / (double)S, 1.0 when S = 0 -- one division, one subtraction, not fused.
// Pair (a, b) is a hit iff indel_similarity >= t, float64 against float64 (rapidfuzz's score_cutoff: equal is a hit).  The
// similarity depends on the lengths through S alone and rises strictly with lcs, so the hits of a pair are lcs >= lmin:
//   indel_lmin(t, S) = the smallest lcs in 0 .. S / 2 with indel_similarity(lcs, S) >= t, S / 2 + 1 if there is none.
// It is found by EVALUATING that formula around a guess, never by ceil(t * S / 2) alone, which rounding puts off by one.
// Two upper bounds of lcs are held against it:
//   the lengths:   lcs <= min(|a|, |b|)                                                              (indel_in_window)
//   the walk:      lcs <= l_j + (lb - j) after j of the lb to-characters, l_j the LCS of a and b's first j characters -- the LCS
//                  grows by at most 1 per to-character                                                (indel_abandon)
// A pair is left out only where an upper bound of lcs is below lmin, i.e. where the formula on that bound is < t.
//
// The packed hit is K11's key (k11_core.h join_pack) with the LCS in the low 16 bits:  row << 40 | to-index << 16 | lcs.
// lcs, not d: d reaches 131 070 and does not fit, lcs <= min(|a|, |b|) <= 65 535 does.  Limits it implies (pfz_indel_join refuses
// beyond them, PFZ_ERR_UNSUPPORTED), K11's: lists of at most 2^24 strings, strings of at most 65 535 characters.
#pragma once

#include "k10_core.h"
#include "k11_core.h"

namespace pfz {

// float64, the definition's order of operations; S = |a| + |b|
K10_HD double indel_similarity(int lcs, int64_t S)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (S == 0) return 1.0;
    return 1.0 - (double)(S - 2 * (int64_t)lcs) / (double)S;
}

K10_HD double indel_similarity(int lcs, int la, int lb) { return indel_similarity(lcs, (int64_t)la + (int64_t)lb); }

K10_HD int indel_lmin(double t, int S)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int h = S / 2;
    double guess = t * (double)S * 0.5;             // a starting point only: the two loops below decide
    int l = guess >= (double)h ? h : (guess <= 0.0 ? 0 : (int)guess);
    while (l > 0 && indel_similarity(l - 1, S) >= t) --l;
    while (l <= h && !(indel_similarity(l, S) >= t)) ++l;
    return l;
}

// the length bound passes: some LCS these two lengths allow is a hit (lmin = indel_lmin(t, la + lb))
K10_HD bool indel_in_window(int lmin, int la, int lb) { return (la < lb ? la : lb) >= lmin; }

// after j (<= lb) to-characters with an LCS of l_j so far: no continuation reaches lcs >= lmin
K10_HD bool indel_abandon(int l_j, int j, int lb, int lmin) { return l_j + (lb - j) < lmin; }

// the LCS a one-word column V stands for: its zero bits among the from-string's la positions
K10_HD int indel_lcs_of(uint32_t v, int la) { return __builtin_popcount(~v & low_ones<uint32_t>(la)); }
K10_HD int indel_lcs_of(uint64_t v, int la) { return __builtin_popcountll(~v & low_ones<uint64_t>(la)); }

K10_HD int indel_distance(int lcs, int la, int lb) { return la + lb - 2 * lcs; }

}  // namespace pfz
