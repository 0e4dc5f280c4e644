// The Indel ratio's per-pair logic as K10 walks it (k10_pairs.hip): the bit-parallel LCS of Crochemore / Hyyro on one 32- or 64-bit
// word per from-string or on several 64-bit words, and rapidfuzz.fuzz.ratio's float64 formula, which K4 (k4_indel.hip) shares.
// Plain integer C++ (and one float64 formula), compiled for the device and for a host program that holds the LCS to the textbook
// table on the CPU (tests/k10_core_host.cpp).
//
// With PM[c] = the positions of character c in the from-string and V = all ones, every to-character c does
//     u = V & PM[c];  V = (V + u) | (V & ~u)
// and LCS(a, b) = the number of zero bits of V among the from-string's positions (the bits above |a| never leave one: PM has
// nothing there).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define K10_HD __host__ __device__ inline
#else
#define K10_HD inline
#endif

namespace pfz {

// the from-string fits one WORD
template <typename WORD> K10_HD void lcs_step_reg(WORD &v, WORD pm)
{
    const WORD u = (WORD)(v & pm);
    v = (WORD)((WORD)(v + u) | (WORD)(v & (WORD)~u));
}

// word w of one step of the multi-word form: `carry` (0 / 1) is what the addition of word w - 1 left, 0 in front of word 0
K10_HD void lcs_step_word(uint64_t &v, uint64_t pm, uint64_t &carry)
{
    const uint64_t u = v & pm;
    const uint64_t s1 = v + u;
    const uint64_t sum = s1 + carry;
    carry = (uint64_t)(s1 < v) | (uint64_t)(sum < s1);
    v = sum | (v & ~u);
}

// rapidfuzz: norm_dist = dist / maximum (0 when both empty); ratio = (1 - norm_dist) * 100 -- maximum = |a| + |b|, so two empty
// strings score 100.0
K10_HD double ratio_of(int lcs, int64_t maximum)
{
    const int64_t dist = maximum - 2 * (int64_t)lcs;
    const double norm_dist = maximum != 0 ? (double)dist / (double)maximum : 0.0;
    return (1.0 - norm_dist) * 100.0;
}

}  // namespace pfz
