// K9's per-pair logic: the unit-cost Levenshtein distance and the optimal-string-alignment (OSA) distance as the bit-vector
// recurrence of Myers / Hyyro, on one 32- or 64-bit word per from-string or on several 64-bit words, and the float64 similarity.
// Plain integer C++ (and one float64 formula), shared by the HIP kernels (k9_levenshtein.hip, k10_pairs.hip, k11_join.hip and
// k12_components.hip through edit_walk.h) and a host program that checks it against the textbook table on the CPU
// (tests/k9_core_host.cpp).
//
// The definition (rapidfuzz's Levenshtein.normalized_similarity / OSA.normalized_similarity, default arguments, on code points):
//   d = the fewest unit-cost insertions, deletions and substitutions that turn a into b; OSA also counts the transposition of two
//   adjacent characters as one edit, no substring edited twice (osa("CA","ABC") = 3, osa("ab","ba") = 1);
//   M = max(|a|, |b|);  sim = 1.0 - (double)d / (double)M, 1.0 when M = 0 -- one division, one subtraction, not fused.
// A lane walks its to-string's characters c with Eq = PM[c] (bit i: a[i] == c; the from-string is the workgroup's match table):
// VP / VN are the +1 / -1 vertical deltas of the table's current column, dist its last cell.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define K9_HD __host__ __device__ inline
#else
#define K9_HD inline
#endif

namespace pfz {

// the lowest n bits of a word (0 <= n <= its width)
template <typename WORD> K9_HD WORD low_ones(int n)
{
    constexpr int WB = (int)sizeof(WORD) * 8;
    return n <= 0 ? (WORD)0 : (WORD)((WORD)~(WORD)0 >> (WB - (n < WB ? n : WB)));
}

// The from-string fits one WORD (32 or 64 characters).
template <typename WORD> struct LevState {
    WORD vp, vn;
    WORD d0, eq_prev;     // the previous step's, for OSA's transposition term
    WORD last;            // bit la - 1 (0 for an empty from-string: dist never moves, see lev_distance)
    int dist;
};

template <typename WORD> K9_HD void lev_begin(LevState<WORD> &s, int la)
{
    s.vp = low_ones<WORD>(la);
    s.vn = s.d0 = s.eq_prev = 0;
    s.last = la > 0 ? (WORD)((WORD)1 << (la - 1)) : (WORD)0;
    s.dist = la;
}

// one to-character; `live` = the character is inside the lane's to-string (the padding behind its end must not move dist)
template <typename WORD, bool OSA> K9_HD void lev_step(LevState<WORD> &s, WORD eq, bool live)
{
    const WORD tr = OSA ? (WORD)((WORD)(((WORD)~s.d0 & eq) << 1) & s.eq_prev) : (WORD)0;
    const WORD d0 = (WORD)((WORD)((WORD)((WORD)(eq & s.vp) + s.vp) ^ s.vp) | eq | s.vn | tr);
    WORD hp = (WORD)(s.vn | (WORD)~(d0 | s.vp));
    WORD hn = (WORD)(d0 & s.vp);
    const int delta = (int)((hp & s.last) != 0) - (int)((hn & s.last) != 0);
    s.dist += live ? delta : 0;
    hp = (WORD)((WORD)(hp << 1) | (WORD)1);
    hn = (WORD)(hn << 1);
    s.vp = (WORD)(hn | (WORD)~(d0 | hp));
    s.vn = (WORD)(hp & d0);
    s.d0 = d0;
    s.eq_prev = eq;
}

// the distance after the lane's lb characters (an empty from-string has no last row bit: d = lb)
K9_HD int lev_distance(int dist, int la, int lb) { return la == 0 ? lb : dist; }

// The multi-word form: the from-string is W 64-bit words, the recurrence is the one above on a W x 64-bit integer.  What crosses
// from word w to word w + 1 within one step: the carry of the addition, and the bits shifted out of HP, HN and OSA's operand.
struct LevCarry {
    uint64_t add, hp, hn, tr;      // (0 / 1 each)
};

K9_HD LevCarry lev_carry_begin() { return LevCarry{0, 1, 0, 0}; }       // (HP << 1) | 1: a one is shifted into word 0

// word w of one step: vp / vn / d0 are that word's state (d0 the previous step's D0), eq / eq_prev its match bits of this and of
// the previous to-character; returns the word's HP and HN before the shift in *hp_out / *hn_out (the last word's hold bit la - 1)
template <bool OSA>
K9_HD void lev_step_word(uint64_t &vp, uint64_t &vn, uint64_t &d0_io, uint64_t eq, uint64_t eq_prev, LevCarry &c, uint64_t *hp_out,
                         uint64_t *hn_out)
{
    uint64_t tr = 0;
    if (OSA) {
        const uint64_t x = ~d0_io & eq;
        tr = ((x << 1) | c.tr) & eq_prev;
        c.tr = x >> 63;
    }
    const uint64_t x = eq & vp;
    const uint64_t s1 = x + vp;
    const uint64_t sum = s1 + c.add;
    c.add = (uint64_t)(s1 < x) | (uint64_t)(sum < s1);
    const uint64_t d0 = (sum ^ vp) | eq | vn | tr;
    const uint64_t hp = vn | ~(d0 | vp);
    const uint64_t hn = d0 & vp;
    *hp_out = hp;
    *hn_out = hn;
    const uint64_t hps = (hp << 1) | c.hp, hns = (hn << 1) | c.hn;
    c.hp = hp >> 63;
    c.hn = hn >> 63;
    vp = hns | ~(d0 | hps);
    vn = hps & d0;
    d0_io = d0;
}

// A lane's multi-word column where the general kernels keep it: word w of VP / VN / D0 at vp / vn / d0[w * stride] (stride = the
// lanes that interleave their columns: 256, or 64 in K10), W words for a from-string of la characters.
#define K9_HD_FLAT K9_HD __attribute__((always_inline))

K9_HD_FLAT void lev_column_begin(uint64_t *vp, uint64_t *vn, uint64_t *d0, int W, int la, int stride)
{
    for (int w = 0; w < W; ++w) {
        vp[(int64_t)w * stride] = low_ones<uint64_t>(la - 64 * w);
        vn[(int64_t)w * stride] = 0ull;
        d0[(int64_t)w * stride] = 0ull;
    }
}

// one to-character: eq / eq_prev = the W match words of this and of the previous to-character (eq_prev and d0 are read for OSA
// alone); returns what dist moves by (`last` = bit la - 1 of the column's last word, 0 for an empty from-string)
template <bool OSA>
K9_HD_FLAT int lev_column_step(uint64_t *vp, uint64_t *vn, uint64_t *d0, const uint64_t *eq, const uint64_t *eq_prev, int W,
                               uint64_t last, int stride)
{
    LevCarry cy = lev_carry_begin();
    uint64_t hp = 0, hn = 0;
    for (int w = 0; w < W; ++w) {
        uint64_t x_vp = vp[(int64_t)w * stride], x_vn = vn[(int64_t)w * stride], x_d0 = OSA ? d0[(int64_t)w * stride] : 0ull;
        lev_step_word<OSA>(x_vp, x_vn, x_d0, eq[w], OSA ? eq_prev[w] : 0ull, cy, &hp, &hn);
        vp[(int64_t)w * stride] = x_vp;
        vn[(int64_t)w * stride] = x_vn;
        if (OSA) d0[(int64_t)w * stride] = x_d0;
    }
    return (int)((hp & last) != 0) - (int)((hn & last) != 0);
}

// float64, the definition's order of operations (a fused multiply-add has no place here, but say so)
K9_HD double lev_similarity(int d, int la, int lb)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int m = la > lb ? la : lb;
    if (m == 0) return 1.0;
    return 1.0 - (double)d / (double)m;
}

// d >= | |a| - |b| |: no pair of these lengths scores above this (the same formula: rounding cannot put a score above its bound)
K9_HD double lev_length_bound(int la, int lb) { return lev_similarity(la > lb ? la - lb : lb - la, la, lb); }

}  // namespace pfz
