// One GIVEN pair under an edit-distance scorer, as the kernels that are handed their pairs score it -- K10 (k10_pairs.hip: a
// candidate table re-ranked) and K16 (k16_pairs_join.hip: the same table against a threshold).  The from-string is in the wave's
// match table, the lane gathers its to-string's code units (1 or 4 bytes) from the raw pfz_strings buffers and maps them through
// the plan's code unit -> symbol table.  The scorers are K4's ratio, K9's Levenshtein / OSA and K8's Jaro / Jaro-Winkler; a pair's
// float64 score comes from the very functions those kernels call (k10_core.h ratio_of, k9_core.h, k8_core.h), so both kernels
// give a pair the bits the all-pairs kernels produce for it.
//   pair_score_reg      the from-string fits one 32- or 64-bit word, its match table is one LDS word per symbol; Jaro keeps a
//                       to-string's flag words in registers with compile-time indices (256 positions, as K8): longer partners are
//                       the general kernel's;
//   pair_score_general  any lengths, any alphabet: match table and the lane's words in global memory.
#pragma once

#include "edit_walk.h"
#include "k10_core.h"
#include "k8_core.h"

namespace pfz {

constexpr int kPairsMaxCandidates = 1024;      // per row, as pfz_dense_rescore_topn
constexpr int kPairsJaroRegLen = 256;          // to-positions whose flags the Jaro register kernel keeps

enum { PAIR_RATIO = 0, PAIR_LEVENSHTEIN = 1, PAIR_OSA = 2, PAIR_JARO = 3, PAIR_JARO_WINKLER = 4 };
enum { MODE_REG32 = 0, MODE_REG64 = 1, MODE_GENERAL = 2 };

struct PairView : FromView {   // (the plan's packed groups are not read here)
    const void *b_chars;       // to-strings, the raw list
    int32_t b_width;
    const int64_t *b_off;      // [n_to + 1]
    int64_t n_to;
    int32_t scorer;            // PAIR_*
};

// one pair in registers: the from-string is in the wave's match table `pm`, the lane walks its to-string [b0, b0 + lb)
template <typename WORD, int FAMILY>      // FAMILY: PAIR_RATIO, PAIR_LEVENSHTEIN, PAIR_OSA, PAIR_JARO (Winkler: A.scorer)
__device__ __forceinline__ double pair_score_reg(const PairView &A, const WORD *pm, int la, int64_t b0, int lb)
{
    if constexpr (FAMILY == PAIR_RATIO) {
        WORD v = (WORD)~(WORD)0;
        for (int t = 0; t < lb; ++t) lcs_step_reg<WORD>(v, pm[edit_symbol(A, A.b_chars, A.b_width, b0 + t)]);
        const int lcs = __popcll((uint64_t)(WORD)~v);
        return la + lb == 0 ? 100.0 : ratio_of(lcs, (int64_t)la + lb);
    }
    else if constexpr (FAMILY == PAIR_LEVENSHTEIN || FAMILY == PAIR_OSA) {
        LevState<WORD> s;
        lev_begin(s, la);
        for (int t = 0; t < lb; ++t) lev_step<WORD, FAMILY == PAIR_OSA>(s, pm[edit_symbol(A, A.b_chars, A.b_width, b0 + t)], true);
        return lev_similarity(lev_distance(s.dist, la, lb), la, lb);
    }
    else {
        constexpr int WB = (int)sizeof(WORD) * 8;
        constexpr int NB = kPairsJaroRegLen / WB;      // lb <= 256: the caller's promise
        JaroFlags<WORD> s;
        WORD fb[NB];
        jaro_begin(s, jaro_range(la, lb));
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            s.fb = 0;
            const int hi = min(lb, (k + 1) * WB);
            for (int j = k * WB; j < hi; ++j) jaro_match<WORD>(s, pm[edit_symbol(A, A.b_chars, A.b_width, b0 + j)], j, j - k * WB);
            fb[k] = s.fb;
        }
        const int m = __popcll((uint64_t)s.fa);
        const int prefix = jaro_prefix(s.pre);
        int half_t = 0;
        if (m >= 2) {          // (one flagged pair cannot be out of order)
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                s.fb = fb[k];
                const int hi = min(lb, (k + 1) * WB);
                for (int j = k * WB; j < hi; ++j)
                    half_t += jaro_transpose<WORD>(s, pm[edit_symbol(A, A.b_chars, A.b_width, b0 + j)], j - k * WB);
            }
        }
        return jaro_score(m, half_t, la, lb, prefix, A.scorer == PAIR_JARO_WINKLER);
    }
}

// one pair of the general kernel: the from-string's match table `pm` (WA words per symbol, W of them in use) and this lane's words
// s0 / s1 / s2[w * 64] are in global memory
__device__ __forceinline__ double pair_score_general(const PairView &A, const uint64_t *pm, uint64_t *s0, uint64_t *s1, uint64_t *s2,
                                                     int WA, int W, int la, int64_t b0, int lb)
{
    if (A.scorer == PAIR_RATIO) {
        for (int w = 0; w < W; ++w) s0[(int64_t)w * 64] = ~0ull;
        for (int t = 0; t < lb; ++t) {
            const uint64_t *pmc = pm + (int64_t)edit_symbol(A, A.b_chars, A.b_width, b0 + t) * WA;
            uint64_t carry = 0;
            for (int w = 0; w < W; ++w) {
                uint64_t v = s0[(int64_t)w * 64];
                lcs_step_word(v, pmc[w], carry);
                s0[(int64_t)w * 64] = v;
            }
        }
        int lcs = 0;
        for (int w = 0; w < W; ++w) lcs += __popcll(~s0[(int64_t)w * 64]);
        return la + lb == 0 ? 100.0 : ratio_of(lcs, (int64_t)la + lb);
    }
    if (A.scorer == PAIR_LEVENSHTEIN || A.scorer == PAIR_OSA) {
        // s0 / s1 / s2: VP / VN / the previous step's D0
        const bool osa = A.scorer == PAIR_OSA;
        lev_column_begin(s0, s1, s2, W, la, 64);
        const uint64_t last = la > 0 ? 1ull << ((la - 1) % 64) : 0ull;
        int dist = la;
        int c_prev = 0;                                         // (symbol 0: an empty table entry)
        for (int t = 0; t < lb; ++t) {
            const int c = edit_symbol(A, A.b_chars, A.b_width, b0 + t);
            const uint64_t *eq = pm + (int64_t)c * WA, *eq_prev = pm + (int64_t)c_prev * WA;
            dist += osa ? lev_column_step<true>(s0, s1, s2, eq, eq_prev, W, last, 64) : lev_column_step<false>(s0, s1, s2, eq, eq_prev, W, last, 64);
            c_prev = c;
        }
        return lev_similarity(lev_distance(dist, la, lb), la, lb);
    }
    // Jaro.  s0: the flagged from-positions (W words), s1: the flagged to-positions ((lb + 63) / 64 words <= WS)
    const int WBl = lb > 0 ? (lb + 63) / 64 : 1;
    const int range = jaro_range(la, lb);
    for (int w = 0; w < W; ++w) s0[(int64_t)w * 64] = 0ull;
    for (int w = 0; w < WBl; ++w) s1[(int64_t)w * 64] = 0ull;
    int m = 0;
    uint32_t pre = 0;
    for (int t = 0; t < lb; ++t) {
        const uint64_t *pmc = pm + (int64_t)edit_symbol(A, A.b_chars, A.b_width, b0 + t) * WA;
        if (t < 4) pre |= (uint32_t)((pmc[0] >> t) & 1) << t;
        const int lo = max(t - range, 0), hi = min(t + range, la - 1);
        for (int w = lo >> 6; w <= hi >> 6 && lo <= hi; ++w) {
            const uint64_t f = s0[(int64_t)w * 64];
            const uint64_t x = pmc[w] & bit_span<uint64_t>(max(lo - 64 * w, 0), min(hi - 64 * w, 63)) & ~f;
            if (x) {
                s0[(int64_t)w * 64] = f | (x & (0 - x));
                s1[(int64_t)(t >> 6) * 64] |= 1ull << (t & 63);
                ++m;
                break;
            }
        }
    }
    int half_t = 0;
    if (m >= 2) {
        int wa = 0;
        uint64_t cur = s0[0];
        for (int t = 0; t < lb; ++t) {
            if (!((s1[(int64_t)(t >> 6) * 64] >> (t & 63)) & 1)) continue;
            while (cur == 0 && wa + 1 < W) cur = s0[(int64_t)(++wa) * 64];      // (as many flags on either side)
            const uint64_t low = cur & (0 - cur);
            cur ^= low;
            half_t += !(pm[(int64_t)edit_symbol(A, A.b_chars, A.b_width, b0 + t) * WA + wa] & low);
        }
    }
    return jaro_score(m, half_t, la, lb, jaro_prefix(pre), A.scorer == PAIR_JARO_WINKLER);
}

}  // namespace pfz
