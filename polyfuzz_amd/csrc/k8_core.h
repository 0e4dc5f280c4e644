// K8's per-pair logic: the greedy Jaro matching as bit operations on one 32- or 64-bit word per string, and the float64 score.
// Plain integer C++ (and one float64 formula), shared by the HIP kernels and the host programs that check it against the
// definition on the CPU (tests/k8_core_host.cpp, tests/k20_core_host.cpp).  The kernels: k8_jaro.hip, the arg-max;
// k20_jaro_join.hip, which holds the bounds at the end of this file against a fixed t, and k21_jaro_topn.hip, which holds them
// against a floor that rises -- both through k8_sweep.h, the device code that walks one pair with these rules.
//
// The definition (jellyfish's jaro_similarity / jaro_winkler_similarity, default arguments, on code points):
//   r = max(max(la, lb) / 2 - 1, 0);  the from-characters i in order take the first unflagged j in [i - r, i + r] with
//   b[j] == a[i];  m = flagged pairs;  t = (k-th flagged a != k-th flagged b, counted over k) / 2;
//   w = (m/la + m/lb + (m - t)/m) / 3;  Winkler: w > 0.7 adds (l * 0.1) * (1 - w), l = common prefix, at most 4.
// Here the outer loop runs over the TO-string (a lane walks its to-string's characters; the from-string is the
// workgroup's match table PM[symbol] = positions of that symbol in a): to-character j takes the lowest unflagged set
// bit of PM[b[j]] inside its window.  Either orientation gave the same score on 1.1 million pairs (company names and
// dense random strings over 2..4 letters); the GPU tests compare with the from-major definition, exactly.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define K8_HD __host__ __device__ inline
#else
#define K8_HD inline
#endif

namespace pfz {

K8_HD int jaro_range(int la, int lb)
{
    const int r = (la > lb ? la : lb) / 2 - 1;
    return r > 0 ? r : 0;
}

// bits [lo, hi] of a word (0 <= lo, hi < its width; empty when lo > hi)
template <typename WORD> K8_HD WORD bit_span(int lo, int hi)
{
    constexpr int WB = (int)sizeof(WORD) * 8;
    return lo > hi ? (WORD)0 : (WORD)((WORD)~(WORD)0 >> (WB - 1 - hi)) & (WORD)((WORD)~(WORD)0 << lo);
}

// The from-string fits one WORD (32 or 64 characters): its flags are one word, and so are the flags of the stretch of
// WORD-many to-positions being walked (a longer to-string has several, see the kernel).
template <typename WORD> struct JaroFlags {
    WORD fa, fb;          // flagged from-positions / to-positions of the current stretch
    WORD win;             // the from-positions [j - r, j + r] of the current to-position j
    uint32_t pre;         // bit j < 4: a[j] == b[j]
    int r;
};

template <typename WORD> K8_HD void jaro_begin(JaroFlags<WORD> &s, int r)
{
    constexpr int WB = (int)sizeof(WORD) * 8;
    s.fa = s.fb = 0;
    s.pre = 0;
    s.r = r;
    s.win = bit_span<WORD>(0, r < WB - 1 ? r : WB - 1);
}

// sweep 1, to-position j = 0, 1, ... (bit jb of its stretch) with pm = PM[b[j]] (0 for the padding behind the string's end)
template <typename WORD> K8_HD void jaro_match(JaroFlags<WORD> &s, WORD pm, int j, int jb)
{
    const WORD x = pm & s.win & (WORD)~s.fa;
    s.fa |= x & (WORD)(0 - x);
    s.fb |= (WORD)(x != 0) << jb;
    if (j < 4) s.pre |= (uint32_t)((pm >> j) & 1) << j;
    s.win = (WORD)(s.win << 1) | (WORD)(j < s.r);       // [j - r, j + r] -> [j + 1 - r, j + 1 + r], cut to the word
}

// sweep 2, the to-positions again (bit jb of the stretch): a flagged one meets the lowest flagged from-position left;
// returns 1 when the two characters differ (a half transposition)
template <typename WORD> K8_HD int jaro_transpose(JaroFlags<WORD> &s, WORD pm, int jb)
{
    const WORD low = s.fa & (WORD)(0 - s.fa);
    const bool flagged = (s.fb >> jb) & 1;
    s.fa ^= flagged ? low : (WORD)0;
    return flagged && !(pm & low);
}

K8_HD int jaro_prefix(uint32_t pre) { return __builtin_ctz(~pre); }      // (four bits: at most 4)

// m flagged pairs, half_t differing flagged characters; float64, the definition's order of operations (the Winkler
// step must stay a product and a sum: fused, its last bit differs)
K8_HD double jaro_score(int m, int half_t, int la, int lb, int prefix, int winkler)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (m == 0) return 0.0;          // (an empty string on either side has no match)
    const double dm = (double)m;
    double w = (dm / (double)la + dm / (double)lb + (double)(m - half_t / 2) / dm) / 3.0;
    if (winkler && w > 0.7) w = w + ((double)prefix * 0.1) * (1.0 - w);
    return w;
}

// The score in float32, for "this pair cannot reach the running best" without three float64 divisions: bound + K8_BOUND_MARGIN
// (the float32 roundings are a hundred times smaller) >= the float64 score.  last = (m - t) / m, or 1 while t is not known
// (w grows with it).  Winkler's step grows with w (its slope is 1 - 0.1 l > 0), and is taken from a margin below 0.7 on: a w
// that float32 puts just below 0.7 may be above it.
constexpr float K8_BOUND_MARGIN = 1e-4f;
K8_HD float jaro_bound(int m, float inv_la, float inv_lb, float last, int prefix, int winkler)
{
    const float ub = ((float)m * inv_la + (float)m * inv_lb + last) * (1.0f / 3.0f);
    return winkler && ub > 0.7f - K8_BOUND_MARGIN ? ub + (float)prefix * 0.1f * (1.0f - ub) : ub;
}

// ---- against a threshold t (K20, k20_jaro_join.hip: fixed; K21, k21_jaro_topn.hip: the row's floor)  ---------------------------
// A pair is a hit iff jaro_score(...) >= t, float64 against float64, equal kept.  Everything below only DISMISSES pairs, and
// only where that comparison is false: the float32 bound + K8_BOUND_MARGIN is >= the float64 score, and the threshold it is held
// against is t rounded to float32 (a relative 6e-8, far inside the margin).  Each function grows (weakly) with m, with `last` and
// with the prefix, whatever the roundings: every operation in it is a correctly rounded monotone one.
// tests/k20_core_host.cpp walks all of it exhaustively against jaro_score.

// can a pair with m matches reach t?  false only where its score is < t.  m = 0 scores 0.0, a hit iff t == 0 -- asked first, so
// that the 0 * inf of an empty string never reaches a comparison
K8_HD bool jaro_reaches(int m, float inv_la, float inv_lb, float last, int prefix, int winkler, float t)
{
    if (m <= 0) return t <= 0.0f;
    return jaro_bound(m, inv_la, inv_lb, last, prefix, winkler) + K8_BOUND_MARGIN >= t;
}

K8_HD int jaro_min3(int a, int b, int c) { return a < b ? (a < c ? a : c) : (b < c ? b : c); }

// the length bound: every character of the shorter string matched, none transposed, the longest prefix the lengths allow.  For one
// la it rises with lb up to lb = la (where it is 1.0) and falls behind it: the admissible lb are one run around la.  The
// reciprocals are IEEE divisions here, on the device too: the run K20's set-up launch finds is the one the host finds.
K8_HD bool jaro_len_ok(int la, int lb, float t, int winkler)
{
    const int mn = la < lb ? la : lb;
    if (mn <= 0) return t <= 0.0f;
    return jaro_reaches(mn, 1.0f / (float)la, 1.0f / (float)lb, 1.0f, jaro_min3(4, la, lb), winkler, t);
}

// the run [*lo, *hi] of to-lengths lb <= lb_max a from-string of la characters can have a hit at (empty: *lo > *hi), by bisection
// over jaro_len_ok on either side of la
K8_HD void jaro_len_run(int la, int lb_max, float t, int winkler, int *lo, int *hi)
{
    if (t <= 0.0f) {
        *lo = 0;
        *hi = lb_max;
        return;
    }
    if (la <= 0) {              // (an empty string scores 0.0 against everything)
        *lo = 1;
        *hi = 0;
        return;
    }
    int a = 1, b = la;          // the smallest admissible lb: la itself is one
    while (a < b) {
        const int mid = a + (b - a) / 2;
        if (jaro_len_ok(la, mid, t, winkler)) b = mid;
        else a = mid + 1;
    }
    *lo = a;
    a = la;                     // the largest: bisection over [la, lb_max]
    b = lb_max > la ? lb_max : la;
    while (a < b) {
        const int mid = a + (b - a + 1) / 2;
        if (jaro_len_ok(la, mid, t, winkler)) a = mid;
        else b = mid - 1;
    }
    *hi = a;
}

// the fewest matches with which a pair of these lengths can still reach t (min(la, lb) + 1: with none): the bound with no
// transposition and the longest prefix the lengths allow, evaluated around a guess from its real-number form
K8_HD int jaro_m_need(int la, int lb, float inv_la, float inv_lb, float t, int winkler)
{
    const int mn = la < lb ? la : lb;
    if (t <= 0.0f) return 0;
    if (mn <= 0) return 1;
    const int prefix = jaro_min3(4, la, lb);
    // ub = (m (1/la + 1/lb) + 1) / 3 >= u, u the threshold below Winkler's step where the step can apply
    float u = t;
    if (winkler) {
        const float v = (t - 0.1f * (float)prefix) / (1.0f - 0.1f * (float)prefix);
        u = v > 0.7f ? v : (t < 0.7f ? t : 0.7f);
    }
    const float guess = (3.0f * u - 1.0f) / (inv_la + inv_lb);
    int m = guess > 0.0f ? (guess < (float)mn ? (int)guess : mn) : 0;
    while (m > 0 && jaro_reaches(m - 1, inv_la, inv_lb, 1.0f, prefix, winkler, t)) --m;
    while (m <= mn && !jaro_reaches(m, inv_la, inv_lb, 1.0f, prefix, winkler, t)) ++m;
    return m;
}

// mid-sweep: `flagged` matches so far, `remaining` to-characters still to come, each at most one more match
K8_HD bool jaro_dead(int la, int flagged, int remaining, int m_need)
{
    const int most = flagged + remaining;
    return (most < la ? most : la) < m_need;
}

}  // namespace pfz
