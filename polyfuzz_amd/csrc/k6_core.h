// K6's per-element decisions (k6_reductions.hip): what one thread decides about one row, one string or one similarity between
// two barriers.  Plain C++ over the arrays the kernels keep, shared by the HIP kernels -- which add the barriers, the atomics and
// the strided loops -- and a host program that drives the same functions phase by phase, sequentially, over every top-1 graph
// on a few rows and holds the result to the sequential walk (tests/k6_core_host.cpp, tests/test_k6_core_cpu.py).
//
// Linkage.  Row s of a top-1 result is (From = s, To = g_s, score); the kept rows are walked in order (k6_reductions.hip has the
// walk and why the phases below restate it).  The arrays, one int32 per row / string:
//   state[x]  bit 1: row x is in R (kept, and not the first kept row t0);  bit 0: row x is active (its From was unmapped or in
//             cluster 0 when the walk reached it) -- a guess while the fixpoint runs, the truth once a round changes nothing;
//   fin[x]    the first active row whose To is x, kLinkInf if there is none -- a row whose To is ITSELF included;
//   ptr[x]    whose cluster x takes: its To for an active row, x itself otherwise (a root).
// A row with g_s == s ("From == To": a list matched against itself as two lists) is an ordinary row here: it is active exactly
// when no active EARLIER row points at s, and then it founds a cluster with itself -- link_active asks fin[x] >= x, not > x,
// because fin[x] == x is that row's own edge and says nothing about earlier rows.  (With > x such a row flips between active and
// inactive for ever: the kernel spun.)  active[x] therefore depends on active[s] for s < x only, so round k of the fixpoint
// settles index k - 1, and a further round sees no change: at most n + 1 rounds (link_round_cap).  The adoption chains of
// active rows fall strictly in index and halve per round of pointer jumping: at most ceil(log2 n) + 2 rounds (link_jump_cap).
// Both caps are carried by the kernel and by the host program; no input reaches them.
//
// PR curve.  pr_bin: the number of ascending thresholds <= v (numpy.searchsorted(thr, v, side="right")); pr_scale / pr_fixed: the
// int64 fixed point the sums are kept in -- scale = 2^(61 - e) with frexp(n * max|v|) = (m, e), so that |sum of n values| * scale
// < 2^61 and every value is rounded ONCE, to the nearest multiple of 1 / scale (an error of at most 2^(e - 62) per value).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define K6_HD __host__ __device__ inline
#else
#define K6_HD inline
#endif

namespace pfz {

constexpr int32_t kLinkInf = 0x7fffffff;
enum LinkStatus { kLinkDone = 0, kLinkFixpointOverrun = 1, kLinkJumpOverrun = 2 };

// the frame's row survives `matches.Similarity > min_similarity`: Similarity = np.round(float64(score), 3), a score that rounds
// below 0.001 or an index outside [0, n) is a row without a match (To = None, Similarity = 0: never > thr >= 0)
K6_HD bool kept_row(int32_t g, float v, int32_t n, double thr)
{
    const double r3 = rint((double)v * 1000.0) / 1000.0;
    return g >= 0 && g < n && r3 >= 0.001 && r3 > thr;
}

K6_HD int32_t link_initial_state(bool kept, int32_t x, int32_t t0) { return kept && x != t0 ? 3 : 0; }

// state of x after one round, given fin of the round's active rows.  fin[x] == x is x's own edge (g_x == x).
K6_HD int32_t link_active(int32_t st, int32_t fin_x, int32_t x) { return (st & 2) ? (2 | (fin_x >= x ? 1 : 0)) : st; }

// active row s (To g) founds a cluster: it is the first active row at g, and g's own row did not map g before
K6_HD bool link_founding(int32_t s, int32_t g, int32_t fin_g, int32_t state_g) { return fin_g == s && !((state_g & 2) && g < s); }

// string x was mapped by a founding row (fin_x, as its To) and not by its own row before that
K6_HD bool link_founded(int32_t x, int32_t fin_x, int32_t state_x) { return fin_x != kLinkInf && !((state_x & 2) && x < fin_x); }

K6_HD int32_t link_pointer(int32_t st, int32_t s, int32_t g) { return (st & 1) ? g : s; }

K6_HD int32_t link_round_cap(int32_t n) { return n + 1; }
K6_HD int32_t link_jump_cap(int32_t n)
{
    int32_t lg = 0;
    while (lg < 31 && ((int64_t)1 << lg) < n) ++lg;
    return lg + 2;
}

// cluster 0: the first kept row's To and From entered the dict first and keep that place; whoever of them no later row
// re-assigned stays in cluster 0.  One thread, after everything else.
K6_HD void link_patch_cluster0(int32_t t0, int32_t g0, int32_t *cluster, int32_t *key)
{
    if (cluster[g0] < 0) cluster[g0] = 0;
    if (cluster[t0] < 0) cluster[t0] = 0;
    key[g0] = 2 * t0;
    key[t0] = 2 * t0 + 1;
}

// number of thresholds <= v (thr ascending, repeats allowed); v is not NaN
template <class ThrPtr> K6_HD int32_t pr_bin(ThrPtr thr, int32_t n_thr, double v)
{
    int32_t lo = 0, hi = n_thr;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (thr[mid] <= v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

K6_HD double pr_scale(int64_t n, double max_abs)
{
    int e = 0;
    frexp((double)(n > 0 ? n : 1) * (max_abs > 0.0 ? max_abs : 1.0), &e);
    return ldexp(1.0, 61 - e);
}

// two's complement: the sums are added as unsigned words, negative values included
K6_HD unsigned long long pr_fixed(double v, double scale) { return (unsigned long long)llrint(v * scale); }

}  // namespace pfz
