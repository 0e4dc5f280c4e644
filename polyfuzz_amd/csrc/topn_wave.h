// Exact per-row top-n of the all-pairs edit-distance kernels (K4 ratio, K9 Levenshtein / OSA, K19 the per-pair scorers, K21 Jaro): the `ntop` best choices of a
// from-string in the order (float64 score descending, original to-index ascending) -- np.argsort(-scores, kind="stable")[:ntop]
// on the scores the reference computes (polyfuzz/models/_distance.py:89-102); entry 0 is the arg-max kernels' first maximum.
//
// No lane keeps a list.  A WAVE keeps one sorted list, entry p in lane p, in two registers per lane (that is why ntop <= 64).
// After a group of 64 pairs is scored, the lanes whose pair beats the list's entry ntop - 1 are taken one at a time: their
// key is read from its lane, every lane compares it with its own entry, the number of entries that stay in front of it --
// the bit count of that ballot: the list is sorted, the better entries are a prefix -- is its place, and the lanes behind
// move up by one with a wave shuffle.  Once the list is full a key that does not beat entry ntop - 1 costs one compare.
// Every wave leaves its list in global memory (TopnKey[ntop] per wave, every list written, the empty ones too: no memset);
// topn_merge (pfz_api.hip) picks a row's top-n out of the lists of its waves and parts with the same insertion, one wave per
// row.  A launch has a list buffer of its own: rows x parts of THAT launch x 4 waves x ntop keys of 16 bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

namespace pfz {

constexpr int kTopnMax = 64;          // one list entry per lane of a wave

struct TopnKey {
    double score;
    int32_t idx, pad;                 // idx < 0: no entry (what a memset to 0xff leaves)
};

// a wave's list: this lane's entry.  idx == INT_MAX: empty -- with score -1 it is behind every real key (scores are >= 0)
struct TopnList {
    double score;
    int idx;
};

__device__ inline TopnList topn_empty() { return TopnList{-1.0, INT_MAX}; }

__device__ inline bool topn_before(double sa, int ia, double sb, int ib) { return sa > sb || (sa == sb && ia < ib); }

// is the list's entry ntop - 1 a real one (then ntop choices at or above its score exist), and its score
__device__ inline bool topn_full(const TopnList &l, int ntop, double *last_score)
{
    *last_score = __shfl(l.score, ntop - 1, 64);
    return __shfl(l.idx, ntop - 1, 64) != INT_MAX;
}

// Every lane offers one key (have: it has one).  Wave-uniform control flow: all 64 lanes of the wave must call.
__device__ inline void topn_insert(TopnList &l, int ntop, bool have, double score, int idx)
{
    const int lane = threadIdx.x & 63;
    // (the shuffles in statements of their own: inside `have && ...` only the lanes that have a key would take part, and a
    // shuffle reads nothing from a lane that does not -- entry ntop - 1 may well sit in one)
    const double last_score = __shfl(l.score, ntop - 1, 64);
    const int last_idx = __shfl(l.idx, ntop - 1, 64);
    unsigned long long todo = __ballot(have && topn_before(score, idx, last_score, last_idx));
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const double cs = __shfl(score, src, 64);
        const int ci = __shfl(idx, src, 64);
        // (the entries in front of the key; the list may have changed since the ballot above: a key that no longer makes it is dropped)
        const int pos = __popcll(__ballot(topn_before(l.score, l.idx, cs, ci)));
        if (pos >= ntop) continue;
        const double us = __shfl_up(l.score, 1, 64);
        const int ui = __shfl_up(l.idx, 1, 64);
        if (lane > pos) {
            l.score = us;
            l.idx = ui;
        }
        else if (lane == pos) {
            l.score = cs;
            l.idx = ci;
        }
    }
}

__device__ inline void topn_store(const TopnList &l, int ntop, TopnKey *dst)
{
    const int lane = threadIdx.x & 63;
    if (lane < ntop) {
        dst[lane].score = l.score;
        dst[lane].idx = l.idx == INT_MAX ? -1 : l.idx;
    }
}

// The row's top-n out of the lists its waves and parts left, the same insertion, one wave per row (pfz_api.hip).  Row r of the
// n_rows of a launch owns the n_lists lists of ntop keys at lists[r * n_lists * ntop]; every one of them was written (an empty
// entry has idx < 0).  Its result goes to row rows[r] - from_begin (rows == NULL: r) of out_idx / out_score (device,
// [.. * ntop]): -1 / 0.0 beyond the choices the row has.  Enqueues on `st`.
int topn_merge(const TopnKey *lists, int32_t n_lists, int32_t ntop, const int32_t *rows, int64_t from_begin, int64_t n_rows,
               int32_t *out_idx, double *out_score, hipStream_t st);

}  // namespace pfz
