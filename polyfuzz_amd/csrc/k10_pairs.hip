// K10 -- a GIVEN list of pairs under an edit-distance scorer: per from-string the candidates of a device-resident table are scored
// and re-ranked (pfz_pairs_rescore_topn).
//
// Extends the hot loop of EditDistance._calculate_edit_distance, reference polyfuzz/models/_distance.py:89-102 -- scorer(from, to)
// for every to-string, then the best -- restricted to the candidates a cheap matcher left (the top_n table of
// polyfuzz/models/_utils.py:82-91): blocking, then exact scoring of the few.  The scorers are K4's ratio, K9's Levenshtein / OSA
// and K8's Jaro / Jaro-Winkler; a pair's float64 score comes from the very functions those kernels call (k10_core.h ratio_of,
// k9_core.h, k8_core.h), so it has the bits the all-pairs kernels produce for that pair.
//
// Mapping to CDNA4
//   workgroup = ONE wave = one from-string at a time: its match table PM[symbol] (bit i: a[i] == symbol) lives in LDS, set for the
//     row's characters and cleared by the positions it set, as in K8 / K9.  A table per wave is what makes the waves independent:
//     a row's work is m candidates, far too little for four waves to share;
//   lane = one candidate, taken in chunks of 64 in the order they stand in the row.  The candidates are wherever the blocking put
//     them, not in the K4 plan's length-sorted groups, so a lane gathers its to-string's code units (1 or 4 bytes) from the raw
//     pfz_strings buffers and maps them through the plan's code unit -> symbol table (`lut`, cached on the to-handle); the lanes
//     of a chunk walk strings of different lengths and the wave waits for its longest;
//   the wave keeps the row's list with topn_wave.h -- one entry per lane, hence ntop <= 64 -- and writes the row's result itself:
//     (float64 score descending, to-index ascending), then (-1, 0.0).  The keys of a row are distinct (distinct indices), so the
//     order in which the chunks offer them does not show in the result.
// Every valid candidate is scored: no bound, no pruning -- the table is short.
// Register kernels: from-strings of up to 32 characters in 32-bit words, of up to 64 in 64-bit words; the to-string is a stream of
// any length for ratio / Levenshtein / OSA.  Jaro keeps a to-string's flag words in registers with compile-time indices (256
// positions, as K8); a row that holds a longer candidate is handed to the general kernel whole (a byte per row says so, written
// here, read there -- the table is never looked at on the host).
// General kernel: longer from-strings, those Jaro rows, and every row when the match table exceeds 60 KiB of LDS -- words and match
// table in global memory, any length, any alphabet, slow.
// Bound: integer VALU + LDS look-ups behind a dependent chain of gathered loads (code unit -> lut -> PM) per to-character
// (measured beside the all-pairs kernels).
// The score of one pair -- pair_score_reg, pair_score_general, the PAIR_* and MODE_* constants, the view of the two lists -- is
// pair_score.h's, which K16 (k16_pairs_join.hip) includes too.
#include "pair_score.h"
#include "topn_wave.h"

#include <algorithm>
#include <limits.h>

namespace pfz {

struct PairArgs : PairView {
    const int32_t *cand;       // [>= n_from][m] candidate to-indices; anything outside [0, n_to) is skipped
    int32_t m;
    const int32_t *rows;       // the from-rows of this launch (register kernels)
    int32_t n_rows;
    uint8_t *mode;             // [n_from] MODE_*: the general kernel serves the rows marked MODE_GENERAL
    int32_t ntop;
    int32_t *out_idx;          // [n_from][ntop]
    double *out_score;
};

// lane k of the chunk at c0: its candidate's to-index, or -1 (no candidate: beyond the row, an empty slot, outside the to-list)
__device__ inline int pair_candidate(const PairArgs &A, int64_t row, int c0)
{
    const int k = c0 + (int)(threadIdx.x & 63);
    const int j = k < A.m ? A.cand[row * A.m + k] : -1;
    return j >= 0 && (int64_t)j < A.n_to ? j : -1;
}

__device__ inline void pair_store_row(const PairArgs &A, int64_t row, const TopnList &l)
{
    const int lane = threadIdx.x & 63;
    if (lane < A.ntop) {
        A.out_idx[row * A.ntop + lane] = l.idx == INT_MAX ? -1 : l.idx;
        A.out_score[row * A.ntop + lane] = l.idx == INT_MAX ? 0.0 : l.score;
    }
}

// WORD: uint32_t (from-strings of <= 32 characters) or uint64_t (<= 64).  One wave per workgroup.
template <typename WORD, int FAMILY>
__global__ __launch_bounds__(64) void k10_pairs_kernel(PairArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    WORD *pm = (WORD *)smem_raw;
    const int lane = threadIdx.x;

    pm_reg_zero(A, pm, lane, 64);

    for (int r = blockIdx.x; r < A.n_rows; r += gridDim.x) {
        const int64_t row = A.rows[r];
        if constexpr (FAMILY == PAIR_JARO) {
            // a candidate of more than 256 characters: the row is the general kernel's
            bool longer = false;
            for (int c0 = 0; c0 < A.m; c0 += 64) {
                const int j = pair_candidate(A, row, c0);
                longer |= j >= 0 && A.b_off[j + 1] - A.b_off[j] > kPairsJaroRegLen;
            }
            if (__any(longer)) {
                if (lane == 0) A.mode[row] = MODE_GENERAL;
                continue;
            }
        }
        const int64_t a0 = A.a_off[row];
        const int la = (int)(A.a_off[row + 1] - a0);      // fits the WORD
        const int my_sym = pm_reg_set(A, pm, a0, la, lane);

        TopnList list = topn_empty();
        for (int c0 = 0; c0 < A.m; c0 += 64) {
            const int j = pair_candidate(A, row, c0);
            const int64_t b0 = j >= 0 ? A.b_off[j] : 0;
            const int lb = j >= 0 ? (int)(A.b_off[j + 1] - b0) : 0;
            double sc = 0.0;
            if (j >= 0) sc = pair_score_reg<WORD, FAMILY>(A, pm, la, b0, lb);
            topn_insert(list, A.ntop, j >= 0, sc, j);      // (all 64 lanes: the loop and its bounds are the wave's)
        }
        pair_store_row(A, row, list);
        pm_reg_clear(pm, my_sym);
    }
}

// The general case: any lengths, any alphabet.  One wave per workgroup and from-string; the match table of the from-string (WA
// words per symbol) and every lane's words -- s0 / s1 / s2[(block * WS + w) * 64 + lane], WS words each: V for ratio, VP / VN / D0
// for Levenshtein / OSA, the from-flags and the to-flags for Jaro -- are in global memory.  Serves the rows marked MODE_GENERAL.
__global__ __launch_bounds__(64) void k10_pairs_general_kernel(PairArgs A, int32_t WA, int32_t WS, uint64_t *__restrict__ pm_all,
                                                              uint64_t *__restrict__ s0_all, uint64_t *__restrict__ s1_all,
                                                              uint64_t *__restrict__ s2_all)
{
    const int lane = threadIdx.x;
    uint64_t *pm = pm_all + (int64_t)blockIdx.x * A.n_sym1 * WA;      // zero on entry, zero again after every row
    uint64_t *s0 = s0_all + (int64_t)blockIdx.x * WS * 64 + lane;     // s0[w * 64]: this lane's word w
    uint64_t *s1 = s1_all + (int64_t)blockIdx.x * WS * 64 + lane;
    uint64_t *s2 = s2_all + (int64_t)blockIdx.x * WS * 64 + lane;
    for (int64_t row = blockIdx.x; row < A.n_rows; row += gridDim.x) {
        if (A.mode[row] != MODE_GENERAL) continue;
        const int64_t a0 = A.a_off[row];
        const int la = (int)(A.a_off[row + 1] - a0);
        const int W = la > 0 ? (la + 63) / 64 : 1;                    // <= WA
        pm_global_set(A, pm, WA, a0, la, lane, 64);

        TopnList list = topn_empty();
        for (int c0 = 0; c0 < A.m; c0 += 64) {
            const int j = pair_candidate(A, row, c0);
            const int64_t b0 = j >= 0 ? A.b_off[j] : 0;
            const int lb = j >= 0 ? (int)(A.b_off[j + 1] - b0) : 0;
            double sc = 0.0;
            if (j >= 0) sc = pair_score_general(A, pm, s0, s1, s2, WA, W, la, b0, lb);
            topn_insert(list, A.ntop, j >= 0, sc, j);      // (all 64 lanes: the loop and its bounds are the wave's)
        }
        pair_store_row(A, row, list);
        pm_global_clear(A, pm, WA, a0, la, lane, 64);
    }
}

template <typename WORD> static void launch_pairs_reg(const PairArgs &A, dim3 grid, size_t lds, hipStream_t st)
{
    switch (A.scorer) {
    case PAIR_RATIO: hipLaunchKernelGGL((k10_pairs_kernel<WORD, PAIR_RATIO>), grid, dim3(64), lds, st, A); break;
    case PAIR_LEVENSHTEIN: hipLaunchKernelGGL((k10_pairs_kernel<WORD, PAIR_LEVENSHTEIN>), grid, dim3(64), lds, st, A); break;
    case PAIR_OSA: hipLaunchKernelGGL((k10_pairs_kernel<WORD, PAIR_OSA>), grid, dim3(64), lds, st, A); break;
    default: hipLaunchKernelGGL((k10_pairs_kernel<WORD, PAIR_JARO>), grid, dim3(64), lds, st, A); break;
    }
}

static int pairs_run(pfz_ctx *ctx, const pfz_strings *F, const pfz_strings *T, const pfz_topn *C, int32_t scorer, int32_t ntop,
                     int32_t *out_idx, double *out_score)
{
    const int64_t n_from = F->n;
    const size_t n_out = (size_t)n_from * (size_t)ntop;
    if (T->n == 0 || C->ntop == 0) {      // no candidate can be valid
        std::fill(out_idx, out_idx + n_out, -1);
        std::fill(out_score, out_score + n_out, 0.0);
        return PFZ_OK;
    }
    PFZ_HIP(hipSetDevice(ctx->device));
    if (T->n >= INT_MAX - 64 || F->n >= INT_MAX || T->max_len >= INT_MAX / 2 || F->max_len >= INT_MAX / 2) {
        set_error("pfz_pairs_rescore_topn: list or string too long");
        return PFZ_ERR_UNSUPPORTED;
    }
    const pfz_indel_plan *pl;
    PFZ_TRY(indel_plan_get(ctx, T, &pl));      // (its code unit -> symbol table; the packed groups are not read here)

    const bool jaro = scorer == PAIR_JARO || scorer == PAIR_JARO_WINKLER;
    const RowClasses rc = classify_rows(F, 0, n_from, lds_table_fits(pl));
    const std::vector<int32_t> (&rows_cls)[3] = rc.rows;
    std::vector<uint8_t> mode((size_t)n_from);      // MODE_* = the row's class
    for (int cls = 0; cls < 3; ++cls)
        for (int32_t i : rows_cls[cls]) mode[(size_t)i] = (uint8_t)cls;
    const int64_t n_general = (int64_t)rows_cls[MODE_GENERAL].size(), longest = rc.longest;
    // (the Jaro register kernels hand a row with a candidate of more than 256 characters on: only a to-list that has one)
    const bool general = n_general > 0 || (jaro && T->max_len > kPairsJaroRegLen);

    DevBuf d_mode, d_rows[2], d_oidx, d_oscore;
    PFZ_TRY(d_mode.upload(ctx, mode));
    PFZ_TRY(d_oidx.alloc(ctx, n_out * sizeof(int32_t)));
    PFZ_TRY(d_oscore.alloc(ctx, n_out * sizeof(double)));

    PairArgs A;
    static_cast<FromView &>(A) = from_view(F, pl);
    A.b_chars = T->chars;
    A.b_width = T->char_width;
    A.b_off = T->offsets;
    A.n_to = T->n;
    A.cand = C->idx;
    A.m = C->ntop;
    A.rows = nullptr;
    A.n_rows = 0;
    A.mode = d_mode.as<uint8_t>();
    A.scorer = scorer;
    A.ntop = ntop;
    A.out_idx = d_oidx.as<int32_t>();
    A.out_score = d_oscore.as<double>();

    // one wave per workgroup: up to 32 of them per compute unit, the rows dealt round robin
    const int64_t max_grid = (int64_t)ctx->prop.multiProcessorCount * 32;
    {
        ProfScope ps_all(ctx, "k10_pairs");
        for (int c = 0; c < 2; ++c) {
            if (rows_cls[c].empty()) continue;
            PFZ_TRY(d_rows[c].upload(ctx, rows_cls[c]));
            A.rows = d_rows[c].as<int32_t>();
            A.n_rows = (int32_t)rows_cls[c].size();
            const dim3 grid((unsigned)std::min<int64_t>(A.n_rows, max_grid));
            const size_t lds = (size_t)A.n_sym1 * (c == 1 ? sizeof(uint64_t) : sizeof(uint32_t));
            if (c == 0) launch_pairs_reg<uint32_t>(A, grid, lds, ctx->stream);
            else launch_pairs_reg<uint64_t>(A, grid, lds, ctx->stream);
            PFZ_HIP(hipGetLastError());
        }
        if (general) {
            A.rows = nullptr;
            A.n_rows = (int32_t)n_from;
            const int32_t WA = (int32_t)((longest + 63) / 64);
            const int32_t WS = jaro ? (int32_t)std::max<int64_t>(WA, (T->max_len + 63) / 64) : WA;
            int64_t grid = std::min<int64_t>(n_general > 0 && !jaro ? n_general : n_from, max_grid);
            PFZ_TRY(general_grid(&grid, A.n_sym1, WA, "pfz_pairs_rescore_topn", "a from-string", longest));
            ProfScope ps(ctx, "k10_pairs_general");
            GeneralBufs gb;
            PFZ_TRY(general_bufs_alloc(ctx, &gb, grid, A.n_sym1, WA, {WS, WS, WS}, 64));
            hipLaunchKernelGGL(k10_pairs_general_kernel, dim3((unsigned)grid), dim3(64), 0, ctx->stream, A, WA, WS, gb.pm.as<uint64_t>(),
                               gb.col[0].as<uint64_t>(), gb.col[1].as<uint64_t>(), gb.col[2].as<uint64_t>());
            PFZ_HIP(hipGetLastError());
        }
    }
    PFZ_TRY(copy_d2h(ctx, out_idx, d_oidx.p, n_out * sizeof(int32_t)));
    PFZ_TRY(copy_d2h(ctx, out_score, d_oscore.p, n_out * sizeof(double)));
    PFZ_HIP(hipStreamSynchronize(ctx->stream));
    return PFZ_OK;
}

}  // namespace pfz

using namespace pfz;

extern "C" {

int pfz_pairs_rescore_topn(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, const pfz_topn *candidates,
                           int32_t scorer, int32_t ntop, int32_t *out_idx, double *out_score)
{
    PFZ_REQUIRE(ctx && from_strings && to_strings && candidates, "pfz_pairs_rescore_topn: NULL argument");
    PFZ_REQUIRE(scorer >= PAIR_RATIO && scorer <= PAIR_JARO_WINKLER, "pfz_pairs_rescore_topn: scorer %d is outside 0 .. 4", scorer);
    PFZ_REQUIRE(ntop >= 1, "pfz_pairs_rescore_topn: ntop %d < 1", ntop);
    PFZ_REQUIRE(candidates->n_rows >= from_strings->n, "pfz_pairs_rescore_topn: the candidate table has %lld rows, the from-list %lld",
                (long long)candidates->n_rows, (long long)from_strings->n);
    if (ntop > kTopnMax) {
        set_error("pfz_pairs_rescore_topn: ntop %d exceeds the limit of %d (one list entry per lane of a wave)", ntop, kTopnMax);
        return PFZ_ERR_UNSUPPORTED;
    }
    if (candidates->ntop > kPairsMaxCandidates) {
        set_error("pfz_pairs_rescore_topn: %d candidates per row exceed the limit of %d", candidates->ntop, kPairsMaxCandidates);
        return PFZ_ERR_UNSUPPORTED;
    }
    if (from_strings->n == 0) return PFZ_OK;
    PFZ_REQUIRE(out_idx && out_score, "pfz_pairs_rescore_topn: NULL output");
    return pairs_run(ctx, from_strings, to_strings, candidates, scorer, ntop, out_idx, out_score);
}

}  // extern "C"
