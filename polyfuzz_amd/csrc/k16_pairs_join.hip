// K16 -- the threshold form of K10: the pairs of a device-resident candidate table with an edit-distance score >= t, as CSR
// (pfz_pairs_join, what BlockedEditDistance.join runs) or united into K12's forest where they are found (pfz_pairs_components,
// BlockedEditDistance.components).  Blocking, then exact scoring of the few, as K10 (k10_pairs.hip) -- with the comparison against
// t where K10 has topn_insert, a hit store or a unite where K10 keeps a list, and, in front, a symmetrisation of the table so that a
// self-join scores and reports every unordered pair once.  The scorers are Levenshtein / OSA / Jaro / Jaro-Winkler; a pair's float64
// score is computed by the functions K10 calls (pair_score.h), so it has K10's bits, which are the all-pairs kernels'.
//
// One walk, two sinks, all on the device:
//   keys    one 64-bit key per table cell (k16_core.h): row << 32 | col, in a self-join min << 32 | max; a cell that is no pair
//           (outside [0, n_to), a row's own index) gets all ones.  A thread per cell, no atomics;
//   sort    sort_codes_u64 (sort_u64.hip).  Equal keys -- a cell listed twice, the two directions of a self-join pair -- are now
//           adjacent, the keys that are no pair stand at the end, and the rest is in (row, to-index) order; row pointers over the
//           sorted keys by k11_unpack's scheme (k16_core.h pair_rows_fill);
//   score   K10's mapping: workgroup = ONE wave = one from-string at a time, its match table PM[symbol] in LDS, a lane per partner
//           in chunks of 64 -- over the row's POINTER RANGE, not over the table's width: after the symmetrisation a string that many
//           others list (a hub) has far more partners than the table has columns.  A lane whose key equals its predecessor's does
//           nothing.  Every distinct pair is scored to its end: no window, no abandon rule, no bound -- the table is short.  Row
//           classes are K10's: from-strings of <= 32 characters in 32-bit words, of <= 64 in 64-bit words; longer ones, a Jaro row
//           with a partner beyond 256 characters (a byte per row says so, written here, read there) and every row when the match
//           table exceeds 60 KiB take the general kernel: words and match table in global memory, slow;
//   sink    join: a hit lane writes its score and a flag at the pair's position in the sorted order; exclusive_scan_i32 over the
//           flags, then a compaction into CSR, which is already in (from, to) order -- no second sort, no atomics, and the order in
//           which the table's columns stood leaves no trace.  A total above the caller's capacity ends before the compaction.
//           components: a hit lane unites its two positions (k12_core.h uf_unite); K12's labelling pass and counts follow, nothing
//           else is stored.
// Call-scoped device memory: 8 B per table cell for the keys and 8 B (rounded up to a power of two of cells) for their sorted
// copy; the join adds 8 B per cell for the scores and 4 B for the flag the scan turns into the hit's position.
// Bound: K10's -- integer VALU + LDS look-ups behind a dependent chain of gathered loads per to-character; the sort in front is
// (log2 cells - 12)(log2 cells - 11) / 2 streaming passes of 16 B per key (the cells rounded up to a power of two).
#include "k12_core.h"
#include "k16_core.h"
#include "pair_score.h"

#include <algorithm>
#include <cmath>
#include <limits.h>

namespace pfz {

struct PairJoinArgs : PairView {
    const uint64_t *keys;      // [n_cells] sorted
    const int32_t *seg;        // [n_from + 1] row pointers over the keys
    const int32_t *rows;       // the from-rows of this launch (register kernels)
    int32_t n_rows;
    uint8_t *mode;             // [n_from] MODE_*: the general kernel serves the rows marked MODE_GENERAL
    double t;                  // min_similarity
    double *score;             // join: [n_cells] a hit's score, at its key's position
    int32_t *flag;             // join: [n_cells + 1] zero on entry, 1 where a hit is
    int32_t *parent;           // components: [n] K12's forest
    unsigned long long *counts;      // [2] distinct pairs scored, hits
};

// lane `lane` of the chunk at c0 of the row's range [c0, p1): the position of its key, or -1 (beyond the row, or a key that
// repeats its predecessor: that pair is another lane's)
__device__ inline int64_t pair_position(const PairJoinArgs &A, int64_t c0, int64_t p1)
{
    const int64_t p = c0 + (int)(threadIdx.x & 63);
    return p < p1 && pair_key_first(A.keys, p) ? p : -1;
}

// the two sinks: the score against the threshold (float64 against float64, equal is a hit), then the store or the unite
template <bool UNITE>
__device__ __forceinline__ void pair_sink(const PairJoinArgs &A, bool mine, double sc, int row, int j, int64_t p,
                                          unsigned long long &n_scored, unsigned long long &n_hits)
{
    const bool hit = mine && sc >= A.t;
    n_scored += mine;
    n_hits += hit;
    if constexpr (UNITE) {
        if (hit) uf_unite<UfDeviceOps>(A.parent, row, j);
    }
    else if (hit) {
        A.score[p] = sc;
        A.flag[p] = 1;
    }
}

// WORD: uint32_t (from-strings of <= 32 characters) or uint64_t (<= 64).  One wave per workgroup.
template <typename WORD, int FAMILY, bool UNITE>
__global__ __launch_bounds__(64) void k16_pairs_kernel(PairJoinArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    WORD *pm = (WORD *)smem_raw;
    const int lane = threadIdx.x;

    pm_reg_zero(A, pm, lane, 64);

    unsigned long long n_scored = 0, n_hits = 0;
    for (int r = blockIdx.x; r < A.n_rows; r += gridDim.x) {
        const int row = A.rows[r];
        const int64_t p0 = A.seg[row], p1 = A.seg[row + 1];
        if (p0 == p1) continue;                               // (the wave's: no pair has this row)
        if constexpr (FAMILY == PAIR_JARO) {
            // a partner of more than 256 characters: the row is the general kernel's
            bool longer = false;
            for (int64_t c0 = p0; c0 < p1; c0 += 64) {
                const int64_t p = pair_position(A, c0, p1);
                const int j = p >= 0 ? pair_key_to(A.keys[p]) : 0;
                longer |= p >= 0 && A.b_off[j + 1] - A.b_off[j] > kPairsJaroRegLen;
            }
            if (__any(longer)) {
                if (lane == 0) A.mode[row] = MODE_GENERAL;
                continue;
            }
        }
        const int64_t a0 = A.a_off[row];
        const int la = (int)(A.a_off[row + 1] - a0);      // fits the WORD
        const int my_sym = pm_reg_set(A, pm, a0, la, lane);

        for (int64_t c0 = p0; c0 < p1; c0 += 64) {        // the row's range: a hub has more than one chunk whatever m is
            const int64_t p = pair_position(A, c0, p1);
            const int j = p >= 0 ? pair_key_to(A.keys[p]) : 0;
            const int64_t b0 = p >= 0 ? A.b_off[j] : 0;
            const int lb = p >= 0 ? (int)(A.b_off[j + 1] - b0) : 0;
            double sc = 0.0;
            if (p >= 0) sc = pair_score_reg<WORD, FAMILY>(A, pm, la, b0, lb);
            pair_sink<UNITE>(A, p >= 0, sc, row, j, p, n_scored, n_hits);
        }
        pm_reg_clear(pm, my_sym);
    }
    wave_count(A.counts + 0, n_scored);
    wave_count(A.counts + 1, n_hits);
}

// The general case: any lengths, any alphabet.  One wave per workgroup and from-string; the match table of the from-string (WA
// words per symbol) and every lane's words -- s0 / s1 / s2[(block * WS + w) * 64 + lane], WS words each: VP / VN / D0 for
// Levenshtein / OSA, the from-flags and the to-flags for Jaro -- are in global memory.  Serves the rows marked MODE_GENERAL.
template <bool UNITE>
__global__ __launch_bounds__(64) void k16_pairs_general_kernel(PairJoinArgs A, int32_t WA, int32_t WS, uint64_t *__restrict__ pm_all,
                                                              uint64_t *__restrict__ s0_all, uint64_t *__restrict__ s1_all,
                                                              uint64_t *__restrict__ s2_all)
{
    const int lane = threadIdx.x;
    uint64_t *pm = pm_all + (int64_t)blockIdx.x * A.n_sym1 * WA;      // zero on entry, zero again after every row
    uint64_t *s0 = s0_all + (int64_t)blockIdx.x * WS * 64 + lane;     // s0[w * 64]: this lane's word w
    uint64_t *s1 = s1_all + (int64_t)blockIdx.x * WS * 64 + lane;
    uint64_t *s2 = s2_all + (int64_t)blockIdx.x * WS * 64 + lane;
    unsigned long long n_scored = 0, n_hits = 0;
    for (int64_t row = blockIdx.x; row < A.n_rows; row += gridDim.x) {
        if (A.mode[row] != MODE_GENERAL) continue;
        const int64_t p0 = A.seg[row], p1 = A.seg[row + 1];
        if (p0 == p1) continue;
        const int64_t a0 = A.a_off[row];
        const int la = (int)(A.a_off[row + 1] - a0);
        const int W = la > 0 ? (la + 63) / 64 : 1;                    // <= WA
        pm_global_set(A, pm, WA, a0, la, lane, 64);

        for (int64_t c0 = p0; c0 < p1; c0 += 64) {
            const int64_t p = pair_position(A, c0, p1);
            const int j = p >= 0 ? pair_key_to(A.keys[p]) : 0;
            const int64_t b0 = p >= 0 ? A.b_off[j] : 0;
            const int lb = p >= 0 ? (int)(A.b_off[j + 1] - b0) : 0;
            double sc = 0.0;
            if (p >= 0) sc = pair_score_general(A, pm, s0, s1, s2, WA, W, la, b0, lb);
            pair_sink<UNITE>(A, p >= 0, sc, (int)row, j, p, n_scored, n_hits);
        }
        pm_global_clear(A, pm, WA, a0, la, lane, 64);
    }
    wave_count(A.counts + 0, n_scored);
    wave_count(A.counts + 1, n_hits);
}

// a thread per table cell: its key (k16_core.h)
__global__ __launch_bounds__(256) void k16_keys(const int32_t *__restrict__ cand, int32_t m, int64_t n_cells, int64_t n_to, int32_t self,
                                                 uint64_t *__restrict__ keys)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < n_cells) keys[c] = pair_key(c / m, cand[c], n_to, self != 0);
}

// the row pointers over the sorted keys; seg[n_rows] = the cells that are a pair
__global__ __launch_bounds__(256) void k16_rows(const uint64_t *__restrict__ keys, int64_t n_cells, int64_t n_rows, int32_t *__restrict__ seg)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < n_cells) pair_rows_fill(keys, p, n_cells, n_rows, seg);
}

// behind the scan: pos[p] = the hits in front of position p, so position p holds a hit iff pos[p + 1] != pos[p], and a row's hits
// begin at pos[seg[row]]
__global__ __launch_bounds__(256) void k16_compact(const uint64_t *__restrict__ keys, const double *__restrict__ score,
                                                    const int32_t *__restrict__ pos, int64_t n_cells, const int32_t *__restrict__ seg,
                                                    int64_t n_rows, int64_t *__restrict__ row_ptr, int32_t *__restrict__ out_idx,
                                                    double *__restrict__ out_sim)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < n_cells) {
        const int32_t at = pos[p];
        if (pos[p + 1] != at) {
            out_idx[at] = pair_key_to(keys[p]);
            out_sim[at] = score[p];
        }
    }
    if (p <= n_rows) row_ptr[p] = pos[seg[p]];
}

template <typename WORD, bool UNITE> static void launch_pairs_reg(const PairJoinArgs &A, dim3 grid, size_t lds, hipStream_t st)
{
    switch (A.scorer) {
    case PAIR_LEVENSHTEIN: hipLaunchKernelGGL((k16_pairs_kernel<WORD, PAIR_LEVENSHTEIN, UNITE>), grid, dim3(64), lds, st, A); break;
    case PAIR_OSA: hipLaunchKernelGGL((k16_pairs_kernel<WORD, PAIR_OSA, UNITE>), grid, dim3(64), lds, st, A); break;
    default: hipLaunchKernelGGL((k16_pairs_kernel<WORD, PAIR_JARO, UNITE>), grid, dim3(64), lds, st, A); break;
    }
}

// what a walk leaves on the device for its caller's tail
struct PairWalk {
    DevBuf keys, sorted, seg, score, flag, state, mode, rows[2];
    int64_t n_cells = 0;
};

// The limits both entries share; `entry` is the name in the message.
static int pairs_limits(const char *entry, const pfz_strings *F, const pfz_strings *T, const pfz_topn *C)
{
    if (C->ntop > kPairsMaxCandidates) {
        set_error("%s: %d candidates per row exceed the limit of %d", entry, C->ntop, kPairsMaxCandidates);
        return PFZ_ERR_UNSUPPORTED;
    }
    if (F->n > (int64_t)INT_MAX || T->n > (int64_t)INT_MAX) {
        set_error("%s: a list of %lld strings exceeds the limit of %d (a key holds two 32-bit positions)", entry,
                  (long long)std::max(F->n, T->n), INT_MAX);
        return PFZ_ERR_UNSUPPORTED;
    }
    if (F->n * (int64_t)C->ntop > (int64_t)INT_MAX) {
        set_error("%s: %lld rows of %d candidates are more than the limit of %d table cells (the scan over them is 32-bit)", entry,
                  (long long)F->n, C->ntop, INT_MAX);
        return PFZ_ERR_UNSUPPORTED;
    }
    if (T->max_len >= INT_MAX / 2 || F->max_len >= INT_MAX / 2) {
        set_error("%s: a string of %lld characters exceeds the limit of %d", entry, (long long)std::max(F->max_len, T->max_len), INT_MAX / 2 - 1);
        return PFZ_ERR_UNSUPPORTED;
    }
    return PFZ_OK;
}

// keys, sort, row pointers and the scoring launches of one call (n_from, n_to, C->ntop > 0), everything enqueued on the context's
// stream; parent == NULL: the join's sink (w.score, w.flag), else the components' (the forest)
static int pairs_walk(pfz_ctx *ctx, const char *entry, const pfz_strings *F, const pfz_strings *T, bool self, const pfz_topn *C,
                      int32_t scorer, double t, int32_t *parent, PairWalk &w)
{
    const int64_t n_from = F->n, n_cells = n_from * (int64_t)C->ntop;
    w.n_cells = n_cells;
    const pfz_indel_plan *pl;
    PFZ_TRY(indel_plan_get(ctx, T, &pl));      // (its code unit -> symbol table; the packed groups are not read here)

    const bool jaro = scorer == PAIR_JARO || scorer == PAIR_JARO_WINKLER;
    const RowClasses rc = classify_rows(F, 0, n_from, lds_table_fits(pl));
    const std::vector<int32_t> (&rows_cls)[3] = rc.rows;
    std::vector<uint8_t> mode((size_t)n_from);      // MODE_* = the row's class
    for (int cls = 0; cls < 3; ++cls)
        for (int32_t i : rows_cls[cls]) mode[(size_t)i] = (uint8_t)cls;
    const int64_t n_general = (int64_t)rows_cls[MODE_GENERAL].size(), longest = rc.longest;
    // (the Jaro register kernels hand a row with a partner of more than 256 characters on: only a to-list that has one)
    const bool general = n_general > 0 || (jaro && T->max_len > kPairsJaroRegLen);

    PFZ_TRY(w.mode.upload(ctx, mode));
    PFZ_TRY(w.keys.alloc(ctx, (size_t)n_cells * sizeof(uint64_t)));
    PFZ_TRY(w.sorted.alloc(ctx, (size_t)sort_codes_capacity(n_cells) * sizeof(uint64_t)));
    PFZ_TRY(w.seg.alloc(ctx, (size_t)(n_from + 1) * sizeof(int32_t)));
    PFZ_TRY(w.state.alloc(ctx, 3 * sizeof(unsigned long long)));      // pairs scored, hits, (components) the roots
    PFZ_HIP(hipMemsetAsync(w.state.p, 0, 3 * sizeof(unsigned long long), ctx->stream));
    if (!parent) {
        PFZ_TRY(w.score.alloc(ctx, (size_t)n_cells * sizeof(double)));
        PFZ_TRY(w.flag.alloc(ctx, (size_t)(n_cells + 1) * sizeof(int32_t)));
        PFZ_HIP(hipMemsetAsync(w.flag.p, 0, (size_t)(n_cells + 1) * sizeof(int32_t), ctx->stream));
    }
    const unsigned cell_blocks = (unsigned)((n_cells + 255) / 256);
    {
        ProfScope ps(ctx, "k16_keys_sort");
        hipLaunchKernelGGL(k16_keys, dim3(cell_blocks), dim3(256), 0, ctx->stream, C->idx, C->ntop, n_cells, T->n, self ? 1 : 0,
                           w.keys.as<uint64_t>());
        PFZ_HIP(hipGetLastError());
        PFZ_TRY(sort_codes_u64(ctx, w.keys.as<uint64_t>(), w.sorted.as<uint64_t>(), n_cells));
        hipLaunchKernelGGL(k16_rows, dim3(cell_blocks), dim3(256), 0, ctx->stream, w.sorted.as<uint64_t>(), n_cells, n_from,
                           w.seg.as<int32_t>());
        PFZ_HIP(hipGetLastError());
    }

    PairJoinArgs A;
    static_cast<FromView &>(A) = from_view(F, pl);
    A.b_chars = T->chars;
    A.b_width = T->char_width;
    A.b_off = T->offsets;
    A.n_to = T->n;
    A.scorer = scorer;
    A.keys = w.sorted.as<uint64_t>();
    A.seg = w.seg.as<int32_t>();
    A.rows = nullptr;
    A.n_rows = 0;
    A.mode = w.mode.as<uint8_t>();
    A.t = t;
    A.score = w.score.as<double>();
    A.flag = w.flag.as<int32_t>();
    A.parent = parent;
    A.counts = w.state.as<unsigned long long>();

    // one wave per workgroup: up to 32 of them per compute unit, the rows dealt round robin
    const int64_t max_grid = (int64_t)ctx->prop.multiProcessorCount * 32;
    ProfScope ps_all(ctx, "k16_pairs_join");
    for (int c = 0; c < 2; ++c) {
        if (rows_cls[c].empty()) continue;
        PFZ_TRY(w.rows[c].upload(ctx, rows_cls[c]));
        A.rows = w.rows[c].as<int32_t>();
        A.n_rows = (int32_t)rows_cls[c].size();
        const dim3 grid((unsigned)std::min<int64_t>(A.n_rows, max_grid));
        const size_t lds = (size_t)A.n_sym1 * (c == 1 ? sizeof(uint64_t) : sizeof(uint32_t));
        if (c == 0 && parent) launch_pairs_reg<uint32_t, true>(A, grid, lds, ctx->stream);
        else if (c == 0) launch_pairs_reg<uint32_t, false>(A, grid, lds, ctx->stream);
        else if (parent) launch_pairs_reg<uint64_t, true>(A, grid, lds, ctx->stream);
        else launch_pairs_reg<uint64_t, false>(A, grid, lds, ctx->stream);
        PFZ_HIP(hipGetLastError());
    }
    if (general) {
        A.rows = nullptr;
        A.n_rows = (int32_t)n_from;
        const int32_t WA = (int32_t)((longest + 63) / 64);
        const int32_t WS = jaro ? (int32_t)std::max<int64_t>(WA, (T->max_len + 63) / 64) : WA;
        int64_t grid = std::min<int64_t>(n_general > 0 && !jaro ? n_general : n_from, max_grid);
        PFZ_TRY(general_grid(&grid, A.n_sym1, WA, entry, "a from-string", longest));
        ProfScope ps(ctx, "k16_pairs_join_general");
        GeneralBufs gb;
        PFZ_TRY(general_bufs_alloc(ctx, &gb, grid, A.n_sym1, WA, {WS, WS, WS}, 64));
        if (parent)
            hipLaunchKernelGGL(k16_pairs_general_kernel<true>, dim3((unsigned)grid), dim3(64), 0, ctx->stream, A, WA, WS, gb.pm.as<uint64_t>(),
                               gb.col[0].as<uint64_t>(), gb.col[1].as<uint64_t>(), gb.col[2].as<uint64_t>());
        else
            hipLaunchKernelGGL(k16_pairs_general_kernel<false>, dim3((unsigned)grid), dim3(64), 0, ctx->stream, A, WA, WS, gb.pm.as<uint64_t>(),
                               gb.col[0].as<uint64_t>(), gb.col[1].as<uint64_t>(), gb.col[2].as<uint64_t>());
        PFZ_HIP(hipGetLastError());
    }
    return PFZ_OK;
}

// out_counters of both entries: the table cells that are a pair, the distinct pairs scored, the hits
static int pairs_counters(pfz_ctx *ctx, const PairWalk &w, int64_t n_from, unsigned long long (&state)[3], int64_t *out_counters)
{
    int32_t cells = 0;
    PFZ_TRY(copy_d2h(ctx, &cells, w.seg.as<int32_t>() + n_from, sizeof(cells)));
    PFZ_TRY(copy_d2h(ctx, state, w.state.p, sizeof(state)));
    if (out_counters) {
        out_counters[0] = cells;
        out_counters[1] = (int64_t)state[0];
        out_counters[2] = (int64_t)state[1];
    }
    return PFZ_OK;
}

static int pairs_join_run(pfz_ctx *ctx, const pfz_strings *F, const pfz_strings *T, bool self, const pfz_topn *C, int32_t scorer,
                          double t, int64_t capacity, int64_t *out_row_ptr, int32_t *out_idx, double *out_sim, int64_t *out_total,
                          int64_t *out_counters)
{
    *out_total = 0;
    if (out_counters) out_counters[0] = out_counters[1] = out_counters[2] = 0;
    const int64_t n_from = F->n;
    if (n_from == 0 || T->n == 0 || C->ntop == 0) {      // no cell can be a pair
        for (int64_t r = 0; r <= n_from; ++r) out_row_ptr[r] = 0;
        return PFZ_OK;
    }
    PFZ_HIP(hipSetDevice(ctx->device));
    PairWalk w;
    PFZ_TRY(pairs_walk(ctx, "pfz_pairs_join", F, T, self, C, scorer, t, nullptr, w));
    {
        ProfScope ps(ctx, "k16_compact");
        PFZ_TRY(exclusive_scan_i32(ctx, w.flag.as<int32_t>(), w.n_cells));
    }
    int32_t total32 = 0;
    PFZ_TRY(copy_d2h(ctx, &total32, w.flag.as<int32_t>() + w.n_cells, sizeof(total32)));      // (waits for the kernels)
    unsigned long long state[3];
    PFZ_TRY(pairs_counters(ctx, w, n_from, state, out_counters));
    const int64_t total = total32;
    *out_total = total;
    if (total > capacity) return PFZ_OK;       // the caller's buffers stay as they are: it repeats the call with room for `total`
    if (total == 0) {
        for (int64_t r = 0; r <= n_from; ++r) out_row_ptr[r] = 0;
        return PFZ_OK;
    }
    DevBuf d_ptr, d_idx, d_sim;
    PFZ_TRY(d_ptr.alloc(ctx, (size_t)(n_from + 1) * sizeof(int64_t)));
    PFZ_TRY(d_idx.alloc(ctx, (size_t)total * sizeof(int32_t)));
    PFZ_TRY(d_sim.alloc(ctx, (size_t)total * sizeof(double)));
    {
        ProfScope ps(ctx, "k16_compact");
        const int64_t n_threads = std::max(w.n_cells, n_from + 1);
        hipLaunchKernelGGL(k16_compact, dim3((unsigned)((n_threads + 255) / 256)), dim3(256), 0, ctx->stream, w.sorted.as<uint64_t>(),
                           w.score.as<double>(), w.flag.as<int32_t>(), w.n_cells, w.seg.as<int32_t>(), n_from, d_ptr.as<int64_t>(),
                           d_idx.as<int32_t>(), d_sim.as<double>());
        PFZ_HIP(hipGetLastError());
    }
    PFZ_TRY(copy_d2h(ctx, out_row_ptr, d_ptr.p, (size_t)(n_from + 1) * sizeof(int64_t)));
    PFZ_TRY(copy_d2h(ctx, out_idx, d_idx.p, (size_t)total * sizeof(int32_t)));
    PFZ_TRY(copy_d2h(ctx, out_sim, d_sim.p, (size_t)total * sizeof(double)));
    PFZ_HIP(hipStreamSynchronize(ctx->stream));
    return PFZ_OK;
}

static int pairs_comp_run(pfz_ctx *ctx, const pfz_strings *F, const pfz_topn *C, int32_t scorer, double t, int32_t *out_label,
                          int64_t *out_pairs, int64_t *out_components, int64_t *out_counters)
{
    *out_pairs = *out_components = 0;
    if (out_counters) out_counters[0] = out_counters[1] = out_counters[2] = 0;
    const int64_t n = F->n;
    if (n == 0) return PFZ_OK;
    if (C->ntop == 0) {                        // no pair: every string is its own component
        for (int64_t i = 0; i < n; ++i) out_label[i] = (int32_t)i;
        *out_components = n;
        return PFZ_OK;
    }
    PFZ_HIP(hipSetDevice(ctx->device));
    DevBuf d_parent, d_label;
    PFZ_TRY(d_parent.alloc(ctx, (size_t)n * sizeof(int32_t)));
    PFZ_TRY(d_label.alloc(ctx, (size_t)n * sizeof(int32_t)));
    PFZ_TRY(k12_forest_begin(ctx, (int32_t)n, d_parent.as<int32_t>()));
    PairWalk w;
    PFZ_TRY(pairs_walk(ctx, "pfz_pairs_components", F, F, true, C, scorer, t, d_parent.as<int32_t>(), w));
    PFZ_TRY(k12_forest_flatten(ctx, d_parent.as<int32_t>(), (int32_t)n, d_label.as<int32_t>(), w.state.as<unsigned long long>() + 2));
    unsigned long long state[3];
    PFZ_TRY(pairs_counters(ctx, w, n, state, out_counters));
    PFZ_TRY(copy_d2h(ctx, out_label, d_label.p, (size_t)n * sizeof(int32_t)));
    PFZ_HIP(hipStreamSynchronize(ctx->stream));
    *out_pairs = (int64_t)state[1];
    *out_components = (int64_t)state[2];
    return PFZ_OK;
}

}  // namespace pfz

using namespace pfz;

// the checks both entries make of scorer and threshold
#define PFZ_PAIRS_REQUIRE_SCORER(entry)                                                                                              \
    PFZ_REQUIRE(scorer != PAIR_RATIO, entry ": scorer 0 (ratio) lives on 0 .. 100, where a min_similarity in [0, 1] is ambiguous: "  \
                                            "the join scorers are 1 (levenshtein), 2 (osa), 3 (jaro), 4 (jaro_winkler)");            \
    PFZ_REQUIRE(scorer >= PAIR_LEVENSHTEIN && scorer <= PAIR_JARO_WINKLER, entry ": scorer %d is outside 1 .. 4", scorer);           \
    PFZ_REQUIRE(!std::isnan(min_similarity) && min_similarity >= 0.0 && min_similarity <= 1.0,                                       \
                entry ": min_similarity %g is not a number in [0, 1]", min_similarity)

extern "C" {

int pfz_pairs_join(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, const pfz_topn *candidates,
                   int32_t scorer, double min_similarity, int64_t capacity, int64_t *out_row_ptr, int32_t *out_idx, double *out_sim,
                   int64_t *out_total, int64_t *out_counters)
{
    PFZ_REQUIRE(ctx && from_strings && candidates, "pfz_pairs_join: NULL argument");
    PFZ_PAIRS_REQUIRE_SCORER("pfz_pairs_join");
    PFZ_REQUIRE(capacity >= 0, "pfz_pairs_join: capacity %lld < 0", (long long)capacity);
    PFZ_REQUIRE(out_row_ptr && out_total, "pfz_pairs_join: NULL out_row_ptr / out_total");
    PFZ_REQUIRE(capacity == 0 || (out_idx && out_sim), "pfz_pairs_join: NULL output with capacity %lld", (long long)capacity);
    PFZ_REQUIRE(candidates->n_rows >= from_strings->n, "pfz_pairs_join: the candidate table has %lld rows, the from-list %lld",
                (long long)candidates->n_rows, (long long)from_strings->n);
    const bool self = to_strings == nullptr || to_strings == from_strings;
    const pfz_strings *T = self ? from_strings : to_strings;
    PFZ_TRY(pairs_limits("pfz_pairs_join", from_strings, T, candidates));
    return pairs_join_run(ctx, from_strings, T, self, candidates, scorer, min_similarity, capacity, out_row_ptr, out_idx, out_sim,
                          out_total, out_counters);
}

int pfz_pairs_components(pfz_ctx *ctx, const pfz_strings *strings, const pfz_topn *candidates, int32_t scorer, double min_similarity,
                         int32_t *out_label, int64_t *out_pairs, int64_t *out_components, int64_t *out_counters)
{
    PFZ_REQUIRE(ctx && strings && candidates, "pfz_pairs_components: NULL argument");
    PFZ_PAIRS_REQUIRE_SCORER("pfz_pairs_components");
    PFZ_REQUIRE(out_pairs && out_components, "pfz_pairs_components: NULL out_pairs / out_components");
    PFZ_REQUIRE(strings->n == 0 || out_label, "pfz_pairs_components: NULL out_label");
    PFZ_REQUIRE(candidates->n_rows >= strings->n, "pfz_pairs_components: the candidate table has %lld rows, the list %lld",
                (long long)candidates->n_rows, (long long)strings->n);
    PFZ_TRY(pairs_limits("pfz_pairs_components", strings, strings, candidates));
    return pairs_comp_run(ctx, strings, candidates, scorer, min_similarity, out_label, out_pairs, out_components, out_counters);
}

}  // extern "C"
