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
//           sorted keys by the joins' shared scheme (k16_core.h pair_rows_fill);
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
// K17 -- the key entries (pfz_pairs_join_keys, pfz_pairs_components_keys; BlockedEditDistance with blocking_similarity): the same
// walk over the sorted keys of a pfz_pairs handle, a TF-IDF threshold join that K15 left in HBM (pfz_cossim_join_dev), in place of a
// table's.  Everything behind "sorted keys in HBM" is ONE host function, pairs_walk_sorted, and one body per kernel
// (pairs_reg_walk, pairs_general_walk) that the table entries and the key entries both instantiate; the key entries skip k16_keys
// and the sort.  What is new is the deal: behind a threshold a row's range has no bound (1 860 partners where the mean row has a
// handful), so the key entries deal (row, slice) ITEMS of at most kPairSlice partners (k17_core.h) where the table entries deal
// rows: counted per row, scanned (exclusive_scan_i32) and filled on the device, in the order of the class-sorted rows, so that a
// class' items are one range [item_ptr[k_lo], item_ptr[k_hi]) whose ends the kernel reads itself -- the host never waits for them
// and sizes the grid by their bound.  An item sets up and clears its row's match table itself.  Jaro's hand-over of a partner
// beyond 256 characters is per ITEM (a byte per item, the row's class on entry): two waves may own slices of one row, and a per-row
// mark would make the general kernel rescore what the other wave has scored.  The table entries keep whole rows and their kernels'
// names (k16_pairs_kernel, k16_pairs_general_kernel); the item forms are k17_items_kernel and k17_items_general_kernel.
// Call-scoped device memory: 8 B per table cell for the keys and 8 B (rounded up to a power of two of cells) for their sorted
// copy; the join adds 8 B per cell for the scores and 4 B for the flag the scan turns into the hit's position.
// Bound: K10's -- integer VALU + LDS look-ups behind a dependent chain of gathered loads per to-character; the sort in front is
// (log2 cells - 12)(log2 cells - 11) / 2 streaming passes of 16 B per key (the cells rounded up to a power of two).
#include "k12_core.h"
#include "k16_core.h"
#include "k17_core.h"
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
    // the key entries (K17): items instead of rows
    const PairItem *items;     // [item_ptr[n_from]] the (row, slice) items, in the order of the class-sorted rows
    const int32_t *item_ptr;   // [n_from + 1] the first item of the k-th class-sorted row
    int32_t k_lo, k_hi;        // this launch serves the items of the class-sorted rows [k_lo, k_hi)
    uint8_t *item_mode;        // [items] MODE_*: the general kernel serves the items marked MODE_GENERAL
};

// lane `lane` of the chunk at c0 of the range [c0, p1): the position of its key, or -1 (beyond the range, or a key that
// repeats its predecessor: that pair is another lane's)
__device__ inline int64_t pair_position(const PairJoinArgs &A, int64_t c0, int64_t p1)
{
    const int64_t p = c0 + (int)(threadIdx.x & 63);
    return p < p1 && pair_key_first(A.keys, p) ? p : -1;
}

// What a wave serves at a time.  The table entries: a from-row with its whole pointer range (rows[r], or row r itself) and the
// row's byte of `mode`.  The key entries (ITEMS): item r of the launch -- a slice of a row's range (k17_core.h) -- and the item's
// own byte: two waves may own slices of one row, so what one of them decides about its slice is the slice's alone.
struct PairWork {
    int32_t row;
    int64_t p0, p1;
    uint8_t *mode;
};

template <bool ITEMS> __device__ __forceinline__ int64_t pair_work_count(const PairJoinArgs &A)
{
    if constexpr (ITEMS) return A.item_ptr[A.k_hi] - A.item_ptr[A.k_lo];
    else return A.n_rows;
}

template <bool ITEMS> __device__ __forceinline__ PairWork pair_work(const PairJoinArgs &A, int64_t r, const int32_t *rows)
{
    if constexpr (ITEMS) {
        const int64_t it = A.item_ptr[A.k_lo] + r;
        const PairItem item = A.items[it];
        return PairWork{item.row, item.p0, item.p1, A.item_mode + it};
    }
    else {
        const int32_t row = rows ? rows[r] : (int32_t)r;
        return PairWork{row, A.seg[row], A.seg[row + 1], A.mode + row};
    }
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

// WORD: uint32_t (from-strings of <= 32 characters) or uint64_t (<= 64).  One wave per workgroup; pm: the wave's match table in LDS.
template <typename WORD, int FAMILY, bool UNITE, bool ITEMS>
__device__ __forceinline__ void pairs_reg_walk(const PairJoinArgs &A, WORD *pm)
{
    const int lane = threadIdx.x;

    pm_reg_zero(A, pm, lane, 64);

    unsigned long long n_scored = 0, n_hits = 0;
    const int64_t n_work = pair_work_count<ITEMS>(A);
    for (int64_t r = blockIdx.x; r < n_work; r += gridDim.x) {
        const PairWork w = pair_work<ITEMS>(A, r, A.rows);
        const int row = w.row;
        const int64_t p0 = w.p0, p1 = w.p1;
        if (p0 == p1) continue;                               // (the wave's: no pair has this row)
        if constexpr (FAMILY == PAIR_JARO) {
            // a partner of more than 256 characters: the row (the item) is the general kernel's
            bool longer = false;
            for (int64_t c0 = p0; c0 < p1; c0 += 64) {
                const int64_t p = pair_position(A, c0, p1);
                const int j = p >= 0 ? pair_key_to(A.keys[p]) : 0;
                longer |= p >= 0 && A.b_off[j + 1] - A.b_off[j] > kPairsJaroRegLen;
            }
            if (__any(longer)) {
                if (lane == 0) *w.mode = MODE_GENERAL;
                continue;
            }
        }
        const int64_t a0 = A.a_off[row];
        const int la = (int)(A.a_off[row + 1] - a0);      // fits the WORD
        const int my_sym = pm_reg_set(A, pm, a0, la, lane);

        for (int64_t c0 = p0; c0 < p1; c0 += 64) {        // the range: a hub has more than one chunk whatever m is
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

// the table entries' kernel: a from-row at a time
template <typename WORD, int FAMILY, bool UNITE>
__global__ __launch_bounds__(64) void k16_pairs_kernel(PairJoinArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    pairs_reg_walk<WORD, FAMILY, UNITE, false>(A, (WORD *)smem_raw);
}

// the key entries' kernel (K17): an item at a time
template <typename WORD, int FAMILY, bool UNITE>
__global__ __launch_bounds__(64) void k17_items_kernel(PairJoinArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    pairs_reg_walk<WORD, FAMILY, UNITE, true>(A, (WORD *)smem_raw);
}

// The general case: any lengths, any alphabet.  One wave per workgroup and from-string; the match table of the from-string (WA
// words per symbol) and every lane's words -- s0 / s1 / s2[(block * WS + w) * 64 + lane], WS words each: VP / VN / D0 for
// Levenshtein / OSA, the from-flags and the to-flags for Jaro -- are in global memory.  Serves the rows (items) marked MODE_GENERAL.
template <bool UNITE, bool ITEMS>
__device__ __forceinline__ void pairs_general_walk(const PairJoinArgs &A, int32_t WA, int32_t WS, uint64_t *__restrict__ pm_all,
                                                   uint64_t *__restrict__ s0_all, uint64_t *__restrict__ s1_all,
                                                   uint64_t *__restrict__ s2_all)
{
    const int lane = threadIdx.x;
    uint64_t *pm = pm_all + (int64_t)blockIdx.x * A.n_sym1 * WA;      // zero on entry, zero again after every row
    uint64_t *s0 = s0_all + (int64_t)blockIdx.x * WS * 64 + lane;     // s0[w * 64]: this lane's word w
    uint64_t *s1 = s1_all + (int64_t)blockIdx.x * WS * 64 + lane;
    uint64_t *s2 = s2_all + (int64_t)blockIdx.x * WS * 64 + lane;
    unsigned long long n_scored = 0, n_hits = 0;
    const int64_t n_work = pair_work_count<ITEMS>(A);
    for (int64_t r = blockIdx.x; r < n_work; r += gridDim.x) {
        const PairWork w = pair_work<ITEMS>(A, r, nullptr);
        if (*w.mode != MODE_GENERAL) continue;
        const int row = w.row;
        const int64_t p0 = w.p0, p1 = w.p1;
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
            pair_sink<UNITE>(A, p >= 0, sc, row, j, p, n_scored, n_hits);
        }
        pm_global_clear(A, pm, WA, a0, la, lane, 64);
    }
    wave_count(A.counts + 0, n_scored);
    wave_count(A.counts + 1, n_hits);
}

template <bool UNITE>
__global__ __launch_bounds__(64) void k16_pairs_general_kernel(PairJoinArgs A, int32_t WA, int32_t WS, uint64_t *__restrict__ pm_all,
                                                              uint64_t *__restrict__ s0_all, uint64_t *__restrict__ s1_all,
                                                              uint64_t *__restrict__ s2_all)
{
    pairs_general_walk<UNITE, false>(A, WA, WS, pm_all, s0_all, s1_all, s2_all);
}

template <bool UNITE>
__global__ __launch_bounds__(64) void k17_items_general_kernel(PairJoinArgs A, int32_t WA, int32_t WS, uint64_t *__restrict__ pm_all,
                                                              uint64_t *__restrict__ s0_all, uint64_t *__restrict__ s1_all,
                                                              uint64_t *__restrict__ s2_all)
{
    pairs_general_walk<UNITE, true>(A, WA, WS, pm_all, s0_all, s1_all, s2_all);
}

// K17's items, built on the device from the row pointers: a thread per class-sorted row k (row order[k]) -- its number of items
// (k17_core.h), then, behind the scan, the items themselves, each with its row's class as its byte
__global__ __launch_bounds__(256) void k17_item_count(const int32_t *__restrict__ order, const int32_t *__restrict__ seg, int64_t n_rows,
                                                       int32_t *__restrict__ item_ptr)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n_rows) item_ptr[k] = pair_item_count((int64_t)seg[order[k] + 1] - seg[order[k]], kPairSlice);
}

__global__ __launch_bounds__(256) void k17_item_fill(const int32_t *__restrict__ order, const int32_t *__restrict__ seg,
                                                      const uint8_t *__restrict__ mode, int64_t n_rows, const int32_t *__restrict__ item_ptr,
                                                      PairItem *__restrict__ items, uint8_t *__restrict__ item_mode)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_rows) return;
    const int32_t row = order[k], first = item_ptr[k], n = item_ptr[k + 1] - first;
    for (int32_t i = 0; i < n; ++i) {
        items[first + i] = pair_item_slice(row, seg[row], seg[row + 1], i, kPairSlice);
        item_mode[first + i] = mode[row];
    }
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

template <typename WORD, bool UNITE, bool ITEMS> static void launch_pairs_reg(const PairJoinArgs &A, dim3 grid, size_t lds, hipStream_t st)
{
#define PFZ_PAIRS_REG(FAMILY)                                                                                                       \
    if constexpr (ITEMS) hipLaunchKernelGGL((k17_items_kernel<WORD, FAMILY, UNITE>), grid, dim3(64), lds, st, A);                    \
    else hipLaunchKernelGGL((k16_pairs_kernel<WORD, FAMILY, UNITE>), grid, dim3(64), lds, st, A)
    switch (A.scorer) {
    case PAIR_LEVENSHTEIN: PFZ_PAIRS_REG(PAIR_LEVENSHTEIN); break;
    case PAIR_OSA: PFZ_PAIRS_REG(PAIR_OSA); break;
    default: PFZ_PAIRS_REG(PAIR_JARO); break;
    }
#undef PFZ_PAIRS_REG
}

template <bool ITEMS> static void launch_pairs_reg_class(int cls, bool unite, const PairJoinArgs &A, dim3 grid, size_t lds, hipStream_t st)
{
    if (cls == 0 && unite) launch_pairs_reg<uint32_t, true, ITEMS>(A, grid, lds, st);
    else if (cls == 0) launch_pairs_reg<uint32_t, false, ITEMS>(A, grid, lds, st);
    else if (unite) launch_pairs_reg<uint64_t, true, ITEMS>(A, grid, lds, st);
    else launch_pairs_reg<uint64_t, false, ITEMS>(A, grid, lds, st);
}

// what a walk leaves on the device for its caller's tail
struct PairWalk {
    DevBuf keys, sorted, seg, score, flag, state, mode, rows[2], order, item_ptr, items, item_mode;
    const uint64_t *skeys = nullptr;      // the sorted keys: `sorted`, or a pfz_pairs handle's
    int64_t n_cells = 0;
    const pfz_indel_plan *pl = nullptr;   // the to-side's plan and the from-rows' classes (pairs_walk_begin)
    RowClasses rc;
    bool items_dealt = false;             // item_ptr[n_from] = the items
};

// The limits both entries share; `entry` is the name in the message.  ntop: the table's width (the key entries: 0)
static int pairs_limits(const char *entry, const pfz_strings *F, const pfz_strings *T, int32_t ntop)
{
    if (ntop > kPairsMaxCandidates) {
        set_error("%s: %d candidates per row exceed the limit of %d", entry, ntop, kPairsMaxCandidates);
        return PFZ_ERR_UNSUPPORTED;
    }
    if (F->n > (int64_t)INT_MAX || T->n > (int64_t)INT_MAX) {
        set_error("%s: a list of %lld strings exceeds the limit of %d (a key holds two 32-bit positions)", entry,
                  (long long)std::max(F->n, T->n), INT_MAX);
        return PFZ_ERR_UNSUPPORTED;
    }
    if (F->n * (int64_t)ntop > (int64_t)INT_MAX) {
        set_error("%s: %lld rows of %d candidates are more than the limit of %d table cells (the scan over them is 32-bit)", entry,
                  (long long)F->n, ntop, INT_MAX);
        return PFZ_ERR_UNSUPPORTED;
    }
    if (T->max_len >= INT_MAX / 2 || F->max_len >= INT_MAX / 2) {
        set_error("%s: a string of %lld characters exceeds the limit of %d", entry, (long long)std::max(F->max_len, T->max_len), INT_MAX / 2 - 1);
        return PFZ_ERR_UNSUPPORTED;
    }
    return PFZ_OK;
}

// What a walk needs before any key is looked at: the to-side's plan, the from-rows' classes and their bytes on the device, the
// state words.  (In front of the table entries' sort, so that the uploads do not queue up behind it.)
static int pairs_walk_begin(pfz_ctx *ctx, const pfz_strings *F, const pfz_strings *T, PairWalk &w)
{
    const int64_t n_from = F->n;
    PFZ_TRY(indel_plan_get(ctx, T, &w.pl));      // (its code unit -> symbol table; the packed groups are not read here)
    w.rc = classify_rows(F, 0, n_from, lds_table_fits(w.pl));
    std::vector<uint8_t> mode((size_t)n_from);      // MODE_* = the row's class
    for (int cls = 0; cls < 3; ++cls)
        for (int32_t i : w.rc.rows[cls]) mode[(size_t)i] = (uint8_t)cls;
    PFZ_TRY(w.mode.upload(ctx, mode));
    return PFZ_OK;
}

// Everything behind "sorted keys in HBM", for the table entries and the key entries alike: the row pointers over the n_cells >= 1
// keys at `skeys` and the scoring launches of one call, enqueued on the context's stream; parent == NULL: the join's sink
// (w.score, w.flag), else the components' (the forest).  items: the key entries' deal -- (row, slice) items of at most kPairSlice
// partners, built here on the device, in place of whole rows.  seg, state, score and flag are allocated (and cleared) by the caller.
static int pairs_walk_sorted(pfz_ctx *ctx, const char *entry, const pfz_strings *F, const pfz_strings *T, const uint64_t *skeys,
                             int64_t n_cells, bool items, int32_t scorer, double t, int32_t *parent, PairWalk &w)
{
    const int64_t n_from = F->n;
    w.skeys = skeys;
    const pfz_indel_plan *pl = w.pl;
    const bool jaro = scorer == PAIR_JARO || scorer == PAIR_JARO_WINKLER;
    const std::vector<int32_t> (&rows_cls)[3] = w.rc.rows;
    const int64_t n_general = (int64_t)rows_cls[MODE_GENERAL].size(), longest = w.rc.longest;
    // (the Jaro register kernels hand a row with a partner of more than 256 characters on: only a to-list that has one)
    const bool handover = jaro && T->max_len > kPairsJaroRegLen;
    const bool general = n_general > 0 || handover;
    {
        ProfScope ps(ctx, "k16_keys_sort");
        hipLaunchKernelGGL(k16_rows, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, ctx->stream, skeys, n_cells, n_from,
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
    A.keys = skeys;
    A.seg = w.seg.as<int32_t>();
    A.rows = nullptr;
    A.n_rows = 0;
    A.mode = w.mode.as<uint8_t>();
    A.t = t;
    A.score = w.score.as<double>();
    A.flag = w.flag.as<int32_t>();
    A.parent = parent;
    A.counts = w.state.as<unsigned long long>();
    A.items = nullptr;
    A.item_ptr = nullptr;
    A.k_lo = A.k_hi = 0;
    A.item_mode = nullptr;

    // the class-sorted rows [bound[c], bound[c + 1]) are class c's
    int64_t bound[4] = {0, 0, 0, 0};
    for (int c = 0; c < 3; ++c) bound[c + 1] = bound[c] + (int64_t)rows_cls[c].size();
    if (items) {
        ProfScope ps(ctx, "k17_items");
        std::vector<int32_t> order;
        order.reserve((size_t)n_from);
        for (int c = 0; c < 3; ++c) order.insert(order.end(), rows_cls[c].begin(), rows_cls[c].end());
        const int64_t room = pair_item_bound(n_from, n_cells, kPairSlice);
        PFZ_TRY(w.order.upload(ctx, order));
        PFZ_TRY(w.item_ptr.alloc(ctx, (size_t)(n_from + 1) * sizeof(int32_t)));
        PFZ_TRY(w.items.alloc(ctx, (size_t)room * sizeof(PairItem)));
        PFZ_TRY(w.item_mode.alloc(ctx, (size_t)room));
        const unsigned row_blocks = (unsigned)((n_from + 255) / 256);
        hipLaunchKernelGGL(k17_item_count, dim3(row_blocks), dim3(256), 0, ctx->stream, w.order.as<int32_t>(), w.seg.as<int32_t>(), n_from,
                           w.item_ptr.as<int32_t>());
        PFZ_HIP(hipGetLastError());
        PFZ_TRY(exclusive_scan_i32(ctx, w.item_ptr.as<int32_t>(), n_from));
        hipLaunchKernelGGL(k17_item_fill, dim3(row_blocks), dim3(256), 0, ctx->stream, w.order.as<int32_t>(), w.seg.as<int32_t>(),
                           w.mode.as<uint8_t>(), n_from, w.item_ptr.as<int32_t>(), w.items.as<PairItem>(), w.item_mode.as<uint8_t>());
        PFZ_HIP(hipGetLastError());
        A.items = w.items.as<PairItem>();
        A.item_ptr = w.item_ptr.as<int32_t>();
        A.item_mode = w.item_mode.as<uint8_t>();
        w.items_dealt = true;
    }

    // one wave per workgroup: up to 32 of them per compute unit, the rows (items) dealt round robin.  The number of a class'
    // items is known on the device alone: the grid is sized by its bound (k17_core.h)
    const int64_t max_grid = (int64_t)ctx->prop.multiProcessorCount * 32;
    ProfScope ps_all(ctx, "k16_pairs_join");
    for (int c = 0; c < 2; ++c) {
        if (rows_cls[c].empty()) continue;
        int64_t n_work = (int64_t)rows_cls[c].size();
        if (items) {
            A.k_lo = (int32_t)bound[c];
            A.k_hi = (int32_t)bound[c + 1];
            n_work = pair_item_bound(n_work, n_cells, kPairSlice);
        }
        else {
            PFZ_TRY(w.rows[c].upload(ctx, rows_cls[c]));
            A.rows = w.rows[c].as<int32_t>();
            A.n_rows = (int32_t)rows_cls[c].size();
        }
        const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(n_work, max_grid)));
        const size_t lds = (size_t)A.n_sym1 * (c == 1 ? sizeof(uint64_t) : sizeof(uint32_t));
        if (items) launch_pairs_reg_class<true>(c, parent != nullptr, A, grid, lds, ctx->stream);
        else launch_pairs_reg_class<false>(c, parent != nullptr, A, grid, lds, ctx->stream);
        PFZ_HIP(hipGetLastError());
    }
    if (general) {
        A.rows = nullptr;
        A.n_rows = (int32_t)n_from;
        // a Jaro call's hand-over may come from any row: the whole list; otherwise the general class alone
        int64_t n_work = n_general > 0 && !jaro ? n_general : n_from;
        if (items) {
            A.k_lo = handover ? 0 : (int32_t)bound[2];
            A.k_hi = (int32_t)bound[3];
            n_work = std::max<int64_t>(1, pair_item_bound(A.k_hi - A.k_lo, n_cells, kPairSlice));
        }
        const int32_t WA = (int32_t)((longest + 63) / 64);
        const int32_t WS = jaro ? (int32_t)std::max<int64_t>(WA, (T->max_len + 63) / 64) : WA;
        int64_t grid = std::min<int64_t>(n_work, max_grid);
        PFZ_TRY(general_grid(&grid, A.n_sym1, WA, entry, "a from-string", longest));
        ProfScope ps(ctx, "k16_pairs_join_general");
        GeneralBufs gb;
        PFZ_TRY(general_bufs_alloc(ctx, &gb, grid, A.n_sym1, WA, {WS, WS, WS}, 64));
#define PFZ_PAIRS_GENERAL(KERNEL)                                                                                                   \
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)grid), dim3(64), 0, ctx->stream, A, WA, WS, gb.pm.as<uint64_t>(), gb.col[0].as<uint64_t>(), \
                       gb.col[1].as<uint64_t>(), gb.col[2].as<uint64_t>())
        if (items && parent) PFZ_PAIRS_GENERAL(k17_items_general_kernel<true>);
        else if (items) PFZ_PAIRS_GENERAL(k17_items_general_kernel<false>);
        else if (parent) PFZ_PAIRS_GENERAL(k16_pairs_general_kernel<true>);
        else PFZ_PAIRS_GENERAL(k16_pairs_general_kernel<false>);
#undef PFZ_PAIRS_GENERAL
        PFZ_HIP(hipGetLastError());
    }
    return PFZ_OK;
}

// the buffers every walk over n_cells keys has: row pointers, state words and, for the join's sink, scores and flags
static int pairs_walk_alloc(pfz_ctx *ctx, int64_t n_from, int64_t n_cells, bool join, PairWalk &w)
{
    w.n_cells = n_cells;
    PFZ_TRY(w.seg.alloc(ctx, (size_t)(n_from + 1) * sizeof(int32_t)));
    PFZ_TRY(w.state.alloc(ctx, 3 * sizeof(unsigned long long)));      // pairs scored, hits, (components) the roots
    PFZ_HIP(hipMemsetAsync(w.state.p, 0, 3 * sizeof(unsigned long long), ctx->stream));
    if (join) {
        PFZ_TRY(w.score.alloc(ctx, (size_t)n_cells * sizeof(double)));
        PFZ_TRY(w.flag.alloc(ctx, (size_t)(n_cells + 1) * sizeof(int32_t)));
        PFZ_HIP(hipMemsetAsync(w.flag.p, 0, (size_t)(n_cells + 1) * sizeof(int32_t), ctx->stream));
    }
    return PFZ_OK;
}

// The table entries (n_from, n_to, C->ntop > 0): one key per table cell and their sort in front of pairs_walk_sorted, whole rows
static int pairs_walk(pfz_ctx *ctx, const char *entry, const pfz_strings *F, const pfz_strings *T, bool self, const pfz_topn *C,
                      int32_t scorer, double t, int32_t *parent, PairWalk &w)
{
    const int64_t n_cells = F->n * (int64_t)C->ntop;
    PFZ_TRY(pairs_walk_begin(ctx, F, T, w));
    PFZ_TRY(w.keys.alloc(ctx, (size_t)n_cells * sizeof(uint64_t)));
    PFZ_TRY(w.sorted.alloc(ctx, (size_t)sort_codes_capacity(n_cells) * sizeof(uint64_t)));
    PFZ_TRY(pairs_walk_alloc(ctx, F->n, n_cells, parent == nullptr, w));
    {
        ProfScope ps(ctx, "k16_keys_sort");
        hipLaunchKernelGGL(k16_keys, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, ctx->stream, C->idx, C->ntop, n_cells, T->n,
                           self ? 1 : 0, w.keys.as<uint64_t>());
        PFZ_HIP(hipGetLastError());
        PFZ_TRY(sort_codes_u64(ctx, w.keys.as<uint64_t>(), w.sorted.as<uint64_t>(), n_cells));
    }
    return pairs_walk_sorted(ctx, entry, F, T, w.sorted.as<uint64_t>(), n_cells, false, scorer, t, parent, w);
}

// The key entries: the keys of a pair list as they lie, dealt as items
static int pairs_walk_keys(pfz_ctx *ctx, const char *entry, const pfz_strings *F, const pfz_strings *T, const pfz_pairs *K,
                           int32_t scorer, double t, int32_t *parent, PairWalk &w)
{
    PFZ_TRY(pairs_walk_begin(ctx, F, T, w));
    PFZ_TRY(pairs_walk_alloc(ctx, F->n, K->count, parent == nullptr, w));
    return pairs_walk_sorted(ctx, entry, F, T, K->keys, K->count, true, scorer, t, parent, w);
}

// where a call's candidate pairs come from: a candidate table (K16), or the sorted keys of a pair list (K17)
struct PairSource {
    const pfz_topn *table = nullptr;
    const pfz_pairs *pairs = nullptr;
    bool empty() const { return table ? table->ntop == 0 : pairs->count == 0; }
    int n_counters() const { return table ? 3 : 4; }
    int walk(pfz_ctx *ctx, const char *entry, const pfz_strings *F, const pfz_strings *T, bool self, int32_t scorer, double t,
             int32_t *parent, PairWalk &w) const
    {
        if (table) return pairs_walk(ctx, entry, F, T, self, table, scorer, t, parent, w);
        return pairs_walk_keys(ctx, entry, F, T, pairs, scorer, t, parent, w);
    }
};

// out_counters of the entries: the table cells (the keys) that are a pair, the distinct pairs scored, the hits; the key entries
// add the work items
static int pairs_counters(pfz_ctx *ctx, const PairWalk &w, int64_t n_from, unsigned long long (&state)[3], int64_t *out_counters)
{
    int32_t cells = 0, items = 0;
    PFZ_TRY(copy_d2h(ctx, &cells, w.seg.as<int32_t>() + n_from, sizeof(cells)));
    if (w.items_dealt) PFZ_TRY(copy_d2h(ctx, &items, w.item_ptr.as<int32_t>() + n_from, sizeof(items)));
    PFZ_TRY(copy_d2h(ctx, state, w.state.p, sizeof(state)));
    if (out_counters) {
        out_counters[0] = cells;
        out_counters[1] = (int64_t)state[0];
        out_counters[2] = (int64_t)state[1];
        if (w.items_dealt) out_counters[3] = items;
    }
    return PFZ_OK;
}

static int pairs_join_run(pfz_ctx *ctx, const char *entry, const pfz_strings *F, const pfz_strings *T, bool self, const PairSource &src,
                          int32_t scorer, double t, int64_t capacity, int64_t *out_row_ptr, int32_t *out_idx, double *out_sim,
                          int64_t *out_total, int64_t *out_counters)
{
    *out_total = 0;
    if (out_counters)
        for (int c = 0; c < src.n_counters(); ++c) out_counters[c] = 0;
    const int64_t n_from = F->n;
    if (n_from == 0 || T->n == 0 || src.empty()) {      // no cell can be a pair
        for (int64_t r = 0; r <= n_from; ++r) out_row_ptr[r] = 0;
        return PFZ_OK;
    }
    PFZ_HIP(hipSetDevice(ctx->device));
    PairWalk w;
    PFZ_TRY(src.walk(ctx, entry, F, T, self, scorer, t, nullptr, w));
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
        hipLaunchKernelGGL(k16_compact, dim3((unsigned)((n_threads + 255) / 256)), dim3(256), 0, ctx->stream, w.skeys,
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

static int pairs_comp_run(pfz_ctx *ctx, const char *entry, const pfz_strings *F, const PairSource &src, int32_t scorer, double t,
                          int32_t *out_label, int64_t *out_pairs, int64_t *out_components, int64_t *out_counters)
{
    *out_pairs = *out_components = 0;
    if (out_counters)
        for (int c = 0; c < src.n_counters(); ++c) out_counters[c] = 0;
    const int64_t n = F->n;
    if (n == 0) return PFZ_OK;
    if (src.empty()) {                         // no pair: every string is its own component
        for (int64_t i = 0; i < n; ++i) out_label[i] = (int32_t)i;
        *out_components = n;
        return PFZ_OK;
    }
    PFZ_HIP(hipSetDevice(ctx->device));
    ForestRun forest;
    PFZ_TRY(forest.alloc(ctx, n));
    PFZ_TRY(forest.begin(ctx));
    PairWalk w;
    PFZ_TRY(src.walk(ctx, entry, F, F, true, scorer, t, forest.parent.as<int32_t>(), w));
    PFZ_TRY(forest.flatten(ctx, w.state.as<unsigned long long>() + 2));
    unsigned long long state[3];
    PFZ_TRY(pairs_counters(ctx, w, n, state, out_counters));
    PFZ_TRY(forest.download(ctx, out_label));
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
    PFZ_TRY(pairs_limits("pfz_pairs_join", from_strings, T, candidates->ntop));
    PairSource src;
    src.table = candidates;
    return pairs_join_run(ctx, "pfz_pairs_join", from_strings, T, self, src, scorer, min_similarity, capacity, out_row_ptr, out_idx,
                          out_sim, out_total, out_counters);
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
    PFZ_TRY(pairs_limits("pfz_pairs_components", strings, strings, candidates->ntop));
    PairSource src;
    src.table = candidates;
    return pairs_comp_run(ctx, "pfz_pairs_components", strings, src, scorer, min_similarity, out_label, out_pairs, out_components,
                          out_counters);
}

int pfz_pairs_join_keys(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, const pfz_pairs *pairs,
                        int32_t scorer, double min_similarity, int64_t capacity, int64_t *out_row_ptr, int32_t *out_idx,
                        double *out_sim, int64_t *out_total, int64_t *out_counters)
{
    PFZ_REQUIRE(ctx && from_strings && pairs, "pfz_pairs_join_keys: NULL argument");
    PFZ_PAIRS_REQUIRE_SCORER("pfz_pairs_join_keys");
    PFZ_REQUIRE(capacity >= 0, "pfz_pairs_join_keys: capacity %lld < 0", (long long)capacity);
    PFZ_REQUIRE(out_row_ptr && out_total, "pfz_pairs_join_keys: NULL out_row_ptr / out_total");
    PFZ_REQUIRE(capacity == 0 || (out_idx && out_sim), "pfz_pairs_join_keys: NULL output with capacity %lld", (long long)capacity);
    PFZ_REQUIRE(pairs->ctx == ctx, "pfz_pairs_join_keys: the pair list belongs to another context");
    const bool self = pairs->self;
    PFZ_REQUIRE(!self || to_strings == nullptr || to_strings == from_strings,
                "pfz_pairs_join_keys: the pair list is a self-join's: it takes one list, not a to-list of its own");
    PFZ_REQUIRE(self || to_strings, "pfz_pairs_join_keys: the pair list is a two-list join's: it takes a to-list");
    const pfz_strings *T = self ? from_strings : to_strings;
    PFZ_REQUIRE(from_strings->n == pairs->n_from && T->n == pairs->n_to,
                "pfz_pairs_join_keys: the lists have %lld and %lld strings, the pair list was made for %lld and %lld",
                (long long)from_strings->n, (long long)T->n, (long long)pairs->n_from, (long long)pairs->n_to);
    PFZ_TRY(pairs_limits("pfz_pairs_join_keys", from_strings, T, 0));
    PairSource src;
    src.pairs = pairs;
    return pairs_join_run(ctx, "pfz_pairs_join_keys", from_strings, T, self, src, scorer, min_similarity, capacity, out_row_ptr,
                          out_idx, out_sim, out_total, out_counters);
}

int pfz_pairs_components_keys(pfz_ctx *ctx, const pfz_strings *strings, const pfz_pairs *pairs, int32_t scorer, double min_similarity,
                              int32_t *out_label, int64_t *out_pairs, int64_t *out_components, int64_t *out_counters)
{
    PFZ_REQUIRE(ctx && strings && pairs, "pfz_pairs_components_keys: NULL argument");
    PFZ_PAIRS_REQUIRE_SCORER("pfz_pairs_components_keys");
    PFZ_REQUIRE(out_pairs && out_components, "pfz_pairs_components_keys: NULL out_pairs / out_components");
    PFZ_REQUIRE(strings->n == 0 || out_label, "pfz_pairs_components_keys: NULL out_label");
    PFZ_REQUIRE(pairs->ctx == ctx, "pfz_pairs_components_keys: the pair list belongs to another context");
    PFZ_REQUIRE(pairs->self, "pfz_pairs_components_keys: the pair list is a two-list join's: the components are those of ONE list");
    PFZ_REQUIRE(strings->n == pairs->n_from, "pfz_pairs_components_keys: the list has %lld strings, the pair list was made for %lld",
                (long long)strings->n, (long long)pairs->n_from);
    PFZ_TRY(pairs_limits("pfz_pairs_components_keys", strings, strings, 0));
    PairSource src;
    src.pairs = pairs;
    return pairs_comp_run(ctx, "pfz_pairs_components_keys", strings, src, scorer, min_similarity, out_label, out_pairs, out_components,
                          out_counters);
}

}  // extern "C"
