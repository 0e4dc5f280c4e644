// K9 -- all-pairs Levenshtein / OSA similarity (rapidfuzz's Levenshtein.normalized_similarity / OSA.normalized_similarity) with
// fused row arg-max.
//
// Replaces the hot loop of EditDistance._calculate_edit_distance, reference polyfuzz/models/_distance.py:89-102, with one of the
// two as scorer(from, to) for every to-string, np.argmax (first maximum), np.max -- float64 on the 0..1 scale.  The definition and
// the bit logic of one pair: k9_core.h.
//
// Mapping to CDNA4 -- K8's (the view of the plan, the match table, the row's best and its merge are the one copy in edit_walk.h),
// on K4's to-side plan (k4_plan.h: alphabet of the to-list, to-strings sorted by length in groups of 64,
// packed symbols), which is built once per to-list and cached on its handle:
//   workgroup (4 waves) = one from-string: its match table PM[symbol] (bit i: a[i] == symbol) lives in LDS, built per from-string
//     and cleared by the positions it set;
//   lane = one to-string: one step of the Myers / Hyyro recurrence per to-character, the column's vertical deltas in two registers
//     of 32 or 64 bits (two more for OSA).  There is no per-to-position state, so a to-string of any length is only a longer walk;
//     a lane's distance stops moving at its own length, whatever the group's longest string still walks.
// The length bound: d >= ||a| - |b||, so no to-string of length |b| scores above 1 - ||a| - |b|| / max(|a|, |b|).  The groups are
// sorted by length, so a wave walks its groups from the one nearest |a| outwards, alternately up and down, skips a group none of
// whose lanes can reach the workgroup's best (an LDS word: the bits of the best float64 score any lane has reached -- non-negative
// doubles order as integers), and ends a direction at the first such group on the monotone side.  Strictly below only: an equal
// score with an earlier original index wins the tie.  Bound and score come from the same formula (k9_core.h), compared as float64.
// Register kernel: from-strings of up to 32 characters in 32-bit words, of up to 64 in 64-bit words.  Longer from-strings, and an
// alphabet whose table exceeds 60 KiB, take the general kernel: words and match table in global memory, every pair walked, slow.
// Every launch leaves (score, index) records per from-string and part; k9_merge picks the first maximum of a row over them.
// The top-n form (pfz_lev_topn, topn_wave.h): every wave keeps ONE sorted list of its ntop best pairs, one entry per lane, in place
// of the lanes' bests.  The workgroup's LDS word then holds the best LAST entry of a full list: ntop choices at or above that
// score exist in the row, so a to-string whose length bound is STRICTLY below it is none of the row's ntop best -- the same
// test, the same walk order, the same end of a direction.  The waves leave their lists side by side, in a buffer per launch
// (rows of the class x its parts x 4 x ntop keys); topn_merge picks the row's.
// Bound: integer VALU + LDS look-ups, one sweep per pair (measured beside K4 and K8).
#include "edit_walk.h"
#include "topn_wave.h"

#include <algorithm>
#include <limits.h>

namespace pfz {

struct LevArgs : EditView {
    const int32_t *rows;       // from-rows of this launch
    int32_t n_rows;
    const int32_t *skip_idx;   // [n_from] or NULL (decoded: pfz_internal.h decode_skip_codes)
    int32_t skip_up_to;
    int64_t from_begin;
    int64_t n_to;
    int32_t *matrix;           // optional [(from_end-from_begin) * n_to] distances: every pair is walked
    int32_t parts;             // the to-groups of a from-string are split over `parts` workgroups, each pruning on its own best
    int32_t n_slots;           // part p of row r leaves its best in rec[(r - from_begin) * n_slots + p]
    BestRec *rec;
    unsigned long long *n_walked;   // optional: pairs whose recurrence was walked (the profile's work count)
    int32_t ntop;              // the top-n kernels: wave w of part p of row r leaves its list in
    TopnKey *lists;            // lists[((r * parts + p) * 4 + w) * ntop], r the row's place in `rows`: one buffer per launch
};

constexpr int K9_LDS_HEAD = 16;      // the workgroup's best in front of the match table (which stays 16-byte aligned)

// WORD: uint32_t (from-strings of <= 32 characters) or uint64_t (<= 64), against to-strings of any length
// TOPN: a list of A.ntop per wave in place of a best per lane
template <typename WORD, int IDB, bool OSA, bool TOPN>
__device__ __forceinline__ void k9_lev_body(const LevArgs &A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    unsigned long long *wg_best = (unsigned long long *)smem_raw;
    WORD *pm = (WORD *)(smem_raw + K9_LDS_HEAD);
    __shared__ double red_s[4];
    __shared__ int red_i[4];
    constexpr int PER = 32 / IDB;  // symbols per dword
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    pm_reg_zero(A, pm, tid, 256);

    const int parts = A.parts;
    const bool prune = A.matrix == nullptr;
    for (int u = blockIdx.x; u < A.n_rows * parts; u += gridDim.x) {
        const int r = u / parts, part = u - r * parts;
        const int row = A.rows[r];
        const int64_t a0 = A.a_off[row];
        const int la = (int)(A.a_off[row + 1] - a0);      // fits the WORD
        // (pm_reg_set, with the workgroup's best reset in front of its barrier)
        const int my_sym = tid < la ? edit_symbol(A, A.a_chars, A.a_width, a0 + tid) : 0;
        if (my_sym) lds_or(&pm[my_sym], (WORD)1 << tid);
        if (tid == 0) *wg_best = 0ull;                     // +0.0: no bound is below it
        __syncthreads();

        const int skip = A.skip_idx ? A.skip_idx[row] : -1;
        ScoreBest best = {-1.0, INT_MAX};
        TopnList list = topn_empty();
        int walked = 0;
        // this wave's groups: base + stride * k, k < K (wave-uniform: say so, or the loops below get a per-lane trip count)
        const int base = __builtin_amdgcn_readfirstlane(wave + 4 * part), stride = 4 * parts;
        const int K = base < A.n_groups ? (A.n_groups - base + stride - 1) / stride : 0;
        // the first of them whose longest string reaches |a| (g_steps rounds up to whole dwords: near is enough, the walk's
        // ends are decided by the lanes' own lengths)
        int lo = 0, hi = K;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (__builtin_amdgcn_readfirstlane(A.g_steps[base + stride * mid]) * PER >= la) hi = mid;
            else lo = mid + 1;
        }
        int up = lo, down = lo - 1;
        bool turn_up = true;
        while (up < K || down >= 0) {
            const bool go_up = up < K && (turn_up || down < 0);
            turn_up = !go_up;
            const int g = base + stride * (go_up ? up++ : down--);
            const int slot = g * 64 + lane;
            const int orig = A.b_orig[slot];
            const int lb = A.b_len[slot];
            const bool real = orig >= 0;
            const bool out = !real || choice_left_out(orig, skip, A.skip_up_to);
            double wb = 0.0;
            if (prune) {
                wb = __longlong_as_double((long long)*(volatile unsigned long long *)wg_best);
                const bool below = lev_length_bound(la, lb) < wb;
                if (!__any(!out && !below)) {
                    // nothing to gain here; and nothing further out either, once every string of the group -- the left-out ones
                    // too -- is below the best and on the far side of |a|: the bound only falls from here
                    if (!__any(real && !(below && (go_up ? lb >= la : lb <= la)))) {
                        if (go_up) up = K;
                        else down = -1;
                    }
                    continue;
                }
            }
            const int steps = __builtin_amdgcn_readfirstlane(A.g_steps[g]);
            const uint32_t *gp = A.b_packed + A.g_off[g] + lane;
            LevState<WORD> s;
            lev_begin(s, la);
            for (int t = 0; t < steps; ++t) {
                const uint32_t pk = gp[(int64_t)t * 64];
#pragma unroll
                for (int q = 0; q < PER; ++q)
                    lev_step<WORD, OSA>(s, pm[__builtin_amdgcn_ubfe(pk, q * IDB, IDB)], t * PER + q < lb);
            }
            if constexpr (TOPN) {
                walked += real;
                topn_insert(list, A.ntop, !out, out ? 0.0 : lev_similarity(lev_distance(s.dist, la, lb), la, lb), orig);
                // a full list: A.ntop choices at or above its last entry's score exist
                double last;
                if (topn_full(list, A.ntop, &last) && last > wb && lane == 0)
                    atomicMax(wg_best, (unsigned long long)__double_as_longlong(last));
                continue;
            }
            if (!real) continue;
            ++walked;
            const int d = lev_distance(s.dist, la, lb);
            if (A.matrix) A.matrix[((int64_t)row - A.from_begin) * A.n_to + orig] = d;
            if (out) continue;
            const double sc = lev_similarity(d, la, lb);
            best_take(best, sc, orig);
            if (prune && sc > wb) atomicMax(wg_best, (unsigned long long)__double_as_longlong(sc));
        }
        if constexpr (TOPN) {
            topn_store(list, A.ntop, A.lists + (((int64_t)r * parts + part) * 4 + wave) * A.ntop);
            __syncthreads();      // (every wave is done with the match table)
        }
        else best_of_block(best, red_s, red_i, A.rec + ((int64_t)row - A.from_begin) * A.n_slots + part);
        wave_count(A.n_walked, walked);
        pm_reg_clear(pm, my_sym);
    }
}

template <typename WORD, int IDB, bool OSA>
__global__ __launch_bounds__(256) void k9_lev_kernel(LevArgs A)
{
    k9_lev_body<WORD, IDB, OSA, false>(A);
}

template <typename WORD, int IDB, bool OSA>
__global__ __launch_bounds__(256) void k9_lev_topn_kernel(LevArgs A)
{
    k9_lev_body<WORD, IDB, OSA, true>(A);
}

// The general case: any from-length, any alphabet.  The match table of the workgroup's from-string (WA words per symbol) and every
// lane's column (VP, VN and, for OSA, the previous D0: WA words each) are in global memory; every pair is walked.
template <int IDB, bool OSA, bool TOPN>
__device__ __forceinline__ void k9_lev_general_body(const LevArgs &A, int32_t WA, uint64_t *__restrict__ pm_all,
                                                    uint64_t *__restrict__ vp_all, uint64_t *__restrict__ vn_all,
                                                    uint64_t *__restrict__ d0_all)
{
    __shared__ double red_s[4];
    __shared__ int red_i[4];
    constexpr int PER = 32 / IDB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t *pm = pm_all + (int64_t)blockIdx.x * A.n_sym1 * WA;      // zero on entry, zero again after every row
    uint64_t *vp = vp_all + (int64_t)blockIdx.x * WA * 256 + tid;     // vp[w * 256]: this lane's word w
    uint64_t *vn = vn_all + (int64_t)blockIdx.x * WA * 256 + tid;
    uint64_t *d0 = d0_all + (int64_t)blockIdx.x * WA * 256 + tid;
    const int parts = A.parts;
    for (int u = blockIdx.x; u < A.n_rows * parts; u += gridDim.x) {
        const int r = u / parts, part = u - r * parts;
        const int row = A.rows[r];
        const int64_t a0 = A.a_off[row];
        const int la = (int)(A.a_off[row + 1] - a0);
        const int W = la > 0 ? (la + 63) / 64 : 1;                    // <= WA
        pm_global_set(A, pm, WA, a0, la, tid, 256);
        const int skip = A.skip_idx ? A.skip_idx[row] : -1;
        const uint64_t last = la > 0 ? 1ull << ((la - 1) % 64) : 0ull;
        ScoreBest best = {-1.0, INT_MAX};
        TopnList list = topn_empty();
        int walked = 0;
        for (int g = wave + 4 * part; g < A.n_groups; g += 4 * parts) {
            const uint32_t *gp = A.b_packed + A.g_off[g] + lane;
            const int steps = A.g_steps[g];
            const int slot = g * 64 + lane;
            const int orig = A.b_orig[slot];
            const int lb = A.b_len[slot];
            for (int w = 0; w < W; ++w) {
                vp[(int64_t)w * 256] = low_ones<uint64_t>(la - 64 * w);
                vn[(int64_t)w * 256] = 0ull;
                d0[(int64_t)w * 256] = 0ull;
            }
            int dist = la;
            uint32_t c_prev = 0;                                        // (symbol 0: an empty table entry)
            for (int t = 0; t < steps; ++t) {
                const uint32_t pk = gp[(int64_t)t * 64];
                for (int q = 0; q < PER; ++q) {
                    if (t * PER + q >= lb) continue;                    // padding behind the string's end
                    const uint32_t c = (pk >> (q * IDB)) & ((1u << IDB) - 1u);
                    // (lev_column_step, written out: through the helper this kernel's OSA instances need up to four registers more)
                    const uint64_t *eq = pm + (int64_t)c * WA, *eq_prev = pm + (int64_t)c_prev * WA;
                    LevCarry cy = lev_carry_begin();
                    uint64_t hp = 0, hn = 0;
                    for (int w = 0; w < W; ++w) {
                        uint64_t x_vp = vp[(int64_t)w * 256], x_vn = vn[(int64_t)w * 256], x_d0 = OSA ? d0[(int64_t)w * 256] : 0ull;
                        lev_step_word<OSA>(x_vp, x_vn, x_d0, eq[w], OSA ? eq_prev[w] : 0ull, cy, &hp, &hn);
                        vp[(int64_t)w * 256] = x_vp;
                        vn[(int64_t)w * 256] = x_vn;
                        if (OSA) d0[(int64_t)w * 256] = x_d0;
                    }
                    dist += (int)((hp & last) != 0) - (int)((hn & last) != 0);
                    c_prev = c;
                }
            }
            if constexpr (TOPN) {
                const bool have = orig >= 0 && !choice_left_out(orig, skip, A.skip_up_to);
                walked += orig >= 0;
                topn_insert(list, A.ntop, have, have ? lev_similarity(lev_distance(dist, la, lb), la, lb) : 0.0, orig);
            }
            else if (orig >= 0) {
                ++walked;
                const int d = lev_distance(dist, la, lb);
                if (A.matrix) A.matrix[((int64_t)row - A.from_begin) * A.n_to + orig] = d;
                if (!choice_left_out(orig, skip, A.skip_up_to)) best_take(best, lev_similarity(d, la, lb), orig);
            }
        }
        if constexpr (TOPN) {
            topn_store(list, A.ntop, A.lists + (((int64_t)r * parts + part) * 4 + wave) * A.ntop);
            __syncthreads();      // (every wave is done with the match table)
        }
        else best_of_block(best, red_s, red_i, A.rec + ((int64_t)row - A.from_begin) * A.n_slots + part);
        wave_count(A.n_walked, walked);
        pm_global_clear(A, pm, WA, a0, la, tid, 256);
    }
}

template <int IDB, bool OSA>
__global__ __launch_bounds__(256) void k9_lev_general_kernel(LevArgs A, int32_t WA, uint64_t *__restrict__ pm_all,
                                                              uint64_t *__restrict__ vp_all, uint64_t *__restrict__ vn_all,
                                                              uint64_t *__restrict__ d0_all)
{
    k9_lev_general_body<IDB, OSA, false>(A, WA, pm_all, vp_all, vn_all, d0_all);
}

template <int IDB, bool OSA>
__global__ __launch_bounds__(256) void k9_lev_general_topn_kernel(LevArgs A, int32_t WA, uint64_t *__restrict__ pm_all,
                                                                   uint64_t *__restrict__ vp_all, uint64_t *__restrict__ vn_all,
                                                                   uint64_t *__restrict__ d0_all)
{
    k9_lev_general_body<IDB, OSA, true>(A, WA, pm_all, vp_all, vn_all, d0_all);
}

// the first maximum of every from-string over the records its launch left
__global__ __launch_bounds__(256) void k9_merge(const BestRec *__restrict__ rec, int32_t n_slots, int64_t n_rows,
                                                 int32_t *__restrict__ out_idx, double *__restrict__ out_score)
{
    best_merge(rec, n_slots, n_rows, out_idx, out_score);
}

template <typename WORD>
static void launch_reg(const LevArgs &A, int idb, int osa, dim3 grid, size_t lds, hipStream_t st)
{
    dispatch_idb_osa(idb, osa != 0, [&](auto IDB, auto OSA) {
        if (A.ntop > 0) hipLaunchKernelGGL((k9_lev_topn_kernel<WORD, decltype(IDB)::value, decltype(OSA)::value>), grid, dim3(256), lds, st, A);
        else hipLaunchKernelGGL((k9_lev_kernel<WORD, decltype(IDB)::value, decltype(OSA)::value>), grid, dim3(256), lds, st, A);
    });
}

static int lev_run(pfz_ctx *ctx, const pfz_strings *F, const pfz_strings *T, int32_t scorer, const int32_t *skip_idx, int64_t begin,
                   int64_t end, int32_t *out_idx, double *out_score, int32_t *out_matrix, pfz_topn *out_dev = nullptr, int32_t ntop = 0)
{
    // ntop == 0: the arg-max kernels; ntop >= 1: the top-n kernels, out_idx / out_score of [rows * ntop]
    PFZ_REQUIRE(ctx && F && T, "pfz_lev: NULL argument");
    PFZ_REQUIRE(scorer == 0 || scorer == 1, "pfz_lev: scorer %d is neither 0 (Levenshtein) nor 1 (OSA)", scorer);
    PFZ_REQUIRE(begin >= 0 && begin <= end && end <= F->n, "pfz_lev: row range [%lld,%lld) outside [0,%lld)", (long long)begin,
                (long long)end, (long long)F->n);
    const int64_t n_rows = end - begin;
    if (n_rows == 0) return PFZ_OK;
    PFZ_HIP(hipSetDevice(ctx->device));
    if (T->n >= INT_MAX - 64 || F->n >= INT_MAX || T->max_len >= INT_MAX / 2 || F->max_len >= INT_MAX / 2) {
        set_error("pfz_lev: list or string too long");
        return PFZ_ERR_UNSUPPORTED;
    }
    const pfz_indel_plan *pl;
    PFZ_TRY(indel_plan_get(ctx, T, &pl));
    const int64_t n_to = T->n;
    const int32_t n_groups = (int32_t)pl->n_groups;

    // The register kernel's share, while the match table fits 60 KiB of LDS (K4's limit): from-strings of <= 32 characters in
    // 32-bit words, of 33 .. 64 in 64-bit words, each against every group.  Everything else is the general kernel's.
    const RowClasses rc = classify_rows(F, begin, end, lds_table_fits(pl));
    const std::vector<int32_t> (&rows_cls)[3] = rc.rows;      // <= 32, 33 .. 64, the general kernel's

    DevBuf d_skip, d_oidx, d_oscore, d_matrix, d_rows[3], d_lists[3], d_rec, d_walked;
    int skip_up_to = 0;
    if (skip_idx) {
        std::vector<int32_t> codes(skip_idx, skip_idx + F->n);
        skip_up_to = decode_skip_codes(codes);
        PFZ_REQUIRE(skip_up_to >= 0, "pfz_lev_argmax: skip_idx mixes single choices (>= 0) and 'up to' codes (<= -2)");
        PFZ_TRY(d_skip.upload(ctx, codes));
    }
    const size_t n_out = (size_t)n_rows * (size_t)std::max(ntop, 1);
    PFZ_TRY(d_oidx.alloc(ctx, n_out * sizeof(int32_t)));
    PFZ_TRY(d_oscore.alloc(ctx, n_out * sizeof(double)));
    if (out_matrix) PFZ_TRY(d_matrix.alloc(ctx, (size_t)n_rows * (size_t)n_to * sizeof(int32_t)));

    // Few from-strings: the to-groups of each are split over `parts` workgroups (K4's rule: >= 4 rounds of work units on the chip,
    // each part at least one group per wave -- four per wave in the register kernel, whose waves prune on what their own
    // workgroup has reached: a wave with a single group has nothing to leave out).  A row is served by one launch: its parts
    // leave their records side by side.
    const int64_t max_grid = (int64_t)ctx->prop.multiProcessorCount * 8;
    int32_t parts[3], n_slots = 1;
    for (int c = 0; c < 3; ++c) {
        parts[c] = 0;
        if (rows_cls[c].empty()) continue;
        PFZ_TRY(d_rows[c].upload(ctx, rows_cls[c]));
        const int64_t n = (int64_t)rows_cls[c].size(), want = (4 * max_grid + n - 1) / n;
        const int64_t cap = std::max<int32_t>(1, n_groups / (c == 2 ? 4 : 16));
        parts[c] = (int32_t)std::max<int64_t>(1, std::min(want, cap));
        n_slots = std::max(n_slots, parts[c]);
    }
    // (top-n: every class has a list buffer of its own -- rows of the class x ITS parts x 4 waves x ntop keys, all of them written)
    const size_t rec_bytes = ntop > 0 ? 0 : (size_t)n_rows * (size_t)n_slots * sizeof(BestRec);
    PFZ_TRY(d_rec.alloc(ctx, rec_bytes));
    if (rec_bytes) PFZ_HIP(hipMemsetAsync(d_rec.p, 0xff, rec_bytes, ctx->stream));      // idx = -1: no candidate
    if (ntop > 0)
        for (int c = 0; c < 3; ++c)
            if (parts[c] != 0) PFZ_TRY(d_lists[c].alloc(ctx, rows_cls[c].size() * (size_t)parts[c] * 4 * (size_t)ntop * sizeof(TopnKey)));

    LevArgs A;
    static_cast<EditView &>(A) = edit_view(F, pl);
    A.skip_idx = skip_idx ? (const int32_t *)d_skip.p : nullptr;
    A.skip_up_to = skip_up_to;
    A.from_begin = begin;
    A.n_to = n_to;
    A.matrix = out_matrix ? (int32_t *)d_matrix.p : nullptr;
    A.n_slots = n_slots;
    A.rec = (BestRec *)d_rec.p;
    A.ntop = ntop;
    A.lists = nullptr;
    A.n_walked = nullptr;
    if (ctx->prof) {          // pfz_prof_get("k9_pairs_walked"): how many pairs the arg-max walked (read after the timed scope)
        PFZ_TRY(d_walked.alloc(ctx, sizeof(unsigned long long)));
        PFZ_HIP(hipMemsetAsync(d_walked.p, 0, sizeof(unsigned long long), ctx->stream));
        A.n_walked = d_walked.as<unsigned long long>();
    }

    {
        ProfScope ps_all(ctx, "k9_lev");
        for (int c = 0; c < 2; ++c) {
            if (parts[c] == 0) continue;
            A.rows = d_rows[c].as<int32_t>();
            A.n_rows = (int32_t)rows_cls[c].size();
            A.parts = parts[c];
            A.lists = d_lists[c].as<TopnKey>();
            const dim3 grid((unsigned)std::min<int64_t>((int64_t)A.n_rows * A.parts, max_grid));
            const size_t lds = K9_LDS_HEAD + (size_t)A.n_sym1 * (c == 1 ? sizeof(uint64_t) : sizeof(uint32_t));
            if (c == 0) launch_reg<uint32_t>(A, pl->idb, scorer, grid, lds, ctx->stream);
            else launch_reg<uint64_t>(A, pl->idb, scorer, grid, lds, ctx->stream);
            PFZ_HIP(hipGetLastError());
        }
        if (parts[2] != 0) {
            A.rows = d_rows[2].as<int32_t>();
            A.n_rows = (int32_t)rows_cls[2].size();
            A.parts = parts[2];
            A.lists = d_lists[2].as<TopnKey>();
            const int32_t WA = (int32_t)((rc.longest + 63) / 64);
            int64_t grid = std::min<int64_t>((int64_t)A.n_rows * A.parts, max_grid);
            PFZ_TRY(general_grid(&grid, A.n_sym1, WA, "pfz_lev", "a from-string", rc.longest));
            ProfScope ps(ctx, "k9_lev_general");
            GeneralBufs gb;
            PFZ_TRY(general_bufs_alloc(ctx, &gb, grid, A.n_sym1, WA, {WA, WA, WA}, 256));
            dispatch_idb_osa(pl->idb, scorer != 0, [&](auto IDB, auto OSA) {
                if (ntop > 0)
                    hipLaunchKernelGGL((k9_lev_general_topn_kernel<decltype(IDB)::value, decltype(OSA)::value>), dim3((unsigned)grid), dim3(256), 0,
                                       ctx->stream, A, WA, gb.pm.as<uint64_t>(), gb.col[0].as<uint64_t>(), gb.col[1].as<uint64_t>(),
                                       gb.col[2].as<uint64_t>());
                else
                    hipLaunchKernelGGL((k9_lev_general_kernel<decltype(IDB)::value, decltype(OSA)::value>), dim3((unsigned)grid), dim3(256), 0,
                                       ctx->stream, A, WA, gb.pm.as<uint64_t>(), gb.col[0].as<uint64_t>(), gb.col[1].as<uint64_t>(),
                                       gb.col[2].as<uint64_t>());
            });
            PFZ_HIP(hipGetLastError());
        }
        if (ntop > 0) {
            for (int c = 0; c < 3; ++c)
                if (parts[c] != 0)
                    PFZ_TRY(topn_merge(d_lists[c].as<TopnKey>(), 4 * parts[c], ntop, d_rows[c].as<int32_t>(), begin, (int64_t)rows_cls[c].size(),
                                       d_oidx.as<int32_t>(), d_oscore.as<double>(), ctx->stream));
        }
        else
            hipLaunchKernelGGL(k9_merge, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, ctx->stream, (const BestRec *)d_rec.p, n_slots,
                               n_rows, d_oidx.as<int32_t>(), d_oscore.as<double>());
        PFZ_HIP(hipGetLastError());
    }
    if (A.n_walked) {
        unsigned long long n = 0;
        PFZ_TRY(copy_d2h(ctx, &n, d_walked.p, sizeof(n)));
        prof_count(ctx, "k9_pairs_walked", (int64_t)n);
    }
    if (out_dev) return best_to_topn(ctx, d_oidx.as<int32_t>(), d_oscore.as<double>(), n_rows, out_dev);     // (no copy, no wait)
    if (out_idx) PFZ_TRY(copy_d2h(ctx, out_idx, d_oidx.p, n_out * sizeof(int32_t)));
    if (out_score) PFZ_TRY(copy_d2h(ctx, out_score, d_oscore.p, n_out * sizeof(double)));
    if (out_matrix) PFZ_TRY(copy_d2h(ctx, out_matrix, d_matrix.p, (size_t)n_rows * (size_t)n_to * sizeof(int32_t)));
    PFZ_HIP(hipStreamSynchronize(ctx->stream));
    return PFZ_OK;
}

}  // namespace pfz

using namespace pfz;

extern "C" {

int pfz_lev_argmax(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, int32_t scorer,
                   const int32_t *skip_idx, int64_t from_begin, int64_t from_end, int32_t *out_idx, double *out_score)
{
    PFZ_REQUIRE(out_idx && out_score, "pfz_lev_argmax: NULL output");
    return lev_run(ctx, from_strings, to_strings, scorer, skip_idx, from_begin, from_end, out_idx, out_score, nullptr);
}

int pfz_lev_argmax_dev(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, int32_t scorer,
                       const int32_t *skip_idx, int64_t from_begin, int64_t from_end, pfz_topn *out)
{
    PFZ_REQUIRE(out && out->ntop == 2 && out->n_rows >= from_end - from_begin,
                "pfz_lev_argmax_dev: the result buffer must have 2 columns and >= %lld rows", (long long)(from_end - from_begin));
    return lev_run(ctx, from_strings, to_strings, scorer, skip_idx, from_begin, from_end, nullptr, nullptr, nullptr, out);
}

int pfz_lev_topn(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, int32_t scorer, const int32_t *skip_idx,
                 int64_t from_begin, int64_t from_end, int32_t ntop, int32_t *out_idx, double *out_score)
{
    PFZ_REQUIRE(out_idx && out_score, "pfz_lev_topn: NULL output");
    PFZ_REQUIRE(ntop >= 1, "pfz_lev_topn: ntop %d < 1", ntop);
    if (ntop > kTopnMax) {
        set_error("pfz_lev_topn: ntop %d exceeds the limit of %d (one list entry per lane of a wave)", ntop, kTopnMax);
        return PFZ_ERR_UNSUPPORTED;
    }
    return lev_run(ctx, from_strings, to_strings, scorer, skip_idx, from_begin, from_end, out_idx, out_score, nullptr, nullptr, ntop);
}

int pfz_lev_matrix_host(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, int32_t scorer,
                        int64_t from_begin, int64_t from_end, int32_t *out_matrix)
{
    PFZ_REQUIRE(out_matrix, "pfz_lev_matrix_host: NULL output");
    if (to_strings && to_strings->n == 0) {
        PFZ_REQUIRE(scorer == 0 || scorer == 1, "pfz_lev: scorer %d is neither 0 (Levenshtein) nor 1 (OSA)", scorer);
        return PFZ_OK;
    }
    return lev_run(ctx, from_strings, to_strings, scorer, nullptr, from_begin, from_end, nullptr, nullptr, out_matrix);
}

}  // extern "C"
