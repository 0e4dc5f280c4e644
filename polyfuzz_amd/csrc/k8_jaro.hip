// K8 -- all-pairs Jaro / Jaro-Winkler similarity (jellyfish.jaro_similarity / jaro_winkler_similarity) with fused row
// arg-max.
//
// Replaces the hot loop of EditDistance._calculate_edit_distance, reference polyfuzz/models/_distance.py:89-102, with
// the scorer of the reference's custom-model tutorial (docs/tutorial/models/models.md:46-58): scorer(from, to) for every
// to-string, np.argmax (first maximum), np.max -- float64 on the 0..1 scale.  The definition and the bit logic of one
// pair: k8_core.h.
//
// Mapping to CDNA4 -- K4's, on K4's to-side plan (k4_plan.h: alphabet of the to-list, to-strings sorted by length in
// groups of 64, packed symbols), which is built once per to-list and cached on its handle:
//   workgroup (4 waves) = one from-string: its match table PM[symbol] (bit i: a[i] == symbol) lives in LDS;
//   lane = one to-string.  Sweep 1 walks the to-characters: x = PM[c] & window(j) & ~flagged_a, the lowest bit of x is
//     flagged in flagged_a and j in flagged_b (two registers of 32 or 64 bits); m = popcount.  Sweep 2 walks them again for the
//     transpositions (the k-th flagged to-character against the k-th flagged from-position) -- skipped by a wave none
//     of whose lanes has two matches and can still reach its running best (the bound below);
//   score: float64 with the definition's order of operations, computed only for the pairs that can change the lane's
//     running best -- not when the float32 upper bound from m alone, or the one with t, stays below it, not when
//     (m, t, |b|, prefix) equal the best's (same score, later index).  The best is ordered by the float64 values, first
//     index first.
// Register kernel: both strings of up to 32 characters in 32-bit words (nine in ten pairs of real titles); from-strings
// of up to 64 characters against to-strings of up to 256 in 64-bit words.  Everything else -- a longer from-string
// against every to-string, every from-string against the groups of longer to-strings, an alphabet whose table exceeds
// 60 KiB -- takes the general kernel: flag words and match table in global memory, any length, slow.  Every launch
// leaves (score, index) records per from-string; k8_merge picks the first maximum of a row over them.
// The view of the plan, the match table's set / clear, the (score, index) best and its merge are edit_walk.h's, shared with K9 .. K12.
// The two sweeps of the register kernel are written out here and not taken from k8_sweep.h (K20's and K21's): behind every shared
// form tried, k8_jaro_kernel<uint64_t, 8, 4> took 97 registers where this text takes 95 -- 5 waves per SIMD become 4
// (docs/JARO_SWEEP_MEASURED.md).  The plan of the launches and the checks of an entry are k8_launch.h's.
// Bound: integer VALU + LDS look-ups, two sweeps per pair where K4 has one (measured beside K4).
#include "edit_walk.h"
#include "k8_core.h"
#include "k8_launch.h"

#include <algorithm>
#include <limits.h>

namespace pfz {

struct JaroArgs : EditView {
    const int32_t *rows;       // from-rows of this launch
    int32_t n_rows;
    int32_t g_begin, g_end;    // the to-groups of this launch
    const int32_t *skip_idx;   // [n_from] or NULL (decoded: pfz_internal.h decode_skip_codes)
    int32_t skip_up_to;
    int32_t winkler;
    int64_t from_begin;
    int64_t n_to;
    double *matrix;            // optional [(from_end-from_begin) * n_to]
    int32_t parts;             // the to-groups of a from-string are split over `parts` workgroups
    int32_t slot0, n_slots;    // part p of row r leaves its best in rec[(r - from_begin) * n_slots + slot0 + p]
    BestRec *rec;
    unsigned long long *n_scored;   // optional: pairs whose float64 score was computed (the profile's work count)
};

// what the lane remembers of the pair that holds its best, to recognise a pair of the same score without scoring it
struct JaroKey {
    int m, t, lb, prefix;
};

// WORD: uint32_t (from-strings of <= 32 characters) or uint64_t (<= 64); NB: to-strings of up to NB words' characters --
// their flags are NB registers, walked stretch by stretch with compile-time indices
template <typename WORD, int IDB, int NB>
__global__ __launch_bounds__(256) void k8_jaro_kernel(JaroArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    WORD *pm = (WORD *)smem_raw;
    __shared__ double red_s[4];
    __shared__ int red_i[4];
    constexpr int PER = 32 / IDB;  // symbols per dword
    constexpr int SPW = (int)sizeof(WORD) * 8 / PER;      // dwords per stretch
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    pm_reg_zero(A, pm, tid, 256);

    const int parts = A.parts;
    for (int u = blockIdx.x; u < A.n_rows * parts; u += gridDim.x) {
        const int r = u / parts, part = u - r * parts;
        const int row = A.rows[r];
        const int64_t a0 = A.a_off[row];
        const int la = (int)(A.a_off[row + 1] - a0);      // fits the WORD
        const int my_sym = pm_reg_set(A, pm, a0, la, tid);

        const int skip = A.skip_idx ? A.skip_idx[row] : -1;
        const float inv_la = __builtin_amdgcn_rcpf((float)la);
        ScoreBest best = {-1.0, INT_MAX};
        JaroKey key = {-1, 0, 0, 0};
        float best_f = -1.0f;
        int scored = 0;
        for (int g = A.g_begin + wave + 4 * part; g < A.g_end; g += 4 * parts) {
            // (g is wave-uniform: say so, or the loops below get a per-lane trip count)
            const int steps = __builtin_amdgcn_readfirstlane(A.g_steps[g]);
            const uint32_t *gp = A.b_packed + A.g_off[g] + lane;
            const int slot = g * 64 + lane;
            const int orig = A.b_orig[slot];
            const int lb = A.b_len[slot];
            JaroFlags<WORD> s;
            WORD fb[NB];
            jaro_begin(s, jaro_range(la, lb));
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                s.fb = 0;
                for (int t = k * SPW; t < min(steps, (k + 1) * SPW); ++t) {
                    const uint32_t pk = gp[(int64_t)t * 64];
#pragma unroll
                    for (int q = 0; q < PER; ++q)
                        jaro_match<WORD>(s, pm[__builtin_amdgcn_ubfe(pk, q * IDB, IDB)], t * PER + q, (t - k * SPW) * PER + q);
                }
                fb[k] = s.fb;
            }
            const int m = __popcll((uint64_t)s.fa);
            const int prefix = jaro_prefix(s.pre);
            const bool out = orig < 0 || choice_left_out(orig, skip, A.skip_up_to);
            // w <= the bound from m alone: below the lane's running best, the pair needs neither t nor its score
            const float inv_lb = __builtin_amdgcn_rcpf((float)lb);
            const bool hopeless = jaro_bound(m, inv_la, inv_lb, 1.0f, prefix, A.winkler) + K8_BOUND_MARGIN < best_f;
            int half_t = 0;
            // (one flagged pair cannot be out of order; the sweep runs for the wave if a single lane wants it)
            if (__any(m >= 2 && orig >= 0 && (A.matrix || !(out || hopeless)))) {
#pragma unroll
                for (int k = 0; k < NB; ++k) {
                    s.fb = fb[k];
                    for (int t = k * SPW; t < min(steps, (k + 1) * SPW); ++t) {
                        const uint32_t pk = gp[(int64_t)t * 64];
#pragma unroll
                        for (int q = 0; q < PER; ++q)
                            half_t += jaro_transpose<WORD>(s, pm[__builtin_amdgcn_ubfe(pk, q * IDB, IDB)], (t - k * SPW) * PER + q);
                    }
                }
            }
            if (orig < 0) continue;
            if (A.matrix) A.matrix[((int64_t)row - A.from_begin) * A.n_to + orig] = out ? -1.0 : jaro_score(m, half_t, la, lb, prefix, A.winkler);
            if (out || hopeless) continue;
            // a lane meets its to-strings by (length, original index) ascending: a pair whose (m, t, |b|, prefix) are the
            // best's has the best's score and a later index
            if (m == key.m && half_t / 2 == key.t && lb == key.lb && prefix == key.prefix) continue;
            // the bound again, with t (m = 0: not a number, not below anything -- scored, 0)
            const float last = (float)(m - half_t / 2) * __builtin_amdgcn_rcpf((float)m);
            if (jaro_bound(m, inv_la, inv_lb, last, prefix, A.winkler) + K8_BOUND_MARGIN < best_f) continue;
            const double sc = jaro_score(m, half_t, la, lb, prefix, A.winkler);
            ++scored;
            if (sc > best.score || (sc == best.score && orig < best.idx)) {
                best.score = sc;
                best.idx = orig;
                best_f = (float)sc;
                key = JaroKey{m, half_t / 2, lb, prefix};
            }
        }
        best_of_block(best, red_s, red_i, A.rec + ((int64_t)row - A.from_begin) * A.n_slots + A.slot0 + part);
        wave_count(A.n_scored, scored);
        pm_reg_clear(pm, my_sym);
    }
}

// The general case: any lengths, any alphabet.  The match table of the workgroup's from-string (W_A words per symbol)
// and every lane's flag words (W_A for the from-side, W_B for its to-string) are in global memory.
template <int IDB>
__global__ __launch_bounds__(256) void k8_jaro_general_kernel(JaroArgs A, int32_t WA, int32_t WB, uint64_t *__restrict__ pm_all,
                                                               uint64_t *__restrict__ fa_all, uint64_t *__restrict__ fb_all)
{
    __shared__ double red_s[4];
    __shared__ int red_i[4];
    constexpr int PER = 32 / IDB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t *pm = pm_all + (int64_t)blockIdx.x * A.n_sym1 * WA;      // zero on entry, zero again after every row
    uint64_t *fa = fa_all + (int64_t)blockIdx.x * WA * 256 + tid;     // fa[w * 256]: this lane's word w
    uint64_t *fb = fb_all + (int64_t)blockIdx.x * WB * 256 + tid;
    const int parts = A.parts;
    for (int u = blockIdx.x; u < A.n_rows * parts; u += gridDim.x) {
        const int r = u / parts, part = u - r * parts;
        const int row = A.rows[r];
        const int64_t a0 = A.a_off[row];
        const int la = (int)(A.a_off[row + 1] - a0);
        pm_global_set(A, pm, WA, a0, la, tid, 256);
        const int skip = A.skip_idx ? A.skip_idx[row] : -1;
        ScoreBest best = {-1.0, INT_MAX};
        int scored = 0;
        for (int g = A.g_begin + wave + 4 * part; g < A.g_end; g += 4 * parts) {
            const uint32_t *gp = A.b_packed + A.g_off[g] + lane;
            const int steps = A.g_steps[g];
            const int slot = g * 64 + lane;
            const int orig = A.b_orig[slot];
            const int lb = A.b_len[slot];
            const int range = jaro_range(la, lb);
            for (int w = 0; w < WA; ++w) fa[(int64_t)w * 256] = 0ull;
            for (int w = 0; w < WB; ++w) fb[(int64_t)w * 256] = 0ull;
            int m = 0;
            uint32_t pre = 0;
            for (int t = 0; t < steps; ++t) {
                const uint32_t pk = gp[(int64_t)t * 64];
                for (int q = 0; q < PER; ++q) {
                    const uint32_t c = (pk >> (q * IDB)) & ((1u << IDB) - 1u);
                    if (c == 0) continue;                           // padding behind the string's end
                    const int j = t * PER + q;
                    const uint64_t *pmc = pm + (int64_t)c * WA;
                    if (j < 4) pre |= (uint32_t)((pmc[0] >> j) & 1) << j;
                    const int lo = max(j - range, 0), hi = min(j + range, la - 1);
                    for (int w = lo >> 6; w <= hi >> 6 && lo <= hi; ++w) {
                        const uint64_t f = fa[(int64_t)w * 256];
                        const uint64_t x = pmc[w] & bit_span<uint64_t>(max(lo - 64 * w, 0), min(hi - 64 * w, 63)) & ~f;
                        if (x) {
                            fa[(int64_t)w * 256] = f | (x & (0 - x));
                            fb[(int64_t)(j >> 6) * 256] |= 1ull << (j & 63);
                            ++m;
                            break;
                        }
                    }
                }
            }
            int half_t = 0;
            if (m >= 2) {
                int wa = 0;
                uint64_t cur = fa[0];
                for (int t = 0; t < steps; ++t) {
                    const uint32_t pk = gp[(int64_t)t * 64];
                    for (int q = 0; q < PER; ++q) {
                        const uint32_t c = (pk >> (q * IDB)) & ((1u << IDB) - 1u);
                        const int j = t * PER + q;
                        if (c == 0 || !((fb[(int64_t)(j >> 6) * 256] >> (j & 63)) & 1)) continue;
                        while (cur == 0 && wa + 1 < WA) cur = fa[(int64_t)(++wa) * 256];      // (as many flags on either side)
                        const uint64_t low = cur & (0 - cur);
                        cur ^= low;
                        half_t += !(pm[(int64_t)c * WA + wa] & low);
                    }
                }
            }
            if (orig >= 0) {
                const bool out = choice_left_out(orig, skip, A.skip_up_to);
                const double sc = out ? -1.0 : jaro_score(m, half_t, la, lb, jaro_prefix(pre), A.winkler);
                if (A.matrix) A.matrix[((int64_t)row - A.from_begin) * A.n_to + orig] = sc;
                if (!out) best_take(best, sc, orig);
                scored += !out;
            }
        }
        best_of_block(best, red_s, red_i, A.rec + ((int64_t)row - A.from_begin) * A.n_slots + A.slot0 + part);
        wave_count(A.n_scored, scored);
        pm_global_clear(A, pm, WA, a0, la, tid, 256);
    }
}

// the first maximum of every from-string over the records its launches left
__global__ __launch_bounds__(256) void k8_merge(const BestRec *__restrict__ rec, int32_t n_slots, int64_t n_rows,
                                                 int32_t *__restrict__ out_idx, double *__restrict__ out_score)
{
    best_merge(rec, n_slots, n_rows, out_idx, out_score);
}

static int jaro_run(pfz_ctx *ctx, const pfz_strings *F, const pfz_strings *T, int32_t scorer, const int32_t *skip_idx, int64_t begin,
                    int64_t end, int32_t *out_idx, double *out_score, double *out_matrix, pfz_topn *out_dev = nullptr)
{
    PFZ_REQUIRE(ctx && F && T, "pfz_jaro: NULL argument");
    PFZ_TRY(jaro_check_scorer("pfz_jaro", scorer));
    PFZ_REQUIRE(begin >= 0 && begin <= end && end <= F->n, "pfz_jaro: row range [%lld,%lld) outside [0,%lld)",
                (long long)begin, (long long)end, (long long)F->n);
    const int64_t n_rows = end - begin;
    if (n_rows == 0) return PFZ_OK;
    PFZ_HIP(hipSetDevice(ctx->device));
    PFZ_TRY(jaro_check_limits("pfz_jaro", F, T));
    const pfz_indel_plan *pl;
    PFZ_TRY(indel_plan_get(ctx, T, &pl));
    const int64_t n_to = T->n;

    // which rows the register kernels serve, against which groups, in how many parts: k8_launch.h
    const JaroPlan plan = jaro_plan(ctx, F, T, pl, begin, end);
    const std::vector<int32_t> &rows_reg = plan.rows_reg, &rows_long = plan.rows_long;
    const int32_t n_groups = plan.n_groups, g256 = plan.g256;
    const int64_t longest = plan.longest;

    DevBuf d_skip, d_oidx, d_oscore, d_matrix, d_rows_reg, d_rows_long, d_rec, d_scored;
    int skip_up_to = 0;
    if (skip_idx) {
        std::vector<int32_t> codes(skip_idx, skip_idx + F->n);
        skip_up_to = decode_skip_codes(codes);
        PFZ_REQUIRE(skip_up_to >= 0, "pfz_jaro_argmax: skip_idx mixes single choices (>= 0) and 'up to' codes (<= -2)");
        PFZ_TRY(d_skip.upload(ctx, codes));
    }
    PFZ_TRY(d_oidx.alloc(ctx, (size_t)n_rows * sizeof(int32_t)));
    PFZ_TRY(d_oscore.alloc(ctx, (size_t)n_rows * sizeof(double)));
    if (out_matrix) PFZ_TRY(d_matrix.alloc(ctx, (size_t)n_rows * (size_t)n_to * sizeof(double)));
    if (!rows_reg.empty()) PFZ_TRY(d_rows_reg.upload(ctx, rows_reg));
    if (!rows_long.empty()) PFZ_TRY(d_rows_long.upload(ctx, rows_long));

    // A row's launches leave their records side by side; the last slot is the general kernel's.
    const int64_t max_grid = plan.max_grid;
    const int32_t parts_long = plan.parts_long, n_slots = plan.n_slots;
    const size_t rec_bytes = (size_t)n_rows * (size_t)n_slots * sizeof(BestRec);
    PFZ_TRY(d_rec.alloc(ctx, rec_bytes));
    PFZ_HIP(hipMemsetAsync(d_rec.p, 0xff, rec_bytes, ctx->stream));      // idx = -1: no candidate

    JaroArgs A;
    static_cast<EditView &>(A) = edit_view(F, pl);
    A.skip_idx = skip_idx ? (const int32_t *)d_skip.p : nullptr;
    A.skip_up_to = skip_up_to;
    A.winkler = scorer;
    A.from_begin = begin;
    A.n_to = n_to;
    A.matrix = out_matrix ? (double *)d_matrix.p : nullptr;
    A.n_slots = n_slots;
    A.rec = (BestRec *)d_rec.p;
    A.n_scored = nullptr;
    if (ctx->prof) {          // pfz_prof_get("k8_pairs_scored"): how many pairs the arg-max needed the float64 score of (read after the timed scope)
        PFZ_TRY(d_scored.alloc(ctx, sizeof(unsigned long long)));
        PFZ_HIP(hipMemsetAsync(d_scored.p, 0, sizeof(unsigned long long), ctx->stream));
        A.n_scored = d_scored.as<unsigned long long>();
    }

    {
        ProfScope ps_all(ctx, "k8_jaro");
        for (const JaroRegLaunch &L : plan.reg) {
            if (L.parts == 0) continue;
            A.rows = d_rows_reg.as<int32_t>() + L.row0;
            A.n_rows = (int32_t)L.n_rows;
            A.g_begin = L.g_begin;
            A.g_end = L.g_end;
            A.parts = L.parts;
            A.slot0 = L.slot0;
            const dim3 grid((unsigned)std::min<int64_t>((int64_t)A.n_rows * L.parts, max_grid));
            const size_t lds = (size_t)A.n_sym1 * (L.wide ? sizeof(uint64_t) : sizeof(uint32_t));
            dispatch_idb(pl->idb, [&](auto IDB) {
                if (L.wide) hipLaunchKernelGGL((k8_jaro_kernel<uint64_t, decltype(IDB)::value, 4>), grid, dim3(256), lds, ctx->stream, A);
                else hipLaunchKernelGGL((k8_jaro_kernel<uint32_t, decltype(IDB)::value, 1>), grid, dim3(256), lds, ctx->stream, A);
            });
            PFZ_HIP(hipGetLastError());
        }
        // the general kernel: the from-strings of the register launches against the groups of longer to-strings, the other
        // from-strings against every group
        const int32_t WB = (int32_t)std::max<int64_t>(1, (T->max_len + 63) / 64);
        for (int pass = 0; pass < 2; ++pass) {
            const std::vector<int32_t> &rows = pass == 0 ? rows_reg : rows_long;
            A.g_begin = pass == 0 ? g256 : 0;
            A.g_end = n_groups;
            if (rows.empty() || A.g_begin >= A.g_end) continue;
            A.rows = (const int32_t *)(pass == 0 ? d_rows_reg.p : d_rows_long.p);
            A.n_rows = (int32_t)rows.size();
            A.parts = pass == 0 ? 1 : parts_long;
            A.slot0 = pass == 0 ? n_slots - 1 : 0;
            const int32_t WA = pass == 0 ? 1 : (int32_t)((longest + 63) / 64);
            int64_t grid = std::min<int64_t>((int64_t)rows.size() * A.parts, max_grid);
            PFZ_TRY(general_grid(&grid, A.n_sym1, WA, "pfz_jaro", "a from-string", longest));
            ProfScope ps(ctx, "k8_jaro_general");
            GeneralBufs gb;      // (col[0]: the from-flags, col[1]: the to-flags)
            PFZ_TRY(general_bufs_alloc(ctx, &gb, grid, A.n_sym1, WA, {WA, WB, 0}, 256));
            dispatch_idb(pl->idb, [&](auto IDB) {
                hipLaunchKernelGGL((k8_jaro_general_kernel<decltype(IDB)::value>), dim3((unsigned)grid), dim3(256), 0, ctx->stream, A, WA, WB,
                                   gb.pm.as<uint64_t>(), gb.col[0].as<uint64_t>(), gb.col[1].as<uint64_t>());
            });
            PFZ_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(k8_merge, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, ctx->stream, (const BestRec *)d_rec.p, n_slots,
                           n_rows, d_oidx.as<int32_t>(), d_oscore.as<double>());
        PFZ_HIP(hipGetLastError());
    }
    if (A.n_scored) {
        unsigned long long n = 0;
        PFZ_TRY(copy_d2h(ctx, &n, d_scored.p, sizeof(n)));
        prof_count(ctx, "k8_pairs_scored", (int64_t)n);
    }
    if (out_dev) return best_to_topn(ctx, d_oidx.as<int32_t>(), d_oscore.as<double>(), n_rows, out_dev);     // (no copy, no wait)
    if (out_idx) PFZ_TRY(copy_d2h(ctx, out_idx, d_oidx.p, (size_t)n_rows * sizeof(int32_t)));
    if (out_score) PFZ_TRY(copy_d2h(ctx, out_score, d_oscore.p, (size_t)n_rows * sizeof(double)));
    if (out_matrix) PFZ_TRY(copy_d2h(ctx, out_matrix, d_matrix.p, (size_t)n_rows * (size_t)n_to * sizeof(double)));
    PFZ_HIP(hipStreamSynchronize(ctx->stream));
    return PFZ_OK;
}

}  // namespace pfz

using namespace pfz;

extern "C" {

int pfz_jaro_argmax(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, int32_t scorer,
                    const int32_t *skip_idx, int64_t from_begin, int64_t from_end, int32_t *out_idx, double *out_score)
{
    PFZ_REQUIRE(out_idx && out_score, "pfz_jaro_argmax: NULL output");
    return jaro_run(ctx, from_strings, to_strings, scorer, skip_idx, from_begin, from_end, out_idx, out_score, nullptr);
}

int pfz_jaro_argmax_dev(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, int32_t scorer,
                        const int32_t *skip_idx, int64_t from_begin, int64_t from_end, pfz_topn *out)
{
    PFZ_REQUIRE(out && out->ntop == 2 && out->n_rows >= from_end - from_begin,
                "pfz_jaro_argmax_dev: the result buffer must have 2 columns and >= %lld rows", (long long)(from_end - from_begin));
    return jaro_run(ctx, from_strings, to_strings, scorer, skip_idx, from_begin, from_end, nullptr, nullptr, nullptr, out);
}

int pfz_jaro_matrix_host(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, int32_t scorer,
                         int64_t from_begin, int64_t from_end, double *out_matrix)
{
    PFZ_REQUIRE(out_matrix, "pfz_jaro_matrix_host: NULL output");
    if (to_strings && to_strings->n == 0) {
        return jaro_check_scorer("pfz_jaro", scorer);
    }
    return jaro_run(ctx, from_strings, to_strings, scorer, nullptr, from_begin, from_end, nullptr, nullptr, out_matrix);
}

}  // extern "C"
