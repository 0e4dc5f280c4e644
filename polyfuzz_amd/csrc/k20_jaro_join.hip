// K20 -- all pairs at or above a Jaro / Jaro-Winkler score, and the connected components of that relation (what
// models.JaroWinkler.join / .components run): for a float64 t in [0, 1], every pair (from i, to j) with
// jaro_score(...) >= t -- K8's score (k8_core.h: jellyfish.jaro_similarity / jaro_winkler_similarity), bit for bit, float64
// against float64, equal kept.  The bit logic of one pair is K8's, unchanged; what a fixed t lets a lane leave out -- the length
// bound, the fewest matches a pair needs, the abandon rule, the bounds behind either sweep -- is k8_core.h's too, every one of them
// a dismissal only where the score is below t.
//
// Mapping to CDNA4 -- K8's word classes on K11's walk, over K4's to-side plan (k4_plan.h: the to-strings sorted by (length, index)
// in groups of 64):
//   workgroup (4 waves) = one from-string per trip of a persistent row loop, its match table PM[symbol] in LDS;  lane = one
//     to-string;  wave = the groups of the row's length window, dealt among the four.
//   the window   for one la the admissible to-lengths are one run around la (k8_core.h jaro_len_run), found once per call for every
//                la by the set-up launch; a row's groups are two binary searches over the plan with that run.  A row whose window
//                is empty never builds its table.
//   in a group   k8_sweep.h's jaro_pair_above against (float)t, shared with K21: sweep 1 with the abandon rule once per packed
//                dword and the wave-uniform exit, the bound with the pair's own prefix, sweep 2 only if a live lane has two matches,
//                the bound with t, the float64 score; then the comparison with t.
//   Every lane of a wave that enters a group reaches the sink -- padding lanes, lanes not owned and dead lanes with hit = false --
//   and every exit from a group is wave-uniform.
// Register kernels: from-strings of <= 32 characters against the groups of <= 32 in 32-bit words; those against the groups of up to
// 256, and from-strings of 33 .. 64 against all groups of up to 256, in 64-bit words with four flag registers.  Everything else --
// longer from-strings, the groups beyond 256 characters for every from-string, an alphabet whose table exceeds 60 KiB -- takes the
// general kernel: pair_score.h's general Jaro (flags and match table in global memory) behind the ownership rule and the length
// window, scored to the end: NO mid-sweep abandon and no bound there.
// Self-join: the plan is the list's own, edit_walk.h's ownership rule walks each unordered pair once, reported as (min, max) --
// which rests on score(a, b) and score(b, a) being the same bits (tests/test_jaro_join_cpu.py holds that).
// The sinks are K18's (k18_sink.h: FuzzAppend -- key = row << 32 | col, the float64 score beside it -- and FuzzUnite on K12's
// forest), the tail behind the join's walk is K18's (score_join_tail); the view, the match-table set / clear, the row classes, the
// launches over them and the general kernel's buffers are edit_walk.h's.
#include "edit_walk.h"
#include "k18_sink.h"
#include "k8_launch.h"
#include "k8_sweep.h"

#include <algorithm>
#include <cmath>
#include <limits.h>

namespace pfz {

struct JaroJoinArgs : JaroWalkArgs {      // (counters: the pairs are those inside the length window)
    const int32_t *len_run;    // [longest from-string + 1][2] the admissible to-lengths [lo, hi] of a from-string of la characters
    double t;
    float t32;                 // t rounded to float32, what the bounds are held against
    int32_t self;
};

// the set-up launch: the run of every from-length and, where a forest is wanted, every position its own root
__global__ __launch_bounds__(256) void k20_begin_kernel(float t32, int32_t winkler, int32_t n_len, int32_t lb_max, int32_t *__restrict__ len_run,
                                                         int32_t n, int32_t *__restrict__ parent)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_len) {
        int lo, hi;
        jaro_len_run((int)i, lb_max, t32, winkler, &lo, &hi);
        len_run[2 * i] = lo;
        len_run[2 * i + 1] = hi;
    }
    if (i < n) parent[i] = (int32_t)i;
}

// the run of groups [lo, hi) of this launch in which a from-string of la characters can have a hit (join_window's shape, the run
// of lengths from the table); the same for every thread of the workgroup
__device__ inline void jaro_window(const JaroJoinArgs &A, bool self, int la, int len_lo, int len_hi, int *lo_out, int *hi_out)
{
    // the first group whose LONGEST string is long enough (a self-join owns nothing shorter than la)
    const int need = self && la > len_lo ? la : len_lo;
    int lo = A.g_begin, hi = A.g_end;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int last = min(A.n_to, (mid + 1) * 64) - 1;
        const int l = __builtin_amdgcn_readfirstlane(A.b_len[last]);
        if (l >= need) hi = mid;
        else lo = mid + 1;
    }
    *lo_out = lo;
    // the first group whose SHORTEST string is too long
    hi = A.g_end;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int l = __builtin_amdgcn_readfirstlane(A.b_len[mid * 64]);
        if (l <= len_hi) lo = mid + 1;
        else hi = mid;
    }
    *hi_out = lo;
}

// WORD, IDB, NB: jaro_pair_above's (k8_sweep.h)
template <typename WORD, int IDB, int NB, typename SINK>
__global__ __launch_bounds__(256) void k20_join_kernel(JaroJoinArgs A, SINK sink)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    WORD *pm = (WORD *)smem_raw;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool self = A.self != 0;

    pm_reg_zero(A, pm, tid, 256);

    JaroWork work;
    for (int r = blockIdx.x; r < A.n_rows; r += gridDim.x) {
        const int row = A.rows[r];
        const int64_t a0 = A.a_off[row];
        const int la = (int)(A.a_off[row + 1] - a0);      // fits the WORD
        const int len_lo = A.len_run[2 * la], len_hi = A.len_run[2 * la + 1];
        int g_lo, g_hi;
        jaro_window(A, self, la, len_lo, len_hi, &g_lo, &g_hi);
        if (g_lo >= g_hi) continue;                       // (the whole workgroup: no table, no barrier)
        const int my_sym = pm_reg_set(A, pm, a0, la, tid);
        const float inv_la = __builtin_amdgcn_rcpf((float)la);

        for (int g = g_lo + wave; g < g_hi; g += 4) {
            const int slot = g * 64 + lane;
            const int orig = A.b_orig[slot];
            const int lb = A.b_len[slot];
            bool alive = join_owned(self, row, la, orig, lb) && lb >= len_lo && lb <= len_hi;
            if (!__any(alive)) continue;
            work.pairs += alive;
            const double sc = jaro_pair_above<WORD, IDB, NB>(A, pm, g, la, lb, inv_la, A.t32, A.winkler, alive, work);
            sink(alive && sc >= A.t, self ? min(row, orig) : row, self ? max(row, orig) : orig, sc);
        }
        __syncthreads();                                  // every wave is done with the match table
        pm_reg_clear(pm, my_sym);
    }
    jaro_work_flush(A.counters, work);
}

// The general case: any lengths, any alphabet.  The match table of the workgroup's from-string (WA words per symbol) and every
// wave's flag words (WA for the from-side, WS for a to-string, 64 lanes each) are in global memory; a lane scores its pair to the
// end with pair_score.h's general Jaro -- no abandon, no bound: the window and the ownership rule are all that is left out.
template <typename SINK>
__global__ __launch_bounds__(256) void k20_join_general_kernel(JaroJoinArgs A, SINK sink, int32_t WA, int32_t WS, uint64_t *__restrict__ pm_all,
                                                                uint64_t *__restrict__ fa_all, uint64_t *__restrict__ fb_all)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool self = A.self != 0;
    const JaroGeneral G = jaro_general_begin(A, WA, WS, pm_all, fa_all, fb_all);
    JaroWork work;
    for (int r = blockIdx.x; r < A.n_rows; r += gridDim.x) {
        const int row = A.rows[r];
        const int64_t a0 = A.a_off[row];
        const int la = (int)(A.a_off[row + 1] - a0);
        const int W = la > 0 ? (la + 63) / 64 : 1;                    // <= WA
        const int len_lo = A.len_run[2 * la], len_hi = A.len_run[2 * la + 1];
        int g_lo, g_hi;
        jaro_window(A, self, la, len_lo, len_hi, &g_lo, &g_hi);
        if (g_lo >= g_hi) continue;
        pm_global_set(A, G.pm, WA, a0, la, tid, 256);
        for (int g = g_lo + wave; g < g_hi; g += 4) {
            const int slot = g * 64 + lane;
            const int orig = A.b_orig[slot];
            const int lb = A.b_len[slot];
            const bool alive = join_owned(self, row, la, orig, lb) && lb >= len_lo && lb <= len_hi;
            if (!__any(alive)) continue;
            work.pairs += alive;
            work.steps += alive ? lb : 0;
            double sc = 0.0;
            if (alive) sc = pair_score_general(G.P, G.pm, G.fa, G.fb, nullptr, WA, W, la, A.t_off[orig], lb);
            sink(alive && sc >= A.t, self ? min(row, orig) : row, self ? max(row, orig) : orig, sc);
        }
        __syncthreads();                                              // every wave is done with the match table
        pm_global_clear(A, G.pm, WA, a0, la, tid, 256);
    }
    work.alive = work.scored = work.pairs;          // scored to the end, every one
    jaro_work_flush(A.counters, work);
}

// The launches of a call on the context's stream: the register kernels over the row classes and their groups (walk_launch), the
// general kernel for the long rows (walk_launch) and for the other rows against the groups of longer to-strings.
template <typename SINK>
static int jaro_join_launch(pfz_ctx *ctx, const pfz_strings *F, const pfz_strings *T, const pfz_indel_plan *pl, JaroJoinArgs &A, const SINK &sink,
                            const char *entry, const char *what, const char *scope_general)
{
    const RowClasses rc = classify_rows(F, 0, F->n, lds_table_fits(pl));      // (a table beyond LDS: every row is the general kernel's)
    DevBuf d_rows[3];
    PFZ_TRY(rows_upload(ctx, rc, d_rows));
    // the groups are sorted by length: the first g32 / g256 of them hold to-strings of <= 32 / <= 256 characters only
    const int32_t n_groups = (int32_t)pl->n_groups;
    const int32_t g32 = whole_groups_up_to(T, pl, 32), g256 = whole_groups_up_to(T, pl, 256);
    const int32_t WS = (int32_t)std::max<int64_t>(1, (T->max_len + 63) / 64);

    auto reg_launch = [&](auto word, auto nb, dim3 grid, int32_t g_begin, int32_t g_end) {
        if (g_begin >= g_end) return;
        A.g_begin = g_begin;
        A.g_end = g_end;
        using WORD = decltype(word);
        constexpr int NB = decltype(nb)::value;
        dispatch_idb(pl->idb, [&](auto IDB) {
            hipLaunchKernelGGL((k20_join_kernel<WORD, decltype(IDB)::value, NB, SINK>), grid, dim3(256), (size_t)A.n_sym1 * sizeof(WORD),
                               ctx->stream, A, sink);
        });
    };
    const int32_t wa_long = (int32_t)((rc.longest + 63) / 64);        // (walk_launch's WA)
    const int32_t ws_cols = (WS + wa_long - 1) / wa_long;
    PFZ_TRY(walk_launch(
        ctx, rc, d_rows, A, {1, ws_cols, 0}, entry, what, scope_general,      // the from-flags; the to-flags, WS words in multiples of WA
        [&](auto word, dim3 grid, size_t) {
            if (sizeof(word) == sizeof(uint32_t)) {
                reg_launch(uint32_t{}, std::integral_constant<int, 1>{}, grid, 0, g32);
                reg_launch(uint64_t{}, std::integral_constant<int, 4>{}, grid, g32, g256);
            }
            else reg_launch(uint64_t{}, std::integral_constant<int, 4>{}, grid, 0, g256);
        },
        [&](dim3 grid, int32_t WA, GeneralBufs &gb) {
            A.g_begin = 0;
            A.g_end = n_groups;
            hipLaunchKernelGGL((k20_join_general_kernel<SINK>), grid, dim3(256), 0, ctx->stream, A, sink, WA, ws_cols * WA, gb.pm.as<uint64_t>(),
                               gb.col[0].as<uint64_t>(), gb.col[1].as<uint64_t>());
        }));
    // the rows of the register kernels against the groups of to-strings beyond 256 characters
    const int64_t max_grid = (int64_t)ctx->prop.multiProcessorCount * 8;
    for (int c = 0; c < 2 && g256 < n_groups; ++c) {
        if (rc.rows[c].empty()) continue;
        A.rows = d_rows[c].as<int32_t>();
        A.n_rows = (int32_t)rc.rows[c].size();
        A.g_begin = g256;
        A.g_end = n_groups;
        int64_t grid = std::min<int64_t>(A.n_rows, max_grid);
        PFZ_TRY(general_grid(&grid, A.n_sym1, 1, entry, what, 64));
        ProfScope ps(ctx, scope_general);
        GeneralBufs gb;
        PFZ_TRY(general_bufs_alloc(ctx, &gb, grid, A.n_sym1, 1, {1, WS, 0}, 256));
        hipLaunchKernelGGL((k20_join_general_kernel<SINK>), dim3((unsigned)grid), dim3(256), 0, ctx->stream, A, sink, 1, WS, gb.pm.as<uint64_t>(),
                           gb.col[0].as<uint64_t>(), gb.col[1].as<uint64_t>());
        PFZ_HIP(hipGetLastError());
    }
    return PFZ_OK;
}

// what both entries do before the walk: limits, the plan, the table of runs (and the forest, every position its own root)
static int jaro_join_begin(pfz_ctx *ctx, const char *entry, const pfz_strings *F, const pfz_strings *T, bool self, int32_t scorer, double t,
                           const pfz_indel_plan **pl, DevBuf *d_run, ForestRun *forest, JaroJoinArgs *A)
{
    PFZ_TRY(jaro_check_limits(entry, F, T));
    PFZ_TRY(indel_plan_get(ctx, T, pl));
    if (forest) PFZ_TRY(forest->alloc(ctx, F->n));
    const int32_t n_len = (int32_t)F->max_len + 1;
    PFZ_TRY(d_run->alloc(ctx, (size_t)n_len * 2 * sizeof(int32_t)));
    const float t32 = (float)t;
    const int32_t n = forest ? forest->n : 0;
    hipLaunchKernelGGL(k20_begin_kernel, dim3((unsigned)((std::max<int64_t>(n_len, n) + 255) / 256)), dim3(256), 0, ctx->stream, t32, scorer,
                       n_len, (int32_t)T->max_len, d_run->as<int32_t>(), n, forest ? forest->parent.as<int32_t>() : nullptr);
    PFZ_HIP(hipGetLastError());
    static_cast<EditView &>(*A) = edit_view(F, *pl);
    A->n_to = (int32_t)T->n;
    A->len_run = d_run->as<int32_t>();
    A->t_chars = T->chars;
    A->t_width = T->char_width;
    A->t_off = T->offsets;
    A->t = t;
    A->t32 = t32;
    A->winkler = scorer;
    A->self = self ? 1 : 0;
    return PFZ_OK;
}

static int jaro_join_run(pfz_ctx *ctx, const pfz_strings *F, const pfz_strings *T, bool self, int32_t scorer, double t, int64_t capacity,
                         int64_t *out_row_ptr, int32_t *out_idx, double *out_sim, int64_t *out_total, int64_t *out_counters)
{
    PFZ_HIP(hipSetDevice(ctx->device));
    *out_total = 0;
    if (out_counters) out_counters[0] = out_counters[1] = out_counters[2] = out_counters[3] = 0;
    const int64_t n_from = F->n, n_to = T->n;
    if (capacity > kFuzzJoinMaxCapacity) {
        set_error("pfz_jaro_join: a capacity of %lld hits exceeds the 2^32 - 1 the sort's payload can number", (long long)capacity);
        return PFZ_ERR_UNSUPPORTED;
    }
    if (n_from == 0 || n_to == 0) {
        for (int64_t r = 0; r <= n_from; ++r) out_row_ptr[r] = 0;
        return PFZ_OK;
    }
    const pfz_indel_plan *pl;
    DevBuf d_run, d_keys, d_score, d_val, d_state;
    JaroJoinArgs A;
    PFZ_TRY(jaro_join_begin(ctx, "pfz_jaro_join", F, T, self, scorer, t, &pl, &d_run, nullptr, &A));
    PFZ_TRY(d_keys.alloc(ctx, (size_t)capacity * sizeof(uint64_t)));
    PFZ_TRY(d_score.alloc(ctx, (size_t)capacity * sizeof(double)));
    PFZ_TRY(d_val.alloc(ctx, (size_t)capacity * sizeof(uint32_t)));
    PFZ_TRY(d_state.alloc(ctx, 5 * sizeof(unsigned long long)));      // the total, then the four counters
    PFZ_HIP(hipMemsetAsync(d_state.p, 0, 5 * sizeof(unsigned long long), ctx->stream));
    unsigned long long *state_dev = d_state.as<unsigned long long>();
    A.counters = out_counters ? state_dev + 1 : nullptr;
    const FuzzAppend sink{state_dev, d_keys.as<uint64_t>(), d_score.as<double>(), d_val.as<uint32_t>(), (unsigned long long)capacity};

    unsigned long long state[5];
    {
        ProfScope ps_all(ctx, "k20_join");
        PFZ_TRY(jaro_join_launch(ctx, F, T, pl, A, sink, "pfz_jaro_join", "a from-string", "k20_join_general"));
        PFZ_TRY(copy_d2h(ctx, state, d_state.p, sizeof(state)));      // (waits for the kernels)
    }
    const int64_t total = (int64_t)state[0];
    *out_total = total;
    if (out_counters)
        for (int k = 0; k < 4; ++k) out_counters[k] = (int64_t)state[k + 1];
    if (total > capacity) return PFZ_OK;       // the caller's buffers stay as they are: it repeats the call with room for `total`
    return score_join_tail(ctx, "k20_sort_unpack", d_keys.as<uint64_t>(), d_val.as<uint32_t>(), d_score.as<double>(), total, n_from,
                           out_row_ptr, out_idx, out_sim);
}

static int jaro_comp_run(pfz_ctx *ctx, const pfz_strings *F, int32_t scorer, double t, int32_t *out_label, int64_t *out_pairs,
                         int64_t *out_components, int64_t *out_counters)
{
    PFZ_HIP(hipSetDevice(ctx->device));
    *out_pairs = *out_components = 0;
    if (out_counters) out_counters[0] = out_counters[1] = out_counters[2] = out_counters[3] = 0;
    const int64_t n = F->n;
    if (n == 0) return PFZ_OK;
    const pfz_indel_plan *pl;
    DevBuf d_run, d_state;
    ForestRun forest;
    JaroJoinArgs A;
    PFZ_TRY(jaro_join_begin(ctx, "pfz_jaro_components", F, F, true, scorer, t, &pl, &d_run, &forest, &A));
    PFZ_TRY(d_state.alloc(ctx, 6 * sizeof(unsigned long long)));      // the hits, the four counters, the roots
    PFZ_HIP(hipMemsetAsync(d_state.p, 0, 6 * sizeof(unsigned long long), ctx->stream));
    unsigned long long *state_dev = d_state.as<unsigned long long>();
    A.counters = out_counters ? state_dev + 1 : nullptr;
    const FuzzUnite sink{state_dev, forest.parent.as<int32_t>()};
    {
        ProfScope ps_all(ctx, "k20_components");
        PFZ_TRY(jaro_join_launch(ctx, F, F, pl, A, sink, "pfz_jaro_components", "a string", "k20_join_general"));
        PFZ_TRY(forest.flatten(ctx, state_dev + 5));
    }
    unsigned long long state[6];
    PFZ_TRY(copy_d2h(ctx, state, d_state.p, sizeof(state)));
    PFZ_TRY(forest.download(ctx, out_label));
    *out_pairs = (int64_t)state[0];
    *out_components = (int64_t)state[5];
    if (out_counters)
        for (int k = 0; k < 4; ++k) out_counters[k] = (int64_t)state[k + 1];
    return PFZ_OK;
}

static int check_jaro_threshold(const char *who, int32_t scorer, double t)
{
    PFZ_TRY(jaro_check_scorer(who, scorer));
    PFZ_REQUIRE(!std::isnan(t) && t >= 0.0 && t <= 1.0, "%s: min_similarity %g is not a number in [0, 1]", who, t);
    return PFZ_OK;
}

}  // namespace pfz

using namespace pfz;

extern "C" {

int pfz_jaro_join(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, int32_t scorer, double min_similarity,
                  int64_t capacity, int64_t *out_row_ptr, int32_t *out_idx, double *out_sim, int64_t *out_total, int64_t *out_counters)
{
    PFZ_REQUIRE(ctx && from_strings, "pfz_jaro_join: NULL argument");
    PFZ_TRY(check_jaro_threshold("pfz_jaro_join", scorer, min_similarity));
    PFZ_REQUIRE(capacity >= 0, "pfz_jaro_join: capacity %lld < 0", (long long)capacity);
    PFZ_REQUIRE(out_row_ptr && out_total, "pfz_jaro_join: NULL out_row_ptr / out_total");
    PFZ_REQUIRE(capacity == 0 || (out_idx && out_sim), "pfz_jaro_join: NULL output with capacity %lld", (long long)capacity);
    const bool self = to_strings == nullptr || to_strings == from_strings;
    return jaro_join_run(ctx, from_strings, self ? from_strings : to_strings, self, scorer, min_similarity, capacity, out_row_ptr, out_idx,
                         out_sim, out_total, out_counters);
}

int pfz_jaro_components(pfz_ctx *ctx, const pfz_strings *strings, int32_t scorer, double min_similarity, int32_t *out_label,
                        int64_t *out_pairs, int64_t *out_components, int64_t *out_counters)
{
    PFZ_REQUIRE(ctx && strings, "pfz_jaro_components: NULL argument");
    PFZ_TRY(check_jaro_threshold("pfz_jaro_components", scorer, min_similarity));
    PFZ_REQUIRE(out_pairs && out_components, "pfz_jaro_components: NULL out_pairs / out_components");
    PFZ_REQUIRE(strings->n == 0 || out_label, "pfz_jaro_components: NULL out_label");
    return jaro_comp_run(ctx, strings, scorer, min_similarity, out_label, out_pairs, out_components, out_counters);
}

}  // extern "C"
