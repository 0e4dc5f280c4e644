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
//   sweep 1      K8's, with the abandon rule once per packed dword: a lane whose matches so far plus the to-characters still to
//                come (or la) are below its pair's m_need is dead; the wave leaves the sweep when no live lane has characters left.
//                Behind it the bound again with the pair's own prefix.
//   sweep 2      for the wave only if a live lane has two matches, left when no live lane has a flagged from-position left; then
//                the bound with t, then the float64 score and the comparison.
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
#include "k8_core.h"
#include "pair_score.h"

#include <algorithm>
#include <cmath>
#include <limits.h>

namespace pfz {

struct JaroJoinArgs : EditView {
    const int32_t *rows;       // from-rows of this launch
    int32_t n_rows;
    int32_t n_to;
    int32_t g_begin, g_end;    // the to-groups of this launch
    const int32_t *len_run;    // [longest from-string + 1][2] the admissible to-lengths [lo, hi] of a from-string of la characters
    const void *t_chars;       // the raw to-list, which the general kernel reads (pair_score.h)
    int32_t t_width;
    const int64_t *t_off;
    double t;
    float t32;                 // t rounded to float32, what the bounds are held against
    int32_t winkler;
    int32_t self;
    unsigned long long *counters;   // optional [4]: pairs inside the length window, pairs alive after sweep 1, pairs scored in
                                    // float64, sweep-1 to-characters of live lanes
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

__device__ inline void jaro_join_count(unsigned long long *counters, unsigned long long w, unsigned long long a, unsigned long long s,
                                       unsigned long long c)
{
    if (!counters) return;
    wave_count(counters + 0, w);
    wave_count(counters + 1, a);
    wave_count(counters + 2, s);
    wave_count(counters + 3, c);
}

// WORD: uint32_t (from-strings of <= 32 characters) or uint64_t (<= 64); NB: to-strings of up to NB words' characters (K8's flag
// registers, walked stretch by stretch with compile-time indices)
template <typename WORD, int IDB, int NB, typename SINK>
__global__ __launch_bounds__(256) void k20_join_kernel(JaroJoinArgs A, SINK sink)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    WORD *pm = (WORD *)smem_raw;
    constexpr int PER = 32 / IDB;  // symbols per dword
    constexpr int SPW = (int)sizeof(WORD) * 8 / PER;      // dwords per stretch
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool self = A.self != 0;

    pm_reg_zero(A, pm, tid, 256);

    unsigned long long n_win = 0, n_alive = 0, n_scored = 0, n_steps = 0;
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
            n_win += alive;
            const float inv_lb = __builtin_amdgcn_rcpf((float)lb);
            const int need = jaro_m_need(la, lb, inv_la, inv_lb, A.t32, A.winkler);
            const int steps = __builtin_amdgcn_readfirstlane(A.g_steps[g]);
            const uint32_t *gp = A.b_packed + A.g_off[g] + lane;
            JaroFlags<WORD> s;
            WORD fb[NB];
            jaro_begin(s, jaro_range(la, lb));
            bool go = true;                               // wave-uniform: a live lane has to-characters left
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                s.fb = 0;
                for (int t = k * SPW; go && t < min(steps, (k + 1) * SPW); ++t) {
                    const uint32_t pk = gp[(int64_t)t * 64];
#pragma unroll
                    for (int q = 0; q < PER; ++q)
                        jaro_match<WORD>(s, pm[__builtin_amdgcn_ubfe(pk, q * IDB, IDB)], t * PER + q, (t - k * SPW) * PER + q);
                    const int done = (t + 1) * PER;       // to-characters behind this lane (its own: min(done, lb))
                    if (alive && done < lb && jaro_dead(la, __popcll((uint64_t)s.fa), lb - done, need)) {
                        alive = false;
                        n_steps += done;
                    }
                    go = __any(alive && done < lb);
                }
                fb[k] = s.fb;
            }
            n_steps += alive ? lb : 0;
            const int m = __popcll((uint64_t)s.fa);
            const int prefix = jaro_prefix(s.pre);
            // the bound from m alone, with the pair's own prefix
            alive = alive && jaro_reaches(m, inv_la, inv_lb, 1.0f, prefix, A.winkler, A.t32);
            n_alive += alive;
            int half_t = 0;
            // (one flagged pair cannot be out of order; the sweep runs for the wave if a single live lane wants it)
            if (__any(alive && m >= 2)) {
                go = true;                                // wave-uniform: a live lane has a flagged from-position left
#pragma unroll
                for (int k = 0; k < NB; ++k) {
                    s.fb = fb[k];
                    for (int t = k * SPW; go && t < min(steps, (k + 1) * SPW); ++t) {
                        const uint32_t pk = gp[(int64_t)t * 64];
#pragma unroll
                        for (int q = 0; q < PER; ++q)
                            half_t += jaro_transpose<WORD>(s, pm[__builtin_amdgcn_ubfe(pk, q * IDB, IDB)], (t - k * SPW) * PER + q);
                        go = __any(alive && s.fa != 0);
                    }
                }
            }
            // the bound again, with t (m = 0: asked before the division's result is)
            const float last = (float)(m - half_t / 2) * __builtin_amdgcn_rcpf((float)m);
            alive = alive && jaro_reaches(m, inv_la, inv_lb, last, prefix, A.winkler, A.t32);
            n_scored += alive;
            const double sc = alive ? jaro_score(m, half_t, la, lb, prefix, A.winkler) : 0.0;
            sink(alive && sc >= A.t, self ? min(row, orig) : row, self ? max(row, orig) : orig, sc);
        }
        __syncthreads();                                  // every wave is done with the match table
        pm_reg_clear(pm, my_sym);
    }
    jaro_join_count(A.counters, n_win, n_alive, n_scored, n_steps);
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
    uint64_t *pm = pm_all + (int64_t)blockIdx.x * A.n_sym1 * WA;      // zero on entry, zero again after every row
    uint64_t *fa = fa_all + ((int64_t)blockIdx.x * 4 + wave) * WA * 64 + lane;      // fa[w * 64]: this lane's word w
    uint64_t *fb = fb_all + ((int64_t)blockIdx.x * 4 + wave) * WS * 64 + lane;
    PairView P;
    static_cast<FromView &>(P) = A;
    P.b_chars = A.t_chars;
    P.b_width = A.t_width;
    P.b_off = A.t_off;
    P.n_to = A.n_to;
    P.scorer = A.winkler ? PAIR_JARO_WINKLER : PAIR_JARO;
    unsigned long long n_win = 0, n_steps = 0;
    for (int r = blockIdx.x; r < A.n_rows; r += gridDim.x) {
        const int row = A.rows[r];
        const int64_t a0 = A.a_off[row];
        const int la = (int)(A.a_off[row + 1] - a0);
        const int W = la > 0 ? (la + 63) / 64 : 1;                    // <= WA
        const int len_lo = A.len_run[2 * la], len_hi = A.len_run[2 * la + 1];
        int g_lo, g_hi;
        jaro_window(A, self, la, len_lo, len_hi, &g_lo, &g_hi);
        if (g_lo >= g_hi) continue;
        pm_global_set(A, pm, WA, a0, la, tid, 256);
        for (int g = g_lo + wave; g < g_hi; g += 4) {
            const int slot = g * 64 + lane;
            const int orig = A.b_orig[slot];
            const int lb = A.b_len[slot];
            const bool alive = join_owned(self, row, la, orig, lb) && lb >= len_lo && lb <= len_hi;
            if (!__any(alive)) continue;
            n_win += alive;
            n_steps += alive ? lb : 0;
            double sc = 0.0;
            if (alive) sc = pair_score_general(P, pm, fa, fb, nullptr, WA, W, la, A.t_off[orig], lb);
            sink(alive && sc >= A.t, self ? min(row, orig) : row, self ? max(row, orig) : orig, sc);
        }
        __syncthreads();                                              // every wave is done with the match table
        pm_global_clear(A, pm, WA, a0, la, tid, 256);
    }
    jaro_join_count(A.counters, n_win, n_win, n_win, n_steps);
}

// The launches of a call on the context's stream: the register kernels over the row classes and their groups (walk_launch), the
// general kernel for the long rows (walk_launch) and for the other rows against the groups of longer to-strings.
template <typename SINK>
static int jaro_join_launch(pfz_ctx *ctx, const pfz_strings *F, const pfz_strings *T, const pfz_indel_plan *pl, JaroJoinArgs &A, const SINK &sink,
                            const char *entry, const char *what, const char *scope_general)
{
    const int64_t n_to = T->n;
    const bool lds_fits = lds_table_fits(pl);
    const RowClasses rc = classify_rows(F, 0, F->n, lds_fits);
    DevBuf d_rows[3];
    PFZ_TRY(rows_upload(ctx, rc, d_rows));
    // the groups are sorted by length: the first g32 / g256 of them hold to-strings of <= 32 / <= 256 characters only
    const int32_t n_groups = (int32_t)pl->n_groups;
    auto whole_groups_up_to = [&](int64_t len) {
        int64_t n = 0;
        for (int64_t j = 0; j < n_to; ++j) n += T->h_off[(size_t)j + 1] - T->h_off[(size_t)j] <= len;
        return n == n_to ? n_groups : (int32_t)(n / 64);
    };
    const int32_t g32 = whole_groups_up_to(32), g256 = whole_groups_up_to(256);
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
    if (T->n >= INT_MAX - 64 || F->n >= INT_MAX || T->max_len >= INT_MAX / 2 || F->max_len >= INT_MAX / 2) {
        set_error("%s: list or string too long", entry);
        return PFZ_ERR_UNSUPPORTED;
    }
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
    PFZ_REQUIRE(scorer == 0 || scorer == 1, "%s: scorer %d is neither 0 (Jaro) nor 1 (Jaro-Winkler)", who, scorer);
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
