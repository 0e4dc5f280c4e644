// K21 -- the n best choices of every from-string under Jaro / Jaro-Winkler (what models.JaroWinkler.match(top_n=, min_similarity=)
// runs): per row the choices not left out whose score is >= score_cutoff, in the order np.argsort(-scores, kind="stable")[:ntop] --
// float64 score descending, equal scores by ascending to-index -- rapidfuzz.process.extract(query, choices,
// scorer=JaroWinkler.similarity, limit=n, score_cutoff=c).  The scores are K8's (k8_core.h jaro_score), bit for bit; column 0 at
// score_cutoff = 0 is pfz_jaro_argmax's answer.
//
// K21 is to K20 what K19 is to K18: K20's sweep with the floor moving.
// Mapping to CDNA4 -- K8's and K20's, over K4's to-side plan (k4_plan.h: the to-strings sorted by (length, index) in groups of 64):
//   workgroup (4 waves) = one from-string (or one of the `parts` a row's groups are split into, K8's rule, k8_launch.h) per trip of
//     a persistent loop, its match table PM[symbol] in LDS;  lane = one to-string;  the word classes are K8's.
//   the list     a WAVE keeps one sorted list of its ntop best pairs, entry p in lane p (topn_wave.h), in place of K8's best per
//                lane.  Every wave stores its list, the empty ones too; topn_merge picks the row's top-n.
//   the floor    F = max(score_cutoff, W).  W is a workgroup word in LDS, in front of the match table: the largest last-entry score
//                of any FULL list of its waves (the bits of a non-negative double order as integers: atomicMax by lane 0), reset per
//                row.  A wave reads F once per group and holds the group against (float)F.
//   the walk     K9's: a wave takes its groups from the one nearest |a| outwards, alternately up and down; jaro_len_ok(la, lb,
//                (float)F) is the length bound.  A group none of whose choices still in passes it is skipped; a direction ends at
//                the first group all of whose real strings fail and lie on the far side of |a| -- the admissible lengths are one
//                run around la (k8_core.h), and the run only shrinks as F rises.
//   in a group   k8_sweep.h's jaro_pair_above against (float)F, the function K20 calls with its t: jaro_m_need per pair, jaro_dead
//                once per packed dword with the wave-uniform early exit, jaro_reaches with the pair's own prefix, sweep 2 only if a
//                live lane has two matches, jaro_reaches with t, jaro_score; then score >= score_cutoff, then topn_insert.  Padding
//                lanes, left-out lanes and dead lanes are predicates: all 64 lanes reach topn_insert, and every exit from a group
//                is wave-uniform.
// K8's shortcut "same (m, t, |b|, prefix) as the best: skip" is NOT here: an equal score at a later index belongs in a top-n.
// Everything else -- longer from-strings, the groups beyond 256 characters for every from-string, an alphabet whose table exceeds
// 60 KiB -- takes the general kernel: pair_score.h's general Jaro, every pair not left out scored to the end, no floor.
//
// Why it is exact.  A pair is skipped, abandoned or left unscored only where a k8_core.h rule says it cannot reach (float)F, and
// each rule is false only where jaro_score < F strictly: the bound plus K8_BOUND_MARGIN (1e-4) is >= the float64 score, and the
// rounding of F to float32 (a relative 6e-8) is three orders of magnitude inside that margin.  If F is the cutoff, the pair is not
// reportable.  If F is W, ntop reportable choices with scores >= W > the pair's score sit in one wave's list, so the pair is in no
// top-ntop whatever its index.  A pair that ties F is never dismissed: it is scored and placed by its index.  W only rises, so the
// result does not depend on timing -- only the counters do.  A choice of the row's top-n is in the list of whichever wave walks
// it, so the merge finds it.
//
// The lists of a row.  A from-string of <= 32 characters is served by up to three launches (groups <= 32, groups 33 .. 256, the
// general kernel beyond), each row split over the launch's parts.  The rows of one class (<= 32, 33 .. 64, the general kernel's
// alone) share a list buffer: row r of the class owns n_lists lists of ntop keys, n_lists = 4 waves x the parts of every launch
// that IS made for the class, launch after launch; wave w of part p of a launch writes list list0 + 4 p + w.  A launch that is not
// made contributes no lists, so the merge of a class reads nothing that was not written: there is no memset.
#include "k8_launch.h"
#include "k8_sweep.h"
#include "topn_wave.h"

#include <algorithm>
#include <cmath>
#include <limits.h>

namespace pfz {

struct JaroTopnArgs : JaroWalkArgs {      // (rows: in their class's order; counters: the pairs are the real strings of the groups walked)
    const int32_t *skip_idx;   // [n_from] or NULL (decoded: pfz_internal.h decode_skip_codes)
    int32_t skip_up_to;
    int32_t parts;             // the to-groups of a from-string are split over `parts` workgroups, each with a floor of its own
    int32_t ntop;
    int32_t n_lists, list0;    // wave w of part p of row r (its place in `rows`) leaves its list in
    TopnKey *lists;            // lists[((int64_t)r * n_lists + list0 + 4 * p + w) * ntop]
    double cutoff;
};

constexpr int K21_LDS_HEAD = 16;     // the floor word in front of the match table (which stays 16-byte aligned)

// WORD, IDB, NB: jaro_pair_above's (k8_sweep.h)
template <typename WORD, int IDB, int NB>
__global__ __launch_bounds__(256) void k21_topn_kernel(JaroTopnArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    unsigned long long *wg_floor = (unsigned long long *)smem_raw;
    WORD *pm = (WORD *)(smem_raw + K21_LDS_HEAD);
    constexpr int PER = 32 / IDB;  // symbols per dword
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    pm_reg_zero(A, pm, tid, 256);

    const int parts = A.parts;
    JaroWork work;
    for (int u = blockIdx.x; u < A.n_rows * parts; u += gridDim.x) {
        const int r = u / parts, part = u - r * parts;
        const int row = A.rows[r];
        const int64_t a0 = A.a_off[row];
        const int la = (int)(A.a_off[row + 1] - a0);      // fits the WORD
        // (pm_reg_set, with the workgroup's floor reset in front of its barrier)
        const int my_sym = tid < la ? edit_symbol(A, A.a_chars, A.a_width, a0 + tid) : 0;
        if (my_sym) lds_or(&pm[my_sym], (WORD)1 << tid);
        if (tid == 0) *wg_floor = 0ull;                    // +0.0: no list is full yet
        __syncthreads();

        const int skip = A.skip_idx ? A.skip_idx[row] : -1;
        const float inv_la = __builtin_amdgcn_rcpf((float)la);
        TopnList list = topn_empty();
        // this wave's groups: base + stride * k, k < K (wave-uniform: say so, or the loops below get a per-lane trip count)
        const int base = __builtin_amdgcn_readfirstlane(A.g_begin + wave + 4 * part), stride = 4 * parts;
        const int K = base < A.g_end ? (A.g_end - base + stride - 1) / stride : 0;
        // the first of them whose longest string reaches |a| (g_steps rounds up to whole dwords: near is enough, the walk's ends
        // are decided by the lanes' own lengths)
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
            // the floor of this group: the cutoff, or the last entry of a full list of this workgroup
            const double wb = __longlong_as_double((long long)*(volatile unsigned long long *)wg_floor);
            const float f32 = (float)fmax(A.cutoff, wb);
            const bool len_ok = jaro_len_ok(la, lb, f32, A.winkler);
            bool alive = !out && len_ok;
            if (!__any(alive)) {
                // nothing to gain here; and nothing further out either, once every string of the group -- the left-out ones too --
                // fails and lies on the far side of |a|: the admissible lengths are one run around la
                if (!__any(real && !(!len_ok && (go_up ? lb >= la : lb <= la)))) {
                    if (go_up) up = K;
                    else down = -1;
                }
                continue;
            }
            work.pairs += real;
            const double sc = jaro_pair_above<WORD, IDB, NB>(A, pm, g, la, lb, inv_la, f32, A.winkler, alive, work);
            topn_insert(list, A.ntop, alive && sc >= A.cutoff, sc, orig);
            // a full list: A.ntop reportable choices at or above its last entry's score exist
            double last_score;
            if (topn_full(list, A.ntop, &last_score) && last_score > wb && lane == 0)
                atomicMax(wg_floor, (unsigned long long)__double_as_longlong(last_score));
        }
        topn_store(list, A.ntop, A.lists + (((int64_t)r * A.n_lists + A.list0 + 4 * part + wave)) * A.ntop);
        __syncthreads();                                  // every wave is done with the match table and the floor
        pm_reg_clear(pm, my_sym);
    }
    jaro_work_flush(A.counters, work);
}

// The general case: any lengths, any alphabet.  The match table of the workgroup's from-string (WA words per symbol) and every
// wave's flag words (WA for the from-side, WS for a to-string, 64 lanes each) are in global memory; a lane scores its pair to the
// end with pair_score.h's general Jaro -- no floor, no bound: only the choices left out are not scored.
__global__ __launch_bounds__(256) void k21_topn_general_kernel(JaroTopnArgs A, int32_t WA, int32_t WS, uint64_t *__restrict__ pm_all,
                                                                uint64_t *__restrict__ fa_all, uint64_t *__restrict__ fb_all)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const JaroGeneral G = jaro_general_begin(A, WA, WS, pm_all, fa_all, fb_all);
    const int parts = A.parts;
    JaroWork work;
    for (int u = blockIdx.x; u < A.n_rows * parts; u += gridDim.x) {
        const int r = u / parts, part = u - r * parts;
        const int row = A.rows[r];
        const int64_t a0 = A.a_off[row];
        const int la = (int)(A.a_off[row + 1] - a0);
        const int W = la > 0 ? (la + 63) / 64 : 1;                    // <= WA
        pm_global_set(A, G.pm, WA, a0, la, tid, 256);
        const int skip = A.skip_idx ? A.skip_idx[row] : -1;
        TopnList list = topn_empty();
        for (int g = A.g_begin + wave + 4 * part; g < A.g_end; g += 4 * parts) {
            const int slot = g * 64 + lane;
            const int orig = A.b_orig[slot];
            const int lb = A.b_len[slot];
            const bool have = orig >= 0 && !choice_left_out(orig, skip, A.skip_up_to);
            work.pairs += orig >= 0;
            work.scored += have;
            work.steps += have ? lb : 0;
            double sc = 0.0;
            if (have) sc = pair_score_general(G.P, G.pm, G.fa, G.fb, nullptr, WA, W, la, A.t_off[orig], lb);
            topn_insert(list, A.ntop, have && sc >= A.cutoff, sc, orig);
        }
        topn_store(list, A.ntop, A.lists + (((int64_t)r * A.n_lists + A.list0 + 4 * part + wave)) * A.ntop);
        __syncthreads();                                              // every wave is done with the match table
        pm_global_clear(A, G.pm, WA, a0, la, tid, 256);
    }
    work.alive = work.scored;          // scored to the end, every one not left out
    jaro_work_flush(A.counters, work);
}

static int jaro_topn_run(pfz_ctx *ctx, const pfz_strings *F, const pfz_strings *T, int32_t scorer, const int32_t *skip_idx, int64_t begin,
                         int64_t end, int32_t ntop, double cutoff, int32_t *out_idx, double *out_score, uint64_t *out_counters)
{
    const int64_t n_rows = end - begin;
    if (out_counters) out_counters[0] = out_counters[1] = out_counters[2] = out_counters[3] = 0;
    std::vector<int32_t> codes;
    int skip_up_to = 0;
    if (skip_idx) {
        codes.assign(skip_idx, skip_idx + F->n);
        skip_up_to = decode_skip_codes(codes);
        PFZ_REQUIRE(skip_up_to >= 0, "pfz_jaro_topn: skip_idx mixes single choices (>= 0) and 'up to' codes (<= -2)");
    }
    if (n_rows == 0) return PFZ_OK;
    if (T->n == 0) {          // no choices: every row is empty, nothing is launched
        std::fill(out_idx, out_idx + n_rows * ntop, -1);
        std::fill(out_score, out_score + n_rows * ntop, 0.0);
        return PFZ_OK;
    }
    PFZ_HIP(hipSetDevice(ctx->device));
    PFZ_TRY(jaro_check_limits("pfz_jaro_topn", F, T));
    const pfz_indel_plan *pl;
    PFZ_TRY(indel_plan_get(ctx, T, &pl));
    const JaroPlan plan = jaro_plan(ctx, F, T, pl, begin, end);      // K8's launches (k8_launch.h)

    // The three classes of rows, each with a list buffer of its own: the lists of the launches that are made for it, side by side
    const bool behind = plan.general_behind_reg();
    struct Class { const std::vector<int32_t> *rows; size_t row0, n_rows; int32_t n_lists; } cls[3] = {
        {&plan.rows_reg, 0, plan.n32, 4 * (plan.reg[0].parts + plan.reg[1].parts + (behind ? 1 : 0))},
        {&plan.rows_reg, plan.n32, plan.rows_reg.size() - plan.n32, 4 * (plan.reg[2].parts + (behind ? 1 : 0))},
        {&plan.rows_long, 0, plan.rows_long.size(), 4 * plan.parts_long}};

    DevBuf d_skip, d_rows_reg, d_rows_long, d_lists[3], d_state, d_oidx, d_oscore;
    if (skip_idx) PFZ_TRY(d_skip.upload(ctx, codes));
    if (!plan.rows_reg.empty()) PFZ_TRY(d_rows_reg.upload(ctx, plan.rows_reg));
    if (!plan.rows_long.empty()) PFZ_TRY(d_rows_long.upload(ctx, plan.rows_long));
    for (int c = 0; c < 3; ++c)
        if (cls[c].n_rows) PFZ_TRY(d_lists[c].alloc(ctx, cls[c].n_rows * (size_t)cls[c].n_lists * (size_t)ntop * sizeof(TopnKey)));
    PFZ_TRY(d_state.alloc(ctx, 4 * sizeof(unsigned long long)));
    PFZ_HIP(hipMemsetAsync(d_state.p, 0, 4 * sizeof(unsigned long long), ctx->stream));
    PFZ_TRY(d_oidx.alloc(ctx, (size_t)n_rows * ntop * sizeof(int32_t)));
    PFZ_TRY(d_oscore.alloc(ctx, (size_t)n_rows * ntop * sizeof(double)));
    auto class_rows = [&](int c) { return (c == 2 ? d_rows_long.as<int32_t>() : d_rows_reg.as<int32_t>()) + cls[c].row0; };

    JaroTopnArgs A;
    static_cast<EditView &>(A) = edit_view(F, pl);
    A.n_to = (int32_t)T->n;
    A.skip_idx = skip_idx ? d_skip.as<int32_t>() : nullptr;
    A.skip_up_to = skip_up_to;
    A.winkler = scorer;
    A.ntop = ntop;
    A.cutoff = cutoff;
    A.t_chars = T->chars;
    A.t_width = T->char_width;
    A.t_off = T->offsets;
    A.counters = out_counters ? d_state.as<unsigned long long>() : nullptr;
    const int32_t WS = (int32_t)std::max<int64_t>(1, (T->max_len + 63) / 64);

    // one general launch: the rows of class c against the groups from g_begin on, `parts` parts a row
    auto general_launch = [&](int c, int32_t g_begin, int32_t parts, int32_t list0, int64_t longest) -> int {
        A.rows = class_rows(c);
        A.n_rows = (int32_t)cls[c].n_rows;
        A.g_begin = g_begin;
        A.g_end = plan.n_groups;
        A.parts = parts;
        A.n_lists = cls[c].n_lists;
        A.list0 = list0;
        A.lists = d_lists[c].as<TopnKey>();
        const int32_t WA = (int32_t)((longest + 63) / 64);
        int64_t grid = std::min<int64_t>((int64_t)A.n_rows * parts, plan.max_grid);
        PFZ_TRY(general_grid(&grid, A.n_sym1, WA, "pfz_jaro_topn", "a from-string", longest));
        ProfScope ps(ctx, "k21_jaro_topn_general");
        GeneralBufs gb;      // (col[0]: the from-flags, col[1]: the to-flags)
        PFZ_TRY(general_bufs_alloc(ctx, &gb, grid, A.n_sym1, WA, {WA, WS, 0}, 256));
        hipLaunchKernelGGL(k21_topn_general_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream, A, WA, WS, gb.pm.as<uint64_t>(),
                           gb.col[0].as<uint64_t>(), gb.col[1].as<uint64_t>());
        PFZ_HIP(hipGetLastError());
        return PFZ_OK;
    };
    {
        ProfScope ps_all(ctx, "k21_jaro_topn");
        for (int k = 0; k < 3; ++k) {
            const JaroRegLaunch &L = plan.reg[k];
            if (L.parts == 0) continue;
            const int c = k == 2 ? 1 : 0;
            A.rows = class_rows(c);
            A.n_rows = (int32_t)L.n_rows;
            A.g_begin = L.g_begin;
            A.g_end = L.g_end;
            A.parts = L.parts;
            A.n_lists = cls[c].n_lists;
            A.list0 = 4 * L.slot0;
            A.lists = d_lists[c].as<TopnKey>();
            const dim3 grid((unsigned)std::min<int64_t>((int64_t)A.n_rows * L.parts, plan.max_grid));
            const size_t lds = K21_LDS_HEAD + (size_t)A.n_sym1 * (L.wide ? sizeof(uint64_t) : sizeof(uint32_t));
            dispatch_idb(pl->idb, [&](auto IDB) {
                if (L.wide) hipLaunchKernelGGL((k21_topn_kernel<uint64_t, decltype(IDB)::value, 4>), grid, dim3(256), lds, ctx->stream, A);
                else hipLaunchKernelGGL((k21_topn_kernel<uint32_t, decltype(IDB)::value, 1>), grid, dim3(256), lds, ctx->stream, A);
            });
            PFZ_HIP(hipGetLastError());
        }
        // the general kernel: the rows of the register launches against the groups of longer to-strings (their last list), the
        // other from-strings against every group
        if (behind) {
            if (cls[0].n_rows) PFZ_TRY(general_launch(0, plan.g256, 1, 4 * (plan.reg[0].parts + plan.reg[1].parts), 32));
            if (cls[1].n_rows) PFZ_TRY(general_launch(1, plan.g256, 1, 4 * plan.reg[2].parts, 64));
        }
        if (cls[2].n_rows) PFZ_TRY(general_launch(2, 0, plan.parts_long, 0, plan.longest));
        for (int c = 0; c < 3; ++c)
            if (cls[c].n_rows)
                PFZ_TRY(topn_merge(d_lists[c].as<TopnKey>(), cls[c].n_lists, ntop, class_rows(c), begin, (int64_t)cls[c].n_rows,
                                   d_oidx.as<int32_t>(), d_oscore.as<double>(), ctx->stream));
    }
    PFZ_TRY(copy_d2h(ctx, out_idx, d_oidx.p, (size_t)n_rows * ntop * sizeof(int32_t)));
    PFZ_TRY(copy_d2h(ctx, out_score, d_oscore.p, (size_t)n_rows * ntop * sizeof(double)));
    if (out_counters) {
        unsigned long long state[4];
        PFZ_TRY(copy_d2h(ctx, state, d_state.p, sizeof(state)));
        for (int k = 0; k < 4; ++k) out_counters[k] = (uint64_t)state[k];
    }
    PFZ_HIP(hipStreamSynchronize(ctx->stream));
    return PFZ_OK;
}

}  // namespace pfz

using namespace pfz;

extern "C" {

int pfz_jaro_topn(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, int32_t scorer, const int32_t *skip_idx,
                  int64_t from_begin, int64_t from_end, int32_t ntop, double score_cutoff, int32_t *out_idx, double *out_score,
                  uint64_t *out_counters)
{
    PFZ_REQUIRE(ctx && from_strings && to_strings, "pfz_jaro_topn: NULL argument");
    PFZ_TRY(jaro_check_scorer("pfz_jaro_topn", scorer));
    PFZ_REQUIRE(from_begin >= 0 && from_begin <= from_end && from_end <= from_strings->n, "pfz_jaro_topn: row range [%lld,%lld) outside [0,%lld)",
                (long long)from_begin, (long long)from_end, (long long)from_strings->n);
    PFZ_REQUIRE(ntop >= 1, "pfz_jaro_topn: ntop %d < 1", ntop);
    PFZ_REQUIRE(!std::isnan(score_cutoff) && score_cutoff >= 0.0 && score_cutoff <= 1.0, "pfz_jaro_topn: score_cutoff %g is not a number in [0, 1]",
                score_cutoff);
    if (ntop > kTopnMax) {
        set_error("pfz_jaro_topn: ntop %d exceeds the limit of %d (one list entry per lane of a wave)", ntop, kTopnMax);
        return PFZ_ERR_UNSUPPORTED;
    }
    PFZ_REQUIRE(from_end == from_begin || (out_idx && out_score), "pfz_jaro_topn: NULL output");
    return jaro_topn_run(ctx, from_strings, to_strings, scorer, skip_idx, from_begin, from_end, ntop, score_cutoff, out_idx, out_score,
                         out_counters);
}

}  // extern "C"
