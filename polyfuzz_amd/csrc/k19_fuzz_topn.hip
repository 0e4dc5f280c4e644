// K19 -- the n best choices of every from-string under the per-pair rapidfuzz scorers (what RapidFuzz.top_n > 1 runs): per row
// the choices not left out whose score is >= score_cutoff, in the order np.argsort(-scores, kind="stable")[:ntop] -- float64
// score descending, equal scores by ascending to-index -- rapidfuzz.process.extract(query, choices, scorer=fuzz.WRatio, limit=n,
// score_cutoff=c) and the six other scorers of K7.  Column 0 at score_cutoff = 0 is pfz_fuzz_extract_one's answer.
//
// A top-n is K18's walk with the floor moving: the kernel and the launches of a call over its three regions are
// k7_join_walk.h (the fast kernel, instances of k7_join_kernel with the sink FuzzTopn) and k7_general.hip (the general kernel's
// third sink); the list of a wave and the merge of a row's lists are topn_wave.h.  Here: the list buffer of a call, the skip
// codes, the one merge, the entry.
//
// The list of a unit is three registers per lane (a double and an int), not LDS: the fast kernel's occupancy is set by its
// registers already (DESIGN.md §4 K19 has the budgets), and an insertion is shuffles between lanes either way.
#include "k7_join_walk.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace pfz {

static int fuzz_topn_run(pfz_ctx *ctx, const pfz_strings *F, const pfz_strings *T, int32_t scorer, const int32_t *skip_idx, int64_t begin,
                         int64_t end, int32_t ntop, double cutoff, int32_t *out_idx, double *out_score, uint64_t *out_counters)
{
    const int64_t n_rows = end - begin;
    if (out_counters) out_counters[0] = out_counters[1] = out_counters[2] = 0;
    if (n_rows == 0) return PFZ_OK;
    if (T->n == 0) {          // no choices: every row is empty, nothing is launched
        std::fill(out_idx, out_idx + n_rows * ntop, -1);
        std::fill(out_score, out_score + n_rows * ntop, 0.0);
        return PFZ_OK;
    }
    PFZ_HIP(hipSetDevice(ctx->device));
    FuzzPrep prep;
    PFZ_TRY(fuzz_prepare(ctx, F, T, scorer, begin, end, &prep));

    DevBuf d_skip, d_lists, d_state, d_oidx, d_oscore;
    int skip_up_to = 0;
    if (skip_idx) {
        std::vector<int32_t> codes(skip_idx, skip_idx + F->n);
        skip_up_to = decode_skip_codes(codes);
        PFZ_REQUIRE(skip_up_to >= 0, "pfz_fuzz_topn: skip_idx mixes single choices (>= 0) and 'up to' codes (<= -2)");
        PFZ_TRY(d_skip.upload(ctx, codes));
    }
    prep.A.skip_idx = skip_idx ? (const int32_t *)d_skip.p : nullptr;
    prep.A.skip_up_to = skip_up_to;

    // the lists of a row: the parts of its fast launch (the largest of the three classes), then the general kernel's
    int32_t max_parts = 1;
    for (int c = 0; c < 3; ++c)
        if (!prep.rows[c].empty()) max_parts = std::max(max_parts, fuzz_parts(ctx, prep.plan, (int64_t)prep.rows[c].size()));
    const int32_t n_lists = max_parts + kTopnGeneralLists;
    const size_t list_bytes = (size_t)n_rows * (size_t)n_lists * (size_t)ntop * sizeof(TopnKey);
    PFZ_TRY(d_lists.alloc(ctx, list_bytes));
    PFZ_HIP(hipMemsetAsync(d_lists.p, 0xff, list_bytes, ctx->stream));      // idx = -1: no entry (topn_wave.h)
    PFZ_TRY(d_state.alloc(ctx, 8 * sizeof(unsigned long long)));            // [1..3] the three counters, [5..] the unit counters
    PFZ_HIP(hipMemsetAsync(d_state.p, 0, 8 * sizeof(unsigned long long), ctx->stream));
    PFZ_TRY(d_oidx.alloc(ctx, (size_t)n_rows * ntop * sizeof(int32_t)));
    PFZ_TRY(d_oscore.alloc(ctx, (size_t)n_rows * ntop * sizeof(double)));
    unsigned long long *state_dev = d_state.as<unsigned long long>();
    prep.A.counters = out_counters ? state_dev + 1 : nullptr;
    const FuzzJoinArgs J{cutoff, 0};
    const FuzzTopn sink{d_lists.as<TopnKey>(), ntop, n_lists, begin, 0};
    {
        ProfScope ps_all(ctx, "k19_topn");
        PFZ_TRY(fuzz_join_launch(ctx, prep, F, T, scorer, J, sink, (int32_t *)(state_dev + 5)));
        PFZ_TRY(topn_merge(d_lists.as<TopnKey>(), n_lists, ntop, nullptr, begin, n_rows, d_oidx.as<int32_t>(), d_oscore.as<double>(), ctx->stream));
    }
    PFZ_TRY(copy_d2h(ctx, out_idx, d_oidx.p, (size_t)n_rows * ntop * sizeof(int32_t)));
    PFZ_TRY(copy_d2h(ctx, out_score, d_oscore.p, (size_t)n_rows * ntop * sizeof(double)));
    if (out_counters) {
        unsigned long long state[4];
        PFZ_TRY(copy_d2h(ctx, state, d_state.p, sizeof(state)));
        for (int k = 0; k < 3; ++k) out_counters[k] = (uint64_t)state[k + 1];
    }
    PFZ_HIP(hipStreamSynchronize(ctx->stream));
    return PFZ_OK;
}

}  // namespace pfz

using namespace pfz;

extern "C" {

int pfz_fuzz_topn(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, int32_t scorer, const int32_t *skip_idx,
                  int64_t from_begin, int64_t from_end, int32_t ntop, double score_cutoff, int32_t *out_idx, double *out_score,
                  uint64_t *out_counters)
{
    PFZ_REQUIRE(ctx && from_strings && to_strings, "pfz_fuzz_topn: NULL argument");
    PFZ_REQUIRE(scorer >= kWRatio && scorer <= kPartialTokenRatio, "pfz_fuzz_topn: unknown scorer %d", scorer);
    PFZ_REQUIRE(from_begin >= 0 && from_begin <= from_end && from_end <= from_strings->n, "pfz_fuzz_topn: row range [%lld,%lld) outside [0,%lld)",
                (long long)from_begin, (long long)from_end, (long long)from_strings->n);
    PFZ_REQUIRE(ntop >= 1, "pfz_fuzz_topn: ntop %d < 1", ntop);
    PFZ_REQUIRE(!std::isnan(score_cutoff) && score_cutoff >= 0.0 && score_cutoff <= 100.0, "pfz_fuzz_topn: score_cutoff %g is not a number in [0, 100]",
                score_cutoff);
    if (ntop > kTopnMax) {
        set_error("pfz_fuzz_topn: ntop %d exceeds the limit of %d (one list entry per lane of a wave)", ntop, kTopnMax);
        return PFZ_ERR_UNSUPPORTED;
    }
    PFZ_REQUIRE(from_end == from_begin || (out_idx && out_score), "pfz_fuzz_topn: NULL output");
    return fuzz_topn_run(ctx, from_strings, to_strings, scorer, skip_idx, from_begin, from_end, ntop, score_cutoff, out_idx, out_score,
                         out_counters);
}

}  // extern "C"
