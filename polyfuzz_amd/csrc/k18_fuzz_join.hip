// K18 -- all pairs at or above a score of the per-pair rapidfuzz scorers, and the connected components of that relation (what
// RapidFuzz.join / .components run): for a float64 cutoff on rapidfuzz's 0..100 scale, every pair (from i, to j) with
// scorer(from[i], to[j]) >= cutoff -- rapidfuzz.process.cdist(..., score_cutoff=c) / process.extract(..., limit=None,
// score_cutoff=c) under fuzz.WRatio (the default scorer of the reference's RapidFuzz matcher, _rapidfuzz.py:99-113) and the six
// other scorers of K7.  The arithmetic of one pair -- the exact score fz_score, its float32 upper bound fz_upper_bound -- is K7's
// (k7_core.h), unchanged; the hit rule, the prune rule and the packed hit are k18_core.h; the sinks k18_sink.h.
//
// A fixed threshold is the easy case for K7's machinery: the floor `cur` a pair is bounded and scored against never moves, so
// there are no seeds, no bound cache, no shared running best, no continuation units -- and no wave ever waits for another
// workgroup.
//
// The kernel -- K7's mapping to CDNA4, one walk that bounds, queues and scores the pairs of a unit and hands the hits to a sink --
// and the launches of a call over its three regions are k7_join_walk.h, shared with the top-n form (k19_fuzz_topn.hip).  Here: the
// join's sort and unpack, the components' forest frame, the two entries.
//
// Output of the join: key = row << 32 | to-index, the float64 score and the position itself at the hit's position of three
// parallel arrays, never past the capacity; the keys sorted with the positions as payload (sort_u64.hip), unpacked into CSR with
// the scores gathered through the payload.  The keys are distinct: the order of the appends leaves no trace.
#include "k7_join_walk.h"
#include "k11_core.h"

#include <algorithm>
#include <climits>
#include <cmath>

namespace pfz {

// the sorted keys -> CSR: hit p of the row-major order, its score gathered through the payload, and its share of the row pointers
__global__ __launch_bounds__(256) void k18_unpack(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                   const double *__restrict__ score, int64_t total, int64_t n_from,
                                                   int64_t *__restrict__ row_ptr, int32_t *__restrict__ out_idx, double *__restrict__ out_score)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= total) return;
    out_idx[p] = fuzz_key_col(keys[p]);
    out_score[p] = score[vals[p]];
    rows_fill(p > 0 ? (int64_t)fuzz_key_row(keys[p - 1]) : -1, (int64_t)fuzz_key_row(keys[p]), p, total, n_from, row_ptr);
}

// behind the walk of a join that appended through FuzzAppend (here and K20, k20_jaro_join.hip): pfz_internal.h has the contract
int score_join_tail(pfz_ctx *ctx, const char *scope, const uint64_t *d_keys, const uint32_t *d_val, const double *d_score, int64_t total,
                    int64_t n_from, int64_t *out_row_ptr, int32_t *out_idx, double *out_score)
{
    if (total == 0) {
        for (int64_t r = 0; r <= n_from; ++r) out_row_ptr[r] = 0;
        return PFZ_OK;
    }
    DevBuf d_skeys, d_svals, d_ptr, d_idx, d_out;
    {
        ProfScope ps(ctx, scope);
        const size_t cap = (size_t)sort_codes_capacity(total);
        PFZ_TRY(d_skeys.alloc(ctx, cap * sizeof(uint64_t)));
        PFZ_TRY(d_svals.alloc(ctx, cap * sizeof(uint32_t)));
        PFZ_TRY(sort_pairs_u64(ctx, d_keys, d_val, d_skeys.as<uint64_t>(), d_svals.as<uint32_t>(), total));
        PFZ_TRY(d_ptr.alloc(ctx, (size_t)(n_from + 1) * sizeof(int64_t)));
        PFZ_TRY(d_idx.alloc(ctx, (size_t)total * sizeof(int32_t)));
        PFZ_TRY(d_out.alloc(ctx, (size_t)total * sizeof(double)));
        hipLaunchKernelGGL(k18_unpack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, d_skeys.as<uint64_t>(),
                           d_svals.as<uint32_t>(), d_score, total, n_from, d_ptr.as<int64_t>(), d_idx.as<int32_t>(), d_out.as<double>());
        PFZ_HIP(hipGetLastError());
    }
    PFZ_TRY(copy_d2h(ctx, out_row_ptr, d_ptr.p, (size_t)(n_from + 1) * sizeof(int64_t)));
    PFZ_TRY(copy_d2h(ctx, out_idx, d_idx.p, (size_t)total * sizeof(int32_t)));
    PFZ_TRY(copy_d2h(ctx, out_score, d_out.p, (size_t)total * sizeof(double)));
    PFZ_HIP(hipStreamSynchronize(ctx->stream));
    return PFZ_OK;
}

static int fuzz_join_run(pfz_ctx *ctx, const pfz_strings *F, const pfz_strings *T, bool self, int32_t scorer, double cutoff,
                         int64_t capacity, int64_t *out_row_ptr, int32_t *out_idx, double *out_score, int64_t *out_total,
                         int64_t *out_counters)
{
    PFZ_HIP(hipSetDevice(ctx->device));
    *out_total = 0;
    if (out_counters) out_counters[0] = out_counters[1] = out_counters[2] = 0;
    const int64_t n_from = F->n, n_to = T->n;
    if (capacity > kFuzzJoinMaxCapacity) {
        set_error("pfz_fuzz_join: a capacity of %lld hits exceeds the 2^32 - 1 the sort's payload can number", (long long)capacity);
        return PFZ_ERR_UNSUPPORTED;
    }
    if (n_from == 0 || n_to == 0) {
        for (int64_t r = 0; r <= n_from; ++r) out_row_ptr[r] = 0;
        return PFZ_OK;
    }
    FuzzPrep prep;
    PFZ_TRY(fuzz_prepare(ctx, F, T, scorer, 0, n_from, &prep));

    DevBuf d_keys, d_score, d_val, d_state;
    PFZ_TRY(d_keys.alloc(ctx, (size_t)capacity * sizeof(uint64_t)));
    PFZ_TRY(d_score.alloc(ctx, (size_t)capacity * sizeof(double)));
    PFZ_TRY(d_val.alloc(ctx, (size_t)capacity * sizeof(uint32_t)));
    PFZ_TRY(d_state.alloc(ctx, 8 * sizeof(unsigned long long)));      // the total, the three counters (a fourth word unused), the unit counters
    PFZ_HIP(hipMemsetAsync(d_state.p, 0, 8 * sizeof(unsigned long long), ctx->stream));
    unsigned long long *state_dev = d_state.as<unsigned long long>();
    prep.A.counters = out_counters ? state_dev + 1 : nullptr;
    const FuzzJoinArgs J{cutoff, self ? 1 : 0};
    const FuzzAppend sink{state_dev, d_keys.as<uint64_t>(), d_score.as<double>(), d_val.as<uint32_t>(), (unsigned long long)capacity};

    unsigned long long state[4];
    {
        ProfScope ps_all(ctx, "k18_join");
        PFZ_TRY(fuzz_join_launch(ctx, prep, F, T, scorer, J, sink, (int32_t *)(state_dev + 5)));
        PFZ_TRY(copy_d2h(ctx, state, d_state.p, sizeof(state)));      // (waits for the kernels)
    }
    const int64_t total = (int64_t)state[0];
    *out_total = total;
    if (out_counters)
        for (int k = 0; k < 3; ++k) out_counters[k] = (int64_t)state[k + 1];
    if (total > capacity) return PFZ_OK;       // the caller's buffers stay as they are: it repeats the call with room for `total`
    return score_join_tail(ctx, "k18_sort_unpack", d_keys.as<uint64_t>(), d_val.as<uint32_t>(), d_score.as<double>(), total, n_from,
                           out_row_ptr, out_idx, out_score);
}

static int fuzz_comp_run(pfz_ctx *ctx, const pfz_strings *F, int32_t scorer, double cutoff, int32_t *out_label, int64_t *out_pairs,
                         int64_t *out_components, int64_t *out_counters)
{
    PFZ_HIP(hipSetDevice(ctx->device));
    *out_pairs = *out_components = 0;
    if (out_counters) out_counters[0] = out_counters[1] = out_counters[2] = 0;
    const int64_t n = F->n;
    if (n == 0) return PFZ_OK;
    FuzzPrep prep;
    PFZ_TRY(fuzz_prepare(ctx, F, F, scorer, 0, n, &prep));

    DevBuf d_state;
    ForestRun forest;
    PFZ_TRY(forest.alloc(ctx, n));
    PFZ_TRY(d_state.alloc(ctx, 8 * sizeof(unsigned long long)));      // the hits, the three counters, the roots, the unit counters
    PFZ_HIP(hipMemsetAsync(d_state.p, 0, 8 * sizeof(unsigned long long), ctx->stream));
    PFZ_TRY(forest.begin(ctx));
    unsigned long long *state_dev = d_state.as<unsigned long long>();
    prep.A.counters = out_counters ? state_dev + 1 : nullptr;
    const FuzzJoinArgs J{cutoff, 1};
    const FuzzUnite sink{state_dev, forest.parent.as<int32_t>()};
    {
        ProfScope ps_all(ctx, "k18_comp");
        PFZ_TRY(fuzz_join_launch(ctx, prep, F, F, scorer, J, sink, (int32_t *)(state_dev + 5)));
    }
    {
        ProfScope ps(ctx, "k18_flatten");
        PFZ_TRY(forest.flatten(ctx, state_dev + 4));
    }
    unsigned long long state[5];
    PFZ_TRY(copy_d2h(ctx, state, d_state.p, sizeof(state)));
    PFZ_TRY(forest.download(ctx, out_label));
    *out_pairs = (int64_t)state[0];
    *out_components = (int64_t)state[4];
    if (out_counters)
        for (int k = 0; k < 3; ++k) out_counters[k] = (int64_t)state[k + 1];
    return PFZ_OK;
}

static int check_threshold(const char *who, int32_t scorer, double cutoff)
{
    PFZ_REQUIRE(scorer >= kWRatio && scorer <= kPartialTokenRatio, "%s: unknown scorer %d", who, scorer);
    PFZ_REQUIRE(!std::isnan(cutoff) && cutoff >= 0.0 && cutoff <= 100.0, "%s: score_cutoff %g is not a number in [0, 100]", who, cutoff);
    return PFZ_OK;
}

}  // namespace pfz

using namespace pfz;

extern "C" {

int pfz_fuzz_join(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, int32_t scorer, double score_cutoff,
                  int64_t capacity, int64_t *out_row_ptr, int32_t *out_idx, double *out_score, int64_t *out_total, int64_t *out_counters)
{
    PFZ_REQUIRE(ctx && from_strings, "pfz_fuzz_join: NULL argument");
    PFZ_TRY(check_threshold("pfz_fuzz_join", scorer, score_cutoff));
    PFZ_REQUIRE(capacity >= 0, "pfz_fuzz_join: capacity %lld < 0", (long long)capacity);
    PFZ_REQUIRE(out_row_ptr && out_total, "pfz_fuzz_join: NULL out_row_ptr / out_total");
    PFZ_REQUIRE(capacity == 0 || (out_idx && out_score), "pfz_fuzz_join: NULL output with capacity %lld", (long long)capacity);
    const bool self = to_strings == nullptr || to_strings == from_strings;
    return fuzz_join_run(ctx, from_strings, self ? from_strings : to_strings, self, scorer, score_cutoff, capacity, out_row_ptr, out_idx,
                         out_score, out_total, out_counters);
}

int pfz_fuzz_components(pfz_ctx *ctx, const pfz_strings *strings, int32_t scorer, double score_cutoff, int32_t *out_label,
                        int64_t *out_pairs, int64_t *out_components, int64_t *out_counters)
{
    PFZ_REQUIRE(ctx && strings, "pfz_fuzz_components: NULL argument");
    PFZ_TRY(check_threshold("pfz_fuzz_components", scorer, score_cutoff));
    PFZ_REQUIRE(out_pairs && out_components, "pfz_fuzz_components: NULL out_pairs / out_components");
    PFZ_REQUIRE(strings->n == 0 || out_label, "pfz_fuzz_components: NULL out_label");
    return fuzz_comp_run(ctx, strings, scorer, score_cutoff, out_label, out_pairs, out_components, out_counters);
}

}  // extern "C"
