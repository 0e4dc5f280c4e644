// K11 -- all pairs at or above a Levenshtein / OSA similarity threshold (the join EditDistance.join runs): for a float64 t in
// [0, 1], every pair (from i, to j) with lev_similarity(d, |a|, |b|) >= t, as CSR over the from-rows.  The definition, the bit
// logic and the float64 formula of one pair are K9's (k9_core.h), unchanged; what the threshold lets a lane leave out: k11_core.h.
//
// Mapping to CDNA4 -- K9's, on K4's to-side plan (k4_plan.h: the to-strings sorted by (length, index) in groups of 64):
//   workgroup (4 waves) = one from-string, its match table PM[symbol] in LDS, built per from-string and cleared by the positions
//     it set;  lane = one to-string, one step of the Myers / Hyyro recurrence per to-character, 32-bit words for from-strings of
//     <= 32 characters, 64-bit for <= 64, 8- or 16-bit symbols.
// With t known before the first pair, two bounds cut the work, both exact (k11_core.h).  The threshold reaches the kernels as a
// table of integer cutoffs, kmax by M = max(|a|, |b|) (the formula depends on the lengths through M alone), made once per call by
// evaluating the float64 formula: a pair is a hit iff d <= kmax[M], and no lane divides.
//   the window   d >= ||a| - |b||: the to-strings whose length can reach t are a contiguous run of the plan's groups, found by two
//                binary searches per from-string; the waves deal that run's groups among themselves;
//   the walk     a lane whose column's bottom cell, less the characters still to come, exceeds its pair's cutoff kmax is dead;
//                a group whose lanes are all dead or done is left.
// Self-join (no to-list, or the from-list's own handle): the row of the shorter string owns a pair, at equal length the lower
// index -- i.e. the plan's order.  A row's window then begins at its own length and each unordered pair is walked once; it is
// reported as (min, max).
// Output: the lanes of a wave append their hits as one 64-bit key each (k11_core.h: row, to-index, distance) behind one atomic
// counter per wave and group; keys beyond the caller's capacity are counted, never written.  The keys are sorted (sort_u64.hip)
// -- they are distinct, so the order of the appends leaves no trace -- and unpacked into CSR.
// Longer from-strings, and an alphabet whose table exceeds K4's 60 KiB, take the general kernel: words and match table in global
// memory, every group visited, slow.
// The argument block with its hit sink (KeyAppend), the window, the ownership rule, the counters, the whole general walk, the
// cutoff table's and the unpacking's kernels and the host side of a join call are edit_walk.h's, which K12 and K13 use too; here
// are the register walk (K12 has its twin: see edit_walk.h for why it is not one body) and what a call passes to the shared frame.
#include "edit_walk.h"

#include <algorithm>
#include <cmath>
#include <limits.h>

namespace pfz {

// WORD: uint32_t (from-strings of <= 32 characters) or uint64_t (<= 64), against to-strings of any length
template <typename WORD, int IDB, bool OSA>
__global__ __launch_bounds__(256) void k11_join_kernel(JoinArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    WORD *pm = (WORD *)smem_raw;
    constexpr int PER = 32 / IDB;  // symbols per dword
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    pm_reg_zero(A, pm, tid, 256);

    unsigned long long n_win = 0, n_fin = 0, n_steps = 0;
    for (int r = blockIdx.x; r < A.n_rows; r += gridDim.x) {
        const int row = A.rows[r];
        const int64_t a0 = A.a_off[row];
        const int la = (int)(A.a_off[row + 1] - a0);      // fits the WORD
        const int my_sym = pm_reg_set(A, pm, a0, la, tid);

        int g_lo, g_hi;
        join_window(A, A.sink.self != 0, la, &g_lo, &g_hi);
        for (int g = g_lo + wave; g < g_hi; g += 4) {
            const int slot = g * 64 + lane;
            const int orig = A.b_orig[slot];
            const int lb = A.b_len[slot];
            const int km = A.cut[max(la, lb)];
            bool alive = join_owned(A.sink.self != 0, row, la, orig, lb) && join_in_window(km, la, lb);
            if (!__any(alive)) continue;
            n_win += alive;
            const int steps = __builtin_amdgcn_readfirstlane(A.g_steps[g]);
            const uint32_t *gp = A.b_packed + A.g_off[g] + lane;
            LevState<WORD> s;
            lev_begin(s, la);
            for (int t = 0; t < steps; ++t) {
                const uint32_t pk = gp[(int64_t)t * 64];
#pragma unroll
                for (int q = 0; q < PER; ++q)
                    lev_step<WORD, OSA>(s, pm[__builtin_amdgcn_ubfe(pk, q * IDB, IDB)], t * PER + q < lb);
                const int done = (t + 1) * PER;           // to-characters behind this lane (its own: min(done, lb))
                if (alive && done < lb && join_abandon(s.dist, done, lb, km)) {
                    alive = false;
                    n_steps += done;
                }
                if (!__any(alive && done < lb)) break;    // every lane is dead or at its end
            }
            n_fin += alive;
            n_steps += alive ? lb : 0;
            const int d = lev_distance(s.dist, la, lb);
            A.sink(alive && d <= km, row, orig, d);
        }
        __syncthreads();                                  // every wave is done with the match table
        pm_reg_clear(pm, my_sym);
    }
    join_count(A.counters, n_win, n_fin, n_steps);
}

// The general case: any from-length, any alphabet (edit_walk.h walk_general_body)
template <int IDB, bool OSA>
__global__ __launch_bounds__(256) void k11_join_general_kernel(JoinArgs A, int32_t WA, uint64_t *__restrict__ pm_all,
                                                                uint64_t *__restrict__ vp_all, uint64_t *__restrict__ vn_all,
                                                                uint64_t *__restrict__ d0_all)
{
    walk_general_body<IDB, OSA, true>(A, A.sink.self != 0, A.sink, WA, pm_all, vp_all, vn_all, d0_all);
}

static int join_run(pfz_ctx *ctx, const pfz_strings *F, const pfz_strings *T, bool self, int32_t scorer, double t, int64_t capacity,
                    int64_t *out_row_ptr, int32_t *out_idx, int32_t *out_dist, double *out_sim, int64_t *out_total,
                    int64_t *out_counters)
{
    auto launch = [&](const pfz_indel_plan *pl, const RowClasses &rc, DevBuf (&d_rows)[3], JoinArgs &A) {
        return walk_launch(
            ctx, rc, d_rows, A, {1, 1, 1}, "pfz_lev_join", "a from-string", "k11_join_general",
            [&](auto word, dim3 grid, size_t lds) {
                dispatch_idb_osa(pl->idb, scorer != 0, [&](auto IDB, auto OSA) {
                    hipLaunchKernelGGL((k11_join_kernel<decltype(word), decltype(IDB)::value, decltype(OSA)::value>), grid, dim3(256), lds,
                                       ctx->stream, A);
                });
            },
            [&](dim3 grid, int32_t WA, GeneralBufs &gb) {
                dispatch_idb_osa(pl->idb, scorer != 0, [&](auto IDB, auto OSA) {
                    hipLaunchKernelGGL((k11_join_general_kernel<decltype(IDB)::value, decltype(OSA)::value>), grid, dim3(256), 0, ctx->stream, A,
                                       WA, gb.pm.as<uint64_t>(), gb.col[0].as<uint64_t>(), gb.col[1].as<uint64_t>(), gb.col[2].as<uint64_t>());
                });
            });
    };
    // the cutoff of every M = max(|a|, |b|) the two lists allow
    return edit_join_run(ctx, {"pfz_lev_join", "distance", "k11_join", "k11_sort_unpack"}, F, T, self, t, capacity,
                         std::max(F->max_len, T->max_len) + 1, lev_walk_begin, launch, edit_unpack_kernel<LevScore>, out_row_ptr, out_idx,
                         out_dist, out_sim, out_total, out_counters);
}

}  // namespace pfz

using namespace pfz;

extern "C" {

int pfz_lev_join(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, int32_t scorer, double min_similarity,
                 int64_t capacity, int64_t *out_row_ptr, int32_t *out_idx, int32_t *out_dist, double *out_sim, int64_t *out_total,
                 int64_t *out_counters)
{
    PFZ_REQUIRE(ctx && from_strings, "pfz_lev_join: NULL argument");
    PFZ_REQUIRE(scorer == 0 || scorer == 1, "pfz_lev_join: scorer %d is neither 0 (Levenshtein) nor 1 (OSA)", scorer);
    PFZ_REQUIRE(!std::isnan(min_similarity) && min_similarity >= 0.0 && min_similarity <= 1.0,
                "pfz_lev_join: min_similarity %g is not a number in [0, 1]", min_similarity);
    PFZ_REQUIRE(capacity >= 0, "pfz_lev_join: capacity %lld < 0", (long long)capacity);
    PFZ_REQUIRE(out_row_ptr && out_total, "pfz_lev_join: NULL out_row_ptr / out_total");
    PFZ_REQUIRE(capacity == 0 || (out_idx && out_dist && out_sim), "pfz_lev_join: NULL output with capacity %lld", (long long)capacity);
    const bool self = to_strings == nullptr || to_strings == from_strings;
    return join_run(ctx, from_strings, self ? from_strings : to_strings, self, scorer, min_similarity, capacity, out_row_ptr, out_idx,
                    out_dist, out_sim, out_total, out_counters);
}

}  // extern "C"
