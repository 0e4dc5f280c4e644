// K13 -- all pairs at or above an Indel similarity threshold, and the connected components of that relation (what
// EditDistance(scorer="indel").join / .components run): for a float64 t in [0, 1], every pair (from i, to j) with
// indel_similarity(lcs, |a|, |b|) >= t -- rapidfuzz.distance.Indel.normalized_similarity, fuzz.ratio on the 0..1 scale.  The bit
// logic of one pair is K10's (k10_core.h lcs_step_reg / lcs_step_word), unchanged; the float64 formula and what the threshold
// lets a lane leave out: k13_core.h.
//
// Mapping to CDNA4 -- K11's, on K4's to-side plan (k4_plan.h: the to-strings sorted by (length, index) in groups of 64):
//   workgroup (4 waves) = one from-string, its match table PM[symbol] in LDS, built per from-string and cleared by the positions
//     it set;  lane = one to-string, one step of the LCS recurrence (five integer operations on one word) per to-character, 32-bit
//     words for from-strings of <= 32 characters, 64-bit for <= 64, 8- or 16-bit symbols.
// The threshold reaches the kernels as a table of integer cutoffs, lmin by S = |a| + |b| (the formula depends on the lengths
// through S alone), made once per call by evaluating the float64 formula: a pair is a hit iff lcs >= lmin[S], no lane divides.
//   the window   lcs <= min(|a|, |b|): for a from-string of la characters the bound rises with lb up to la and falls beyond it,
//                so the to-strings that can reach t are a contiguous run of the plan's groups around length la, found by two
//                binary searches per from-string; the waves deal that run's groups among themselves;
//   the walk     a lane whose LCS so far plus the to-characters still to come is below its pair's lmin is dead, tested once per
//                packed dword (a bit count of the column); a group whose lanes are all dead or done is left.
// Self-join: K11's ownership rule (edit_walk.h join_owned), unchanged.  Output of the join: K11's -- one 64-bit key per hit
// (k13_core.h: row, to-index, LCS) behind one atomic per wave and group, never past the capacity, sorted (sort_u64.hip), unpacked
// into CSR with d = S - 2 lcs.  Components: a hit lane unites its two positions in K12's forest (k12_core.h) there and then;
// O(n) device memory, no pair is stored.
// Longer from-strings, and an alphabet whose table exceeds K4's 60 KiB, take the general kernel: match table and one column V of
// WA 64-bit words per lane in global memory, the carry chained across the words, every group visited, slow.
// The views, the argument blocks with their hit sinks (KeyAppend for the join, ForestHook for the components), the match-table
// helpers, the ownership rule, the counters, the set-up and unpack kernels (here with indel_lmin by S, and the LCS as the key's
// payload), the launches over the row classes and the host side of a join call are edit_walk.h's, the forest K12's, all used as
// they are.  The window search and the two walks are here and not there: edit_walk.h's carry K9's state and the cutoff by
// max(la, lb) in their signatures.  Both walks take the hit sink as a parameter, so each is written once.  K11 / K12 wrote their
// register walk out twice because a common body
// cost them registers; here the state is one word, and the shared body's instances take 27 .. 44 VGPRs, no scratch (DESIGN.md,
// K13, has the figures; tests/test_indel_join_cpu.py holds them to 64).
#include "edit_walk.h"
#include "k12_core.h"
#include "k13_core.h"

#include <algorithm>
#include <cmath>
#include <limits.h>

namespace pfz {

// the run of groups [lo, hi) a from-string of la characters can have a hit in (join_window's shape, the Indel predicate);
// wave-uniform.  A to-string of la characters is always inside (the bound is 1.0), so the run is around length la.
__device__ inline void indel_window(const WalkArgs &A, bool self, int la, int *lo_out, int *hi_out)
{
    // the first group whose LONGEST string is long enough (a self-join owns nothing shorter than la)
    int lo = 0, hi = A.n_groups;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int last = min(A.n_to, (mid + 1) * 64) - 1;
        const int l = __builtin_amdgcn_readfirstlane(A.b_len[last]);
        if (l >= la || (!self && indel_in_window(A.cut[la + l], la, l))) hi = mid;
        else lo = mid + 1;
    }
    *lo_out = lo;
    // the first group whose SHORTEST string is too long
    hi = A.n_groups;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int l = __builtin_amdgcn_readfirstlane(A.b_len[mid * 64]);
        if (l <= la || indel_in_window(A.cut[la + l], la, l)) lo = mid + 1;
        else hi = mid;
    }
    *hi_out = lo;
}

// The register walk.  WORD: uint32_t (from-strings of <= 32 characters) or uint64_t (<= 64), against to-strings of any length.
// The padding behind a lane's end is symbol 0, whose table entry is empty: it leaves V as it is.
template <typename WORD, int IDB, bool TWO_LISTS, typename SINK>
__device__ __forceinline__ void indel_walk_reg_body(const WalkArgs &A, bool self_arg, const SINK &sink)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    WORD *pm = (WORD *)smem_raw;
    constexpr int PER = 32 / IDB;  // symbols per dword
    const bool self = !TWO_LISTS || self_arg;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    pm_reg_zero(A, pm, tid, 256);

    unsigned long long n_win = 0, n_fin = 0, n_steps = 0;
    for (int r = blockIdx.x; r < A.n_rows; r += gridDim.x) {
        const int row = A.rows[r];
        const int64_t a0 = A.a_off[row];
        const int la = (int)(A.a_off[row + 1] - a0);      // fits the WORD
        const int my_sym = pm_reg_set(A, pm, a0, la, tid);

        int g_lo, g_hi;
        indel_window(A, self, la, &g_lo, &g_hi);
        for (int g = g_lo + wave; g < g_hi; g += 4) {
            const int slot = g * 64 + lane;
            const int orig = A.b_orig[slot];
            const int lb = A.b_len[slot];
            const int lm = A.cut[la + lb];
            bool alive = join_owned(self, row, la, orig, lb) && indel_in_window(lm, la, lb);
            if (!__any(alive)) continue;
            n_win += alive;
            const int steps = __builtin_amdgcn_readfirstlane(A.g_steps[g]);
            const uint32_t *gp = A.b_packed + A.g_off[g] + lane;
            WORD v = (WORD)~(WORD)0;
            for (int t = 0; t < steps; ++t) {
                const uint32_t pk = gp[(int64_t)t * 64];
#pragma unroll
                for (int q = 0; q < PER; ++q) lcs_step_reg<WORD>(v, pm[__builtin_amdgcn_ubfe(pk, q * IDB, IDB)]);
                const int done = (t + 1) * PER;           // to-characters behind this lane (its own: min(done, lb))
                if (alive && done < lb && indel_abandon(indel_lcs_of(v, la), done, lb, lm)) {
                    alive = false;
                    n_steps += done;
                }
                if (!__any(alive && done < lb)) break;    // every lane is dead or at its end
            }
            n_fin += alive;
            n_steps += alive ? lb : 0;
            const int lcs = indel_lcs_of(v, la);
            sink(alive && lcs >= lm, row, orig, lcs);
        }
        __syncthreads();                                  // every wave is done with the match table
        pm_reg_clear(pm, my_sym);
    }
    join_count(A.counters, n_win, n_fin, n_steps);
}

// The general walk: any from-length, any alphabet.  The match table of the workgroup's from-string (WA words per symbol) and
// every lane's column V (WA words) are in global memory; every group is visited, a lane walks its own to-string alone and stops
// where it is dead (the test, as above, once per packed dword: it reads the column again to count its zero bits).
template <int IDB, bool TWO_LISTS, typename SINK>
__device__ __forceinline__ void indel_walk_general_body(const WalkArgs &A, bool self_arg, const SINK &sink, int32_t WA,
                                                        uint64_t *__restrict__ pm_all, uint64_t *__restrict__ v_all)
{
    constexpr int PER = 32 / IDB;
    const bool self = !TWO_LISTS || self_arg;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t *pm = pm_all + (int64_t)blockIdx.x * A.n_sym1 * WA;      // zero on entry, zero again after every row
    uint64_t *v = v_all + (int64_t)blockIdx.x * WA * 256 + tid;       // v[w * 256]: this lane's word w
    unsigned long long n_win = 0, n_fin = 0, n_steps = 0;
    for (int r = blockIdx.x; r < A.n_rows; r += gridDim.x) {
        const int row = A.rows[r];
        const int64_t a0 = A.a_off[row];
        const int la = (int)(A.a_off[row + 1] - a0);
        const int W = la > 0 ? (la + 63) / 64 : 1;                    // <= WA
        pm_global_set(A, pm, WA, a0, la, tid, 256);
        for (int g = wave; g < A.n_groups; g += 4) {
            const int slot = g * 64 + lane;
            const int orig = A.b_orig[slot];
            const int lb = A.b_len[slot];
            const int lm = A.cut[la + lb];
            bool alive = join_owned(self, row, la, orig, lb) && indel_in_window(lm, la, lb);
            if (!__any(alive)) continue;
            n_win += alive;
            int lcs = 0;
            if (alive) {
                const uint32_t *gp = A.b_packed + A.g_off[g] + lane;
                for (int w = 0; w < W; ++w) v[(int64_t)w * 256] = ~0ull;
                for (int j = 0; j < lb; ++j) {
                    const uint32_t pk = gp[(int64_t)(j / PER) * 64];
                    const uint32_t c = (pk >> ((j % PER) * IDB)) & ((1u << IDB) - 1u);
                    const uint64_t *eq = pm + (int64_t)c * WA;
                    uint64_t carry = 0;
                    for (int w = 0; w < W; ++w) {
                        uint64_t x = v[(int64_t)w * 256];
                        lcs_step_word(x, eq[w], carry);
                        v[(int64_t)w * 256] = x;
                    }
                    if ((j + 1) % PER == 0 && j + 1 < lb) {
                        int l_j = 0;
                        for (int w = 0; w < W; ++w) l_j += indel_lcs_of(v[(int64_t)w * 256], la - 64 * w);
                        if (indel_abandon(l_j, j + 1, lb, lm)) {
                            alive = false;
                            n_steps += j + 1;
                            break;
                        }
                    }
                }
                if (alive)
                    for (int w = 0; w < W; ++w) lcs += indel_lcs_of(v[(int64_t)w * 256], la - 64 * w);
            }
            n_fin += alive;
            n_steps += alive ? lb : 0;
            sink(alive && lcs >= lm, row, orig, lcs);
        }
        __syncthreads();                                              // every wave is done with the match table
        pm_global_clear(A, pm, WA, a0, la, tid, 256);
    }
    join_count(A.counters, n_win, n_fin, n_steps);
}

template <typename WORD, int IDB>
__global__ __launch_bounds__(256) void k13_join_kernel(JoinArgs A)
{
    indel_walk_reg_body<WORD, IDB, true>(A, A.sink.self != 0, A.sink);
}

template <typename WORD, int IDB>
__global__ __launch_bounds__(256) void k13_comp_kernel(CompArgs A)
{
    indel_walk_reg_body<WORD, IDB, false>(A, true, A.sink);
}

template <int IDB>
__global__ __launch_bounds__(256) void k13_join_general_kernel(JoinArgs A, int32_t WA, uint64_t *__restrict__ pm_all,
                                                                uint64_t *__restrict__ v_all)
{
    indel_walk_general_body<IDB, true>(A, A.sink.self != 0, A.sink, WA, pm_all, v_all);
}

template <int IDB>
__global__ __launch_bounds__(256) void k13_comp_general_kernel(CompArgs A, int32_t WA, uint64_t *__restrict__ pm_all,
                                                                uint64_t *__restrict__ v_all)
{
    indel_walk_general_body<IDB, false>(A, true, A.sink, WA, pm_all, v_all);
}

// the cutoff of every S = |a| + |b| the two lists allow (the formula evaluated around a guess, k13_core.h)
struct LminByS {
    __device__ static int at(double t, int s) { return indel_lmin(t, s); }
};

// a key's payload, the LCS, as the join reports it: d = S - 2 lcs and the similarity of the definition
struct IndelScore {
    __device__ static int distance(int lcs, int la, int lb) { return indel_distance(lcs, la, lb); }
    __device__ static double similarity(int lcs, int la, int lb) { return indel_similarity(lcs, la, lb); }
};

static int indel_join_run(pfz_ctx *ctx, const pfz_strings *F, const pfz_strings *T, bool self, double t, int64_t capacity,
                          int64_t *out_row_ptr, int32_t *out_idx, int32_t *out_dist, double *out_sim, int64_t *out_total,
                          int64_t *out_counters)
{
    auto launch = [&](const pfz_indel_plan *pl, const RowClasses &rc, DevBuf (&d_rows)[3], JoinArgs &A) {
        return walk_launch(
            ctx, rc, d_rows, A, {1, 0, 0}, "pfz_indel_join", "a from-string", "k13_join_general",      // one column, V
            [&](auto word, dim3 grid, size_t lds) {
                dispatch_idb(pl->idb, [&](auto IDB) {
                    hipLaunchKernelGGL((k13_join_kernel<decltype(word), decltype(IDB)::value>), grid, dim3(256), lds, ctx->stream, A);
                });
            },
            [&](dim3 grid, int32_t WA, GeneralBufs &gb) {
                dispatch_idb(pl->idb, [&](auto IDB) {
                    hipLaunchKernelGGL((k13_join_general_kernel<decltype(IDB)::value>), grid, dim3(256), 0, ctx->stream, A, WA,
                                       gb.pm.as<uint64_t>(), gb.col[0].as<uint64_t>());
                });
            });
    };
    return edit_join_run(ctx, {"pfz_indel_join", "LCS", "k13_join", "k13_sort_unpack"}, F, T, self, t, capacity, F->max_len + T->max_len + 1,
                         walk_begin<LminByS>, launch, edit_unpack_kernel<IndelScore>, out_row_ptr, out_idx, out_dist, out_sim, out_total,
                         out_counters);
}

static int indel_comp_run(pfz_ctx *ctx, const pfz_strings *F, double t, int32_t *out_label, int64_t *out_pairs, int64_t *out_components,
                          int64_t *out_counters)
{
    auto launch = [&](const pfz_indel_plan *pl, const RowClasses &rc, DevBuf (&d_rows)[3], CompArgs &A) {
        return walk_launch(
            ctx, rc, d_rows, A, {1, 0, 0}, "pfz_indel_components", "a string", "k13_comp_general",      // one column, V
            [&](auto word, dim3 grid, size_t lds) {
                dispatch_idb(pl->idb, [&](auto IDB) {
                    hipLaunchKernelGGL((k13_comp_kernel<decltype(word), decltype(IDB)::value>), grid, dim3(256), lds, ctx->stream, A);
                });
            },
            [&](dim3 grid, int32_t WA, GeneralBufs &gb) {
                dispatch_idb(pl->idb, [&](auto IDB) {
                    hipLaunchKernelGGL((k13_comp_general_kernel<decltype(IDB)::value>), grid, dim3(256), 0, ctx->stream, A, WA,
                                       gb.pm.as<uint64_t>(), gb.col[0].as<uint64_t>());
                });
            });
    };
    return edit_comp_run(ctx, {"pfz_indel_components", "the sum of two lengths", "k13_comp", "k13_flatten"}, F, t, 2 * F->max_len + 1,
                         walk_begin<LminByS>, launch, out_label, out_pairs, out_components, out_counters);
}

}  // namespace pfz

using namespace pfz;

extern "C" {

int pfz_indel_join(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, double min_similarity, int64_t capacity,
                   int64_t *out_row_ptr, int32_t *out_idx, int32_t *out_dist, double *out_sim, int64_t *out_total, int64_t *out_counters)
{
    PFZ_REQUIRE(ctx && from_strings, "pfz_indel_join: NULL argument");
    PFZ_REQUIRE(!std::isnan(min_similarity) && min_similarity >= 0.0 && min_similarity <= 1.0,
                "pfz_indel_join: min_similarity %g is not a number in [0, 1]", min_similarity);
    PFZ_REQUIRE(capacity >= 0, "pfz_indel_join: capacity %lld < 0", (long long)capacity);
    PFZ_REQUIRE(out_row_ptr && out_total, "pfz_indel_join: NULL out_row_ptr / out_total");
    PFZ_REQUIRE(capacity == 0 || (out_idx && out_dist && out_sim), "pfz_indel_join: NULL output with capacity %lld", (long long)capacity);
    const bool self = to_strings == nullptr || to_strings == from_strings;
    return indel_join_run(ctx, from_strings, self ? from_strings : to_strings, self, min_similarity, capacity, out_row_ptr, out_idx,
                          out_dist, out_sim, out_total, out_counters);
}

int pfz_indel_components(pfz_ctx *ctx, const pfz_strings *strings, double min_similarity, int32_t *out_label, int64_t *out_pairs,
                         int64_t *out_components, int64_t *out_counters)
{
    PFZ_REQUIRE(ctx && strings, "pfz_indel_components: NULL argument");
    PFZ_REQUIRE(!std::isnan(min_similarity) && min_similarity >= 0.0 && min_similarity <= 1.0,
                "pfz_indel_components: min_similarity %g is not a number in [0, 1]", min_similarity);
    PFZ_REQUIRE(out_pairs && out_components, "pfz_indel_components: NULL out_pairs / out_components");
    PFZ_REQUIRE(strings->n == 0 || out_label, "pfz_indel_components: NULL out_label");
    return indel_comp_run(ctx, strings, min_similarity, out_label, out_pairs, out_components, out_counters);
}

}  // extern "C"
