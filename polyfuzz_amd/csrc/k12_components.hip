// K12 -- the connected components of "Levenshtein / OSA similarity >= t" over one list (what EditDistance.components runs):
// label[i] = the smallest position j that a chain of pairs with lev_similarity >= t links to i.  The pairs are K11's self-join
// (k11_join.hip), found by the same walk -- K4's plan of the list, one workgroup per from-string with its match table in LDS, one
// lane per to-string, the integer cutoff table kmax[M], the length window, join_abandon, each unordered pair walked once by the
// row the plan's order puts first (k11_core.h, k9_core.h and k4_plan.h, used as they are) -- but a hit is not written anywhere:
// its lane unites the two positions in a union-find forest, parent int32[n] in HBM (k12_core.h), there and then.  No key buffer,
// no capacity, no sort, no CSR, no repeat: device memory is O(n) whatever the number of hits, and what comes to the host is the
// n labels and five counts.
//
// parent inside the walk kernels: every access is an agent-scope atomic -- relaxed loads in the finds, relaxed stores for the
// path halving, compare-and-swap for the hooks; no plain load or store, no fence.  The eight L2s of the part are not coherent with
// each other and a CU's L1 is never refreshed by another CU's stores, so a lane may well read an old parent; k12_core.h argues
// why that costs a failed CAS at most and never a wrong forest.  No lane waits for another.
// The three launches of a call (from-strings of <= 32, of 33 .. 64 characters, the general kernel's) share the one forest, in
// order, on the context's stream.  Behind them, across the kernel boundary, k12_flatten reads the finished forest with plain
// loads: label[i] = root of i, and the roots counted.  The root of a component is its smallest position (k12_core.h), so the
// labels do not depend on the order in which the hooks happened.
// Hits are counted as K11 counts them (one ballot and one atomic add per wave and group), which holds `pairs` to K11's total.
// The walk is the one K11 runs: argument block, window, ownership rule, counters, the general body, the set-up kernel and the
// launches over the row classes are edit_walk.h's, with "no second list" as a compile-time constant and ForestHook as the hit
// sink; the register walk is k11_join_kernel's, written out here with the same two choices (edit_walk.h says why it is not one
// body).  The forest of a components run -- this one's, K13's, K14's, K15's, K16's -- is pfz_internal.h's ForestRun, whose two
// kernels are launched from here.
#include "edit_walk.h"
#include "k12_core.h"

#include <algorithm>
#include <cmath>
#include <limits.h>

namespace pfz {

// WORD: uint32_t (from-strings of <= 32 characters) or uint64_t (<= 64), against to-strings of any length
template <typename WORD, int IDB, bool OSA>
__global__ __launch_bounds__(256) void k12_walk_kernel(CompArgs A)
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
        join_window(A, true, la, &g_lo, &g_hi);
        for (int g = g_lo + wave; g < g_hi; g += 4) {
            const int slot = g * 64 + lane;
            const int orig = A.b_orig[slot];
            const int lb = A.b_len[slot];
            const int km = A.cut[max(la, lb)];
            bool alive = join_owned(true, row, la, orig, lb) && join_in_window(km, la, lb);
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
__global__ __launch_bounds__(256) void k12_walk_general_kernel(CompArgs A, int32_t WA, uint64_t *__restrict__ pm_all,
                                                                uint64_t *__restrict__ vp_all, uint64_t *__restrict__ vn_all,
                                                                uint64_t *__restrict__ d0_all)
{
    walk_general_body<IDB, OSA, false>(A, true, A.sink, WA, pm_all, vp_all, vn_all, d0_all);
}

// after the walk, behind the kernel boundary: label[i] = the root of i's tree, and the roots counted (one atomic per wave)
__global__ __launch_bounds__(256) void k12_flatten(const int32_t *__restrict__ parent, int32_t n, int32_t *__restrict__ label,
                                                    unsigned long long *__restrict__ n_roots)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int32_t root = -1;
    if (i < n) {
        root = uf_root<UfPlainOps>(parent, (int32_t)i);
        label[i] = root;
    }
    const unsigned long long m = __ballot(root == (int32_t)i);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_roots, (unsigned long long)__popcll(m));
}

// K11's and K12's set-up launch (edit_walk.h): the cutoff table and, for n > 0, every position its own root
int lev_walk_begin(pfz_ctx *ctx, double t, int32_t n_kmax, int32_t *kmax, int32_t n, int32_t *parent)
{
    return walk_begin<KmaxByM>(ctx, t, n_kmax, kmax, n, parent);
}

// the two ends of a forest (pfz_internal.h ForestRun): every position its own root, on the context's stream ...
int k12_forest_begin(pfz_ctx *ctx, int32_t n, int32_t *parent) { return lev_walk_begin(ctx, 0.0, 0, nullptr, n, parent); }

// ... and, behind the kernels that hooked, the labels and the number of roots added to *n_roots
int k12_forest_flatten(pfz_ctx *ctx, const int32_t *parent, int32_t n, int32_t *label, unsigned long long *n_roots)
{
    hipLaunchKernelGGL(k12_flatten, dim3((unsigned)(((int64_t)n + 255) / 256)), dim3(256), 0, ctx->stream, parent, n, label, n_roots);
    PFZ_HIP(hipGetLastError());
    return PFZ_OK;
}

static int comp_run(pfz_ctx *ctx, const pfz_strings *F, int32_t scorer, double t, int32_t *out_label, int64_t *out_pairs,
                    int64_t *out_components, int64_t *out_counters)
{
    auto launch = [&](const pfz_indel_plan *pl, const RowClasses &rc, DevBuf (&d_rows)[3], CompArgs &A) {
        return walk_launch(
            ctx, rc, d_rows, A, {1, 1, 1}, "pfz_lev_components", "a string", "k12_walk_general",
            [&](auto word, dim3 grid, size_t lds) {
                dispatch_idb_osa(pl->idb, scorer != 0, [&](auto IDB, auto OSA) {
                    hipLaunchKernelGGL((k12_walk_kernel<decltype(word), decltype(IDB)::value, decltype(OSA)::value>), grid, dim3(256), lds,
                                       ctx->stream, A);
                });
            },
            [&](dim3 grid, int32_t WA, GeneralBufs &gb) {
                dispatch_idb_osa(pl->idb, scorer != 0, [&](auto IDB, auto OSA) {
                    hipLaunchKernelGGL((k12_walk_general_kernel<decltype(IDB)::value, decltype(OSA)::value>), grid, dim3(256), 0, ctx->stream, A,
                                       WA, gb.pm.as<uint64_t>(), gb.col[0].as<uint64_t>(), gb.col[1].as<uint64_t>(), gb.col[2].as<uint64_t>());
                });
            });
    };
    return edit_comp_run(ctx, {"pfz_lev_components", "lengths", "k12_walk", "k12_flatten"}, F, t, F->max_len + 1, lev_walk_begin, launch,
                         out_label, out_pairs, out_components, out_counters);
}

}  // namespace pfz

using namespace pfz;

extern "C" {

int pfz_lev_components(pfz_ctx *ctx, const pfz_strings *strings, int32_t scorer, double min_similarity, int32_t *out_label,
                       int64_t *out_pairs, int64_t *out_components, int64_t *out_counters)
{
    PFZ_REQUIRE(ctx && strings, "pfz_lev_components: NULL argument");
    PFZ_REQUIRE(scorer == 0 || scorer == 1, "pfz_lev_components: scorer %d is neither 0 (Levenshtein) nor 1 (OSA)", scorer);
    PFZ_REQUIRE(!std::isnan(min_similarity) && min_similarity >= 0.0 && min_similarity <= 1.0,
                "pfz_lev_components: min_similarity %g is not a number in [0, 1]", min_similarity);
    PFZ_REQUIRE(out_pairs && out_components, "pfz_lev_components: NULL out_pairs / out_components");
    PFZ_REQUIRE(strings->n == 0 || out_label, "pfz_lev_components: NULL out_label");
    return comp_run(ctx, strings, scorer, min_similarity, out_label, out_pairs, out_components, out_counters);
}

}  // extern "C"
