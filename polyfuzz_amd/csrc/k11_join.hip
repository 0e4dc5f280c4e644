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
// The argument block, the window, the ownership rule, the counters and the whole general walk are edit_walk.h's, which K12 uses
// too; here are the hit sink (JoinAppend), the register walk (K12 has its twin: see edit_walk.h for why it is not one body), the
// cutoff table, the unpacking and the host side.
#include "edit_walk.h"

#include <algorithm>
#include <cmath>
#include <limits.h>

namespace pfz {

struct JoinArgs : WalkArgs {
    int32_t self;              // self-join: the plan is the from-list's own
    uint64_t *keys;            // [capacity] the hits, in the order the waves got there
    unsigned long long capacity;
};

// the walk's hit sink: the hits of one wave and group behind one atomic for all of them, written while there is room
struct JoinAppend {
    const JoinArgs &A;
    __device__ void operator()(bool hit, int row, int orig, int d) const
    {
        const unsigned long long m = __ballot(hit);
        if (m == 0) return;
        const int lane = threadIdx.x & 63;
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(A.total, (unsigned long long)__popcll(m));
        base = __shfl(base, 0, 64);
        const unsigned long long pos = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
        if (hit && pos < A.capacity) A.keys[pos] = A.self ? join_pack(min(row, orig), max(row, orig), d) : join_pack(row, orig, d);
    }
};

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
        join_window(A, A.self != 0, la, &g_lo, &g_hi);
        for (int g = g_lo + wave; g < g_hi; g += 4) {
            const int slot = g * 64 + lane;
            const int orig = A.b_orig[slot];
            const int lb = A.b_len[slot];
            const int km = A.kmax[max(la, lb)];
            bool alive = join_owned(A.self != 0, row, la, orig, lb) && join_in_window(km, la, lb);
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
            JoinAppend{A}(alive && d <= km, row, orig, d);
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
    walk_general_body<IDB, OSA, true>(A, A.self != 0, JoinAppend{A}, WA, pm_all, vp_all, vn_all, d0_all);
}

// the cutoff of every M = max(|a|, |b|) the two lists allow: K9's formula evaluated around a guess (k11_core.h), once per call
__global__ __launch_bounds__(256) void k11_kmax_table(double t, int32_t n, int32_t *__restrict__ kmax)
{
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m < n) kmax[m] = join_kmax(t, m, m);
}

// the sorted keys -> CSR: hit p of the row-major order, and the row pointers of every row that begins between hit p - 1 and hit p
__global__ __launch_bounds__(256) void k11_unpack(const uint64_t *__restrict__ keys, int64_t total, int64_t n_from,
                                                   const int64_t *__restrict__ f_off, const int64_t *__restrict__ t_off,
                                                   int64_t *__restrict__ row_ptr, int32_t *__restrict__ out_idx,
                                                   int32_t *__restrict__ out_dist, double *__restrict__ out_sim)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= total) return;
    const uint64_t key = keys[p];
    const int row = join_key_row(key), to = join_key_to(key), d = join_key_dist(key);
    out_idx[p] = to;
    out_dist[p] = d;
    out_sim[p] = lev_similarity(d, (int)(f_off[row + 1] - f_off[row]), (int)(t_off[to + 1] - t_off[to]));
    const int prev = p > 0 ? join_key_row(keys[p - 1]) : -1;
    for (int64_t r = (int64_t)prev + 1; r <= row; ++r) row_ptr[r] = p;
    if (p == total - 1)
        for (int64_t r = (int64_t)row + 1; r <= n_from; ++r) row_ptr[r] = total;
}

static int join_run(pfz_ctx *ctx, const pfz_strings *F, const pfz_strings *T, bool self, int32_t scorer, double t, int64_t capacity,
                    int64_t *out_row_ptr, int32_t *out_idx, int32_t *out_dist, double *out_sim, int64_t *out_total,
                    int64_t *out_counters)
{
    PFZ_HIP(hipSetDevice(ctx->device));
    if (T->n > kJoinMaxStrings || F->n > kJoinMaxStrings || T->max_len > kJoinMaxLength || F->max_len > kJoinMaxLength) {
        set_error("pfz_lev_join: a list of more than %lld strings or a string of more than %lld characters does not fit the packed hit "
                  "(24-bit indices, 16-bit distance)", (long long)kJoinMaxStrings, (long long)kJoinMaxLength);
        return PFZ_ERR_UNSUPPORTED;
    }
    *out_total = 0;
    if (out_counters) out_counters[0] = out_counters[1] = out_counters[2] = 0;
    const int64_t n_from = F->n, n_to = T->n;
    if (n_from == 0 || n_to == 0) {
        for (int64_t r = 0; r <= n_from; ++r) out_row_ptr[r] = 0;
        return PFZ_OK;
    }
    const pfz_indel_plan *pl;
    PFZ_TRY(indel_plan_get(ctx, T, &pl));

    // The register kernel's share, while the match table fits 60 KiB of LDS (K4's limit): from-strings of <= 32 characters in
    // 32-bit words, of 33 .. 64 in 64-bit words.  Everything else is the general kernel's.
    const RowClasses rc = classify_rows(F, 0, n_from, lds_table_fits(pl));
    const std::vector<int32_t> (&rows_cls)[3] = rc.rows;      // <= 32, 33 .. 64, the general kernel's

    DevBuf d_rows[3], d_kmax, d_keys, d_sorted, d_state, d_ptr, d_idx, d_dist, d_sim;
    for (int c = 0; c < 3; ++c)
        if (!rows_cls[c].empty()) PFZ_TRY(d_rows[c].upload(ctx, rows_cls[c]));
    PFZ_TRY(d_keys.alloc(ctx, (size_t)capacity * sizeof(uint64_t)));
    const int32_t n_kmax = (int32_t)std::max(F->max_len, T->max_len) + 1;
    PFZ_TRY(d_kmax.alloc(ctx, (size_t)n_kmax * sizeof(int32_t)));
    hipLaunchKernelGGL(k11_kmax_table, dim3((unsigned)((n_kmax + 255) / 256)), dim3(256), 0, ctx->stream, t, n_kmax, d_kmax.as<int32_t>());
    PFZ_HIP(hipGetLastError());
    PFZ_TRY(d_state.alloc(ctx, 4 * sizeof(unsigned long long)));      // the total, then the three counters
    PFZ_HIP(hipMemsetAsync(d_state.p, 0, 4 * sizeof(unsigned long long), ctx->stream));

    JoinArgs A;
    static_cast<EditView &>(A) = edit_view(F, pl);
    A.n_to = (int32_t)n_to;
    A.self = self ? 1 : 0;
    A.kmax = d_kmax.as<int32_t>();
    A.keys = d_keys.as<uint64_t>();
    A.capacity = (unsigned long long)capacity;
    A.total = d_state.as<unsigned long long>();
    A.counters = out_counters ? d_state.as<unsigned long long>() + 1 : nullptr;

    const int64_t max_grid = (int64_t)ctx->prop.multiProcessorCount * 8;
    unsigned long long state[4];
    {
        ProfScope ps_all(ctx, "k11_join");
        for (int c = 0; c < 2; ++c) {
            if (rows_cls[c].empty()) continue;
            A.rows = d_rows[c].as<int32_t>();
            A.n_rows = (int32_t)rows_cls[c].size();
            const dim3 grid((unsigned)std::min<int64_t>(A.n_rows, max_grid));
            const size_t lds = (size_t)A.n_sym1 * (c == 1 ? sizeof(uint64_t) : sizeof(uint32_t));
            dispatch_idb_osa(pl->idb, scorer != 0, [&](auto IDB, auto OSA) {
                if (c == 0) hipLaunchKernelGGL((k11_join_kernel<uint32_t, decltype(IDB)::value, decltype(OSA)::value>), grid, dim3(256), lds, ctx->stream, A);
                else hipLaunchKernelGGL((k11_join_kernel<uint64_t, decltype(IDB)::value, decltype(OSA)::value>), grid, dim3(256), lds, ctx->stream, A);
            });
            PFZ_HIP(hipGetLastError());
        }
        if (!rows_cls[2].empty()) {
            A.rows = d_rows[2].as<int32_t>();
            A.n_rows = (int32_t)rows_cls[2].size();
            const int32_t WA = (int32_t)((rc.longest + 63) / 64);
            int64_t grid = std::min<int64_t>(A.n_rows, max_grid);
            PFZ_TRY(general_grid(&grid, A.n_sym1, WA, "pfz_lev_join", "a from-string", rc.longest));
            ProfScope ps(ctx, "k11_join_general");
            GeneralBufs gb;
            PFZ_TRY(general_bufs_alloc(ctx, &gb, grid, A.n_sym1, WA, {WA, WA, WA}, 256));
            dispatch_idb_osa(pl->idb, scorer != 0, [&](auto IDB, auto OSA) {
                hipLaunchKernelGGL((k11_join_general_kernel<decltype(IDB)::value, decltype(OSA)::value>), dim3((unsigned)grid), dim3(256), 0,
                                   ctx->stream, A, WA, gb.pm.as<uint64_t>(), gb.col[0].as<uint64_t>(), gb.col[1].as<uint64_t>(),
                                   gb.col[2].as<uint64_t>());
            });
            PFZ_HIP(hipGetLastError());
        }
        PFZ_TRY(copy_d2h(ctx, state, d_state.p, sizeof(state)));      // (waits for the kernels)
    }
    const int64_t total = (int64_t)state[0];
    *out_total = total;
    if (out_counters)
        for (int k = 0; k < 3; ++k) out_counters[k] = (int64_t)state[k + 1];
    if (total > capacity) return PFZ_OK;       // the caller's buffers stay as they are: it repeats the call with room for `total`
    if (total == 0) {
        for (int64_t r = 0; r <= n_from; ++r) out_row_ptr[r] = 0;
        return PFZ_OK;
    }
    {
        ProfScope ps(ctx, "k11_sort_unpack");
        PFZ_TRY(d_sorted.alloc(ctx, (size_t)sort_codes_capacity(total) * sizeof(uint64_t)));
        PFZ_TRY(sort_codes_u64(ctx, d_keys.as<uint64_t>(), d_sorted.as<uint64_t>(), total));
        PFZ_TRY(d_ptr.alloc(ctx, (size_t)(n_from + 1) * sizeof(int64_t)));
        PFZ_TRY(d_idx.alloc(ctx, (size_t)total * sizeof(int32_t)));
        PFZ_TRY(d_dist.alloc(ctx, (size_t)total * sizeof(int32_t)));
        PFZ_TRY(d_sim.alloc(ctx, (size_t)total * sizeof(double)));
        hipLaunchKernelGGL(k11_unpack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, d_sorted.as<uint64_t>(), total,
                           n_from, F->offsets, T->offsets, d_ptr.as<int64_t>(), d_idx.as<int32_t>(), d_dist.as<int32_t>(),
                           d_sim.as<double>());
        PFZ_HIP(hipGetLastError());
    }
    PFZ_TRY(copy_d2h(ctx, out_row_ptr, d_ptr.p, (size_t)(n_from + 1) * sizeof(int64_t)));
    PFZ_TRY(copy_d2h(ctx, out_idx, d_idx.p, (size_t)total * sizeof(int32_t)));
    PFZ_TRY(copy_d2h(ctx, out_dist, d_dist.p, (size_t)total * sizeof(int32_t)));
    PFZ_TRY(copy_d2h(ctx, out_sim, d_sim.p, (size_t)total * sizeof(double)));
    PFZ_HIP(hipStreamSynchronize(ctx->stream));
    return PFZ_OK;
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
