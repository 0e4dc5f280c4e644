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
#include "k11_core.h"
#include "k4_plan.h"

#include <algorithm>
#include <cmath>
#include <limits.h>

namespace pfz {

struct JoinArgs {
    const void *a_chars;       // from-strings: code units of a_width bytes
    int32_t a_width;
    const int64_t *a_off;      // [n_from + 1]
    const uint16_t *lut;       // code unit -> symbol rank (0 = not in the to-list's alphabet), lut_len entries
    uint32_t lut_len;
    const int32_t *rows;       // from-rows of this launch
    int32_t n_rows;
    const uint32_t *b_packed;  // to-strings, groups of 64, [t/PER][lane]
    const int64_t *g_off;      // [n_groups] dword offset of each group
    const int32_t *g_steps;    // [n_groups] dwords per lane
    const int32_t *b_len;      // [n_groups*64]
    const int32_t *b_orig;     // [n_groups*64] original to-index, -1 = padding lane
    int32_t n_groups;
    int32_t n_to;
    int32_t n_sym1;            // alphabet size + 1 (symbol 0 = padding)
    int32_t self;              // self-join: the plan is the from-list's own
    const int32_t *kmax;       // [longest string + 1] join_kmax of the threshold by M = max(|a|, |b|): all the kernels know of it
    uint64_t *keys;            // [capacity] the hits, in the order the waves got there
    unsigned long long capacity;
    unsigned long long *total;      // every hit, written or not
    unsigned long long *counters;   // optional [3]: pairs in the window, pairs not abandoned, recurrence steps of live lanes
};

// (K9's lev_a_symbol / lev_lds_or, which read K9's own argument block, restated on K11's: K9's translation unit stays as it is)
__device__ inline int join_a_symbol(const JoinArgs &A, int64_t at)
{
    const uint32_t c = A.a_width == 1 ? (uint32_t)((const uint8_t *)A.a_chars)[at] : ((const uint32_t *)A.a_chars)[at];
    return c < A.lut_len ? (int)A.lut[c] : 0;
}

__device__ inline void join_lds_or(uint32_t *p, uint32_t v) { atomicOr(p, v); }
__device__ inline void join_lds_or(uint64_t *p, uint64_t v) { atomicOr((unsigned long long *)p, (unsigned long long)v); }

// the run of groups [lo, hi) a from-string of la characters can have a hit in; wave-uniform
__device__ inline void join_window(const JoinArgs &A, int la, int *lo_out, int *hi_out)
{
    // the first group whose LONGEST string is long enough: nothing shorter than that passes (a self-join owns nothing shorter than la)
    int lo = 0, hi = A.n_groups;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int last = min(A.n_to, (mid + 1) * 64) - 1;
        const int l = __builtin_amdgcn_readfirstlane(A.b_len[last]);
        if (l >= la || (!A.self && join_in_window(A.kmax[la], la, l))) hi = mid;
        else lo = mid + 1;
    }
    *lo_out = lo;
    // the first group whose SHORTEST string is too long
    hi = A.n_groups;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int l = __builtin_amdgcn_readfirstlane(A.b_len[mid * 64]);
        if (l <= la || join_in_window(A.kmax[l], la, l)) lo = mid + 1;
        else hi = mid;
    }
    *hi_out = lo;
}

// the hits of one wave and group: one atomic for all of them, written while there is room
__device__ inline void join_emit(const JoinArgs &A, bool hit, int row, int orig, int d)
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

// a wave's work counts, once, when it has served its last row (three atomics per wave: per row they would queue up on three words)
__device__ inline void join_count(unsigned long long *counters, unsigned long long w, unsigned long long f, unsigned long long s)
{
    if (!counters) return;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        w += __shfl_xor(w, d, 64);
        f += __shfl_xor(f, d, 64);
        s += __shfl_xor(s, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(counters + 0, w);
        atomicAdd(counters + 1, f);
        atomicAdd(counters + 2, s);
    }
}

// is this lane's to-string the row's to walk?  (self-join: the plan's order -- shorter first, then the lower index)
__device__ inline bool join_owned(const JoinArgs &A, int row, int la, int orig, int lb)
{
    return orig >= 0 && (!A.self || lb > la || (lb == la && orig > row));
}

// WORD: uint32_t (from-strings of <= 32 characters) or uint64_t (<= 64), against to-strings of any length
template <typename WORD, int IDB, bool OSA>
__global__ __launch_bounds__(256) void k11_join_kernel(JoinArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    WORD *pm = (WORD *)smem_raw;
    constexpr int PER = 32 / IDB;  // symbols per dword
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    for (int p = tid; p < A.n_sym1; p += 256) pm[p] = 0;
    __syncthreads();

    unsigned long long n_win = 0, n_fin = 0, n_steps = 0;
    for (int r = blockIdx.x; r < A.n_rows; r += gridDim.x) {
        const int row = A.rows[r];
        const int64_t a0 = A.a_off[row];
        const int la = (int)(A.a_off[row + 1] - a0);      // fits the WORD
        const int my_sym = tid < la ? join_a_symbol(A, a0 + tid) : 0;
        if (my_sym) join_lds_or(&pm[my_sym], (WORD)1 << tid);
        __syncthreads();

        int g_lo, g_hi;
        join_window(A, la, &g_lo, &g_hi);
        for (int g = g_lo + wave; g < g_hi; g += 4) {
            const int slot = g * 64 + lane;
            const int orig = A.b_orig[slot];
            const int lb = A.b_len[slot];
            const int km = A.kmax[max(la, lb)];
            bool alive = join_owned(A, row, la, orig, lb) && join_in_window(km, la, lb);
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
            join_emit(A, alive && d <= km, row, orig, d);
        }
        __syncthreads();                                  // every wave is done with the match table
        if (my_sym) pm[my_sym] = 0;                       // clear the entries of this from-string
        __syncthreads();
    }
    join_count(A.counters, n_win, n_fin, n_steps);
}

// The general case: any from-length, any alphabet.  The match table of the workgroup's from-string (WA words per symbol) and every
// lane's column (VP, VN and, for OSA, the previous D0: WA words each) are in global memory; every group is visited, a lane walks
// its own to-string alone and stops where it is dead.
template <int IDB, bool OSA>
__global__ __launch_bounds__(256) void k11_join_general_kernel(JoinArgs A, int32_t WA, uint64_t *__restrict__ pm_all,
                                                                uint64_t *__restrict__ vp_all, uint64_t *__restrict__ vn_all,
                                                                uint64_t *__restrict__ d0_all)
{
    constexpr int PER = 32 / IDB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t *pm = pm_all + (int64_t)blockIdx.x * A.n_sym1 * WA;      // zero on entry, zero again after every row
    uint64_t *vp = vp_all + (int64_t)blockIdx.x * WA * 256 + tid;     // vp[w * 256]: this lane's word w
    uint64_t *vn = vn_all + (int64_t)blockIdx.x * WA * 256 + tid;
    uint64_t *d0 = d0_all + (int64_t)blockIdx.x * WA * 256 + tid;
    unsigned long long n_win = 0, n_fin = 0, n_steps = 0;
    for (int r = blockIdx.x; r < A.n_rows; r += gridDim.x) {
        const int row = A.rows[r];
        const int64_t a0 = A.a_off[row];
        const int la = (int)(A.a_off[row + 1] - a0);
        const int W = la > 0 ? (la + 63) / 64 : 1;                    // <= WA
        for (int p = tid; p < la; p += 256) {
            const int sy = join_a_symbol(A, a0 + p);
            if (sy) atomicOr((unsigned long long *)&pm[(int64_t)sy * WA + p / 64], 1ull << (p % 64));
        }
        __threadfence_block();
        __syncthreads();
        const uint64_t last = la > 0 ? 1ull << ((la - 1) % 64) : 0ull;
        for (int g = wave; g < A.n_groups; g += 4) {
            const int slot = g * 64 + lane;
            const int orig = A.b_orig[slot];
            const int lb = A.b_len[slot];
            const int km = A.kmax[max(la, lb)];
            bool alive = join_owned(A, row, la, orig, lb) && join_in_window(km, la, lb);
            if (!__any(alive)) continue;
            n_win += alive;
            int dist = la;
            if (alive) {
                const uint32_t *gp = A.b_packed + A.g_off[g] + lane;
                for (int w = 0; w < W; ++w) {
                    vp[(int64_t)w * 256] = low_ones<uint64_t>(la - 64 * w);
                    vn[(int64_t)w * 256] = 0ull;
                    d0[(int64_t)w * 256] = 0ull;
                }
                uint32_t c_prev = 0;                                    // (symbol 0: an empty table entry)
                for (int j = 0; j < lb; ++j) {
                    const uint32_t pk = gp[(int64_t)(j / PER) * 64];
                    const uint32_t c = (pk >> ((j % PER) * IDB)) & ((1u << IDB) - 1u);
                    const uint64_t *eq = pm + (int64_t)c * WA, *eq_prev = pm + (int64_t)c_prev * WA;
                    LevCarry cy = lev_carry_begin();
                    uint64_t hp = 0, hn = 0;
                    for (int w = 0; w < W; ++w) {
                        uint64_t x_vp = vp[(int64_t)w * 256], x_vn = vn[(int64_t)w * 256], x_d0 = OSA ? d0[(int64_t)w * 256] : 0ull;
                        lev_step_word<OSA>(x_vp, x_vn, x_d0, eq[w], OSA ? eq_prev[w] : 0ull, cy, &hp, &hn);
                        vp[(int64_t)w * 256] = x_vp;
                        vn[(int64_t)w * 256] = x_vn;
                        if (OSA) d0[(int64_t)w * 256] = x_d0;
                    }
                    dist += (int)((hp & last) != 0) - (int)((hn & last) != 0);
                    c_prev = c;
                    if (j + 1 < lb && join_abandon(dist, j + 1, lb, km)) {
                        alive = false;
                        n_steps += j + 1;
                        break;
                    }
                }
            }
            n_fin += alive;
            n_steps += alive ? lb : 0;
            const int d = lev_distance(dist, la, lb);
            join_emit(A, alive && d <= km, row, orig, d);
        }
        __syncthreads();                                              // every wave is done with the match table
        for (int p = tid; p < la; p += 256) {
            const int sy = join_a_symbol(A, a0 + p);
            if (sy) pm[(int64_t)sy * WA + p / 64] = 0ull;
        }
        __threadfence_block();
        __syncthreads();
    }
    join_count(A.counters, n_win, n_fin, n_steps);
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

template <typename WORD>
static void join_launch_reg(const JoinArgs &A, int idb, int osa, dim3 grid, size_t lds, hipStream_t st)
{
    if (idb == 8 && !osa) hipLaunchKernelGGL((k11_join_kernel<WORD, 8, false>), grid, dim3(256), lds, st, A);
    else if (idb == 8) hipLaunchKernelGGL((k11_join_kernel<WORD, 8, true>), grid, dim3(256), lds, st, A);
    else if (!osa) hipLaunchKernelGGL((k11_join_kernel<WORD, 16, false>), grid, dim3(256), lds, st, A);
    else hipLaunchKernelGGL((k11_join_kernel<WORD, 16, true>), grid, dim3(256), lds, st, A);
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
    const int32_t n_groups = (int32_t)pl->n_groups;

    // The register kernel's share, while the match table fits 60 KiB of LDS (K4's limit): from-strings of <= 32 characters in
    // 32-bit words, of 33 .. 64 in 64-bit words.  Everything else is the general kernel's.
    const bool lds_fits = (size_t)(pl->n_sym + 1) * sizeof(uint64_t) <= 60 * 1024;
    std::vector<int32_t> rows_cls[3];      // <= 32, 33 .. 64, the general kernel's
    int64_t longest = 1;
    for (int64_t i = 0; i < n_from; ++i) {
        const int64_t la = F->h_off[(size_t)i + 1] - F->h_off[(size_t)i];
        const int cls = !lds_fits || la > 64 ? 2 : (la > 32 ? 1 : 0);
        rows_cls[cls].push_back((int32_t)i);
        if (cls == 2) longest = std::max(longest, la);
    }

    DevBuf d_rows[3], d_kmax, d_keys, d_sorted, d_state, d_pm, d_vp, d_vn, d_d0, d_ptr, d_idx, d_dist, d_sim;
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
    A.a_chars = F->chars;
    A.a_width = F->char_width;
    A.a_off = F->offsets;
    A.lut = pl->lut;
    A.lut_len = pl->lut_len;
    A.b_packed = pl->packed;
    A.g_off = pl->g_off;
    A.g_steps = pl->g_steps;
    A.b_len = pl->b_len;
    A.b_orig = pl->b_orig;
    A.n_groups = n_groups;
    A.n_to = (int32_t)n_to;
    A.n_sym1 = pl->n_sym + 1;
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
            if (c == 0) join_launch_reg<uint32_t>(A, pl->idb, scorer, grid, lds, ctx->stream);
            else join_launch_reg<uint64_t>(A, pl->idb, scorer, grid, lds, ctx->stream);
            PFZ_HIP(hipGetLastError());
        }
        if (!rows_cls[2].empty()) {
            A.rows = d_rows[2].as<int32_t>();
            A.n_rows = (int32_t)rows_cls[2].size();
            const int32_t WA = (int32_t)((longest + 63) / 64);
            int64_t grid = std::min<int64_t>(A.n_rows, max_grid);
            const size_t pm_per = (size_t)A.n_sym1 * (size_t)WA * sizeof(uint64_t);
            while (grid > 1 && pm_per * (size_t)grid > ((size_t)2 << 30)) grid /= 2;      // <= 2 GiB of match tables
            if (pm_per * (size_t)grid > ((size_t)8 << 30)) {
                set_error("pfz_lev_join: a from-string of %lld characters with %d alphabet symbols needs a %zu-byte match table",
                          (long long)longest, pl->n_sym, pm_per);
                return PFZ_ERR_UNSUPPORTED;
            }
            ProfScope ps(ctx, "k11_join_general");
            const size_t col_bytes = (size_t)grid * (size_t)WA * 256 * sizeof(uint64_t);
            PFZ_TRY(d_pm.alloc(ctx, pm_per * (size_t)grid));
            PFZ_TRY(d_vp.alloc(ctx, col_bytes));
            PFZ_TRY(d_vn.alloc(ctx, col_bytes));
            PFZ_TRY(d_d0.alloc(ctx, col_bytes));
            PFZ_HIP(hipMemsetAsync(d_pm.p, 0, pm_per * (size_t)grid, ctx->stream));
#define PFZ_K11_GENERAL(IDB, OSA)                                                                                                  \
    hipLaunchKernelGGL((k11_join_general_kernel<IDB, OSA>), dim3((unsigned)grid), dim3(256), 0, ctx->stream, A, WA, d_pm.as<uint64_t>(), \
                       d_vp.as<uint64_t>(), d_vn.as<uint64_t>(), d_d0.as<uint64_t>())
            if (pl->idb == 8 && !scorer) PFZ_K11_GENERAL(8, false);
            else if (pl->idb == 8) PFZ_K11_GENERAL(8, true);
            else if (!scorer) PFZ_K11_GENERAL(16, false);
            else PFZ_K11_GENERAL(16, true);
#undef PFZ_K11_GENERAL
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
