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
// (K11's argument block, window and ownership rule are restated here on K12's own block, as K11 restated K9's: K11's translation
// unit, whose kernels tests pin by name and register count, stays as it is.)
#include "k11_core.h"
#include "k12_core.h"
#include "k4_plan.h"

#include <algorithm>
#include <cmath>
#include <limits.h>

namespace pfz {

struct CompArgs {
    const void *a_chars;       // the list's strings: code units of a_width bytes
    int32_t a_width;
    const int64_t *a_off;      // [n + 1]
    const uint16_t *lut;       // code unit -> symbol rank, lut_len entries
    uint32_t lut_len;
    const int32_t *rows;       // from-rows of this launch
    int32_t n_rows;
    const uint32_t *b_packed;  // the same strings as the plan packs them, groups of 64, [t/PER][lane]
    const int64_t *g_off;      // [n_groups] dword offset of each group
    const int32_t *g_steps;    // [n_groups] dwords per lane
    const int32_t *b_len;      // [n_groups*64]
    const int32_t *b_orig;     // [n_groups*64] original position, -1 = padding lane
    int32_t n_groups;
    int32_t n;
    int32_t n_sym1;            // alphabet size + 1 (symbol 0 = padding)
    const int32_t *kmax;       // [longest string + 1] join_kmax of the threshold by M = max(|a|, |b|)
    int32_t *parent;           // [n] the forest (k12_core.h)
    unsigned long long *total;      // every hit
    unsigned long long *counters;   // optional [3], K11's: pairs in the window, pairs not abandoned, recurrence steps of live lanes
};

// parent as the walk kernels touch it: relaxed, agent scope, nothing else
struct UfDeviceOps {
    __device__ static int32_t load(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ static void store(int32_t *p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ static int32_t cas(int32_t *p, int32_t expected, int32_t desired)
    {
        __hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return expected;
    }
};

// the finished forest, behind the kernel boundary: plain loads
struct UfPlainOps {
    __device__ static int32_t load(const int32_t *p) { return *p; }
};

__device__ inline int comp_a_symbol(const CompArgs &A, int64_t at)
{
    const uint32_t c = A.a_width == 1 ? (uint32_t)((const uint8_t *)A.a_chars)[at] : ((const uint32_t *)A.a_chars)[at];
    return c < A.lut_len ? (int)A.lut[c] : 0;
}

__device__ inline void comp_lds_or(uint32_t *p, uint32_t v) { atomicOr(p, v); }
__device__ inline void comp_lds_or(uint64_t *p, uint64_t v) { atomicOr((unsigned long long *)p, (unsigned long long)v); }

// K11's join_window of a self-join: the run of groups [lo, hi) in which a row of la characters owns a pair that can be a hit
__device__ inline void comp_window(const CompArgs &A, int la, int *lo_out, int *hi_out)
{
    // the first group whose LONGEST string is as long as the row: it owns nothing shorter
    int lo = 0, hi = A.n_groups;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int last = min(A.n, (mid + 1) * 64) - 1;
        const int l = __builtin_amdgcn_readfirstlane(A.b_len[last]);
        if (l >= la) hi = mid;
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

// K11's ownership rule: the row of the shorter string walks the pair, at equal length the lower position
__device__ inline bool comp_owned(int row, int la, int orig, int lb) { return orig >= 0 && (lb > la || (lb == la && orig > row)); }

// the hits of one wave and group: counted with one atomic, and each hit lane hooks its pair into the forest
__device__ inline void comp_hook(const CompArgs &A, bool hit, int row, int orig)
{
    const unsigned long long m = __ballot(hit);
    if (m == 0) return;
    if ((threadIdx.x & 63) == 0) atomicAdd(A.total, (unsigned long long)__popcll(m));
    if (hit) uf_unite<UfDeviceOps>(A.parent, row, orig);
}

__device__ inline void comp_count(unsigned long long *counters, unsigned long long w, unsigned long long f, unsigned long long s)
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

// WORD: uint32_t (from-strings of <= 32 characters) or uint64_t (<= 64), against to-strings of any length.  K11's k11_join_kernel
// with comp_hook in the place of the append.
template <typename WORD, int IDB, bool OSA>
__global__ __launch_bounds__(256) void k12_walk_kernel(CompArgs A)
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
        const int my_sym = tid < la ? comp_a_symbol(A, a0 + tid) : 0;
        if (my_sym) comp_lds_or(&pm[my_sym], (WORD)1 << tid);
        __syncthreads();

        int g_lo, g_hi;
        comp_window(A, la, &g_lo, &g_hi);
        for (int g = g_lo + wave; g < g_hi; g += 4) {
            const int slot = g * 64 + lane;
            const int orig = A.b_orig[slot];
            const int lb = A.b_len[slot];
            const int km = A.kmax[max(la, lb)];
            bool alive = comp_owned(row, la, orig, lb) && join_in_window(km, la, lb);
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
            comp_hook(A, alive && d <= km, row, orig);
        }
        __syncthreads();                                  // every wave is done with the match table
        if (my_sym) pm[my_sym] = 0;                       // clear the entries of this from-string
        __syncthreads();
    }
    comp_count(A.counters, n_win, n_fin, n_steps);
}

// The general case: any from-length, any alphabet -- K11's k11_join_general_kernel with comp_hook in the place of the append.  The
// match table of the workgroup's from-string (WA words per symbol) and every lane's column (VP, VN and, for OSA, the previous D0:
// WA words each) are in global memory; every group is visited, a lane walks its own to-string alone and stops where it is dead.
template <int IDB, bool OSA>
__global__ __launch_bounds__(256) void k12_walk_general_kernel(CompArgs A, int32_t WA, uint64_t *__restrict__ pm_all,
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
            const int sy = comp_a_symbol(A, a0 + p);
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
            bool alive = comp_owned(row, la, orig, lb) && join_in_window(km, la, lb);
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
            comp_hook(A, alive && d <= km, row, orig);
        }
        __syncthreads();                                              // every wave is done with the match table
        for (int p = tid; p < la; p += 256) {
            const int sy = comp_a_symbol(A, a0 + p);
            if (sy) pm[(int64_t)sy * WA + p / 64] = 0ull;
        }
        __threadfence_block();
        __syncthreads();
    }
    comp_count(A.counters, n_win, n_fin, n_steps);
}

// before the walk: the cutoff of every M (K11's table: K9's formula evaluated around a guess, k11_core.h) and every position its
// own root
__global__ __launch_bounds__(256) void k12_begin(double t, int32_t n_kmax, int32_t *__restrict__ kmax, int32_t n, int32_t *__restrict__ parent)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_kmax) kmax[i] = join_kmax(t, (int)i, (int)i);
    if (i < n) parent[i] = (int32_t)i;
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

template <typename WORD>
static void comp_launch_reg(const CompArgs &A, int idb, int osa, dim3 grid, size_t lds, hipStream_t st)
{
    if (idb == 8 && !osa) hipLaunchKernelGGL((k12_walk_kernel<WORD, 8, false>), grid, dim3(256), lds, st, A);
    else if (idb == 8) hipLaunchKernelGGL((k12_walk_kernel<WORD, 8, true>), grid, dim3(256), lds, st, A);
    else if (!osa) hipLaunchKernelGGL((k12_walk_kernel<WORD, 16, false>), grid, dim3(256), lds, st, A);
    else hipLaunchKernelGGL((k12_walk_kernel<WORD, 16, true>), grid, dim3(256), lds, st, A);
}

static int comp_run(pfz_ctx *ctx, const pfz_strings *F, int32_t scorer, double t, int32_t *out_label, int64_t *out_pairs,
                    int64_t *out_components, int64_t *out_counters)
{
    PFZ_HIP(hipSetDevice(ctx->device));
    *out_pairs = *out_components = 0;
    if (out_counters) out_counters[0] = out_counters[1] = out_counters[2] = 0;
    const int64_t n = F->n;
    if (n == 0) return PFZ_OK;
    if (n > (int64_t)INT_MAX - 64 || F->max_len >= (int64_t)INT_MAX) {
        set_error("pfz_lev_components: %lld strings, the longest of %lld characters: positions (padded to groups of 64) and lengths "
                  "are 32-bit", (long long)n, (long long)F->max_len);
        return PFZ_ERR_UNSUPPORTED;
    }
    const pfz_indel_plan *pl;
    PFZ_TRY(indel_plan_get(ctx, F, &pl));
    const int32_t n_groups = (int32_t)pl->n_groups;

    // K11's three classes: <= 32 characters in 32-bit words, 33 .. 64 in 64-bit words while the match table fits 60 KiB of LDS
    // (K4's limit); everything else is the general kernel's
    const bool lds_fits = (size_t)(pl->n_sym + 1) * sizeof(uint64_t) <= 60 * 1024;
    std::vector<int32_t> rows_cls[3];
    int64_t longest = 1;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t la = F->h_off[(size_t)i + 1] - F->h_off[(size_t)i];
        const int cls = !lds_fits || la > 64 ? 2 : (la > 32 ? 1 : 0);
        rows_cls[cls].push_back((int32_t)i);
        if (cls == 2) longest = std::max(longest, la);
    }

    DevBuf d_rows[3], d_kmax, d_parent, d_label, d_state, d_pm, d_vp, d_vn, d_d0;
    for (int c = 0; c < 3; ++c)
        if (!rows_cls[c].empty()) PFZ_TRY(d_rows[c].upload(ctx, rows_cls[c]));
    const int32_t n_kmax = (int32_t)F->max_len + 1;
    PFZ_TRY(d_kmax.alloc(ctx, (size_t)n_kmax * sizeof(int32_t)));
    PFZ_TRY(d_parent.alloc(ctx, (size_t)n * sizeof(int32_t)));
    PFZ_TRY(d_label.alloc(ctx, (size_t)n * sizeof(int32_t)));
    PFZ_TRY(d_state.alloc(ctx, 5 * sizeof(unsigned long long)));      // the hits, the three counters, the roots
    PFZ_HIP(hipMemsetAsync(d_state.p, 0, 5 * sizeof(unsigned long long), ctx->stream));
    const int64_t n_begin = std::max<int64_t>(n, n_kmax);
    hipLaunchKernelGGL(k12_begin, dim3((unsigned)((n_begin + 255) / 256)), dim3(256), 0, ctx->stream, t, n_kmax, d_kmax.as<int32_t>(),
                       (int32_t)n, d_parent.as<int32_t>());
    PFZ_HIP(hipGetLastError());

    CompArgs A;
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
    A.n = (int32_t)n;
    A.n_sym1 = pl->n_sym + 1;
    A.kmax = d_kmax.as<int32_t>();
    A.parent = d_parent.as<int32_t>();
    A.total = d_state.as<unsigned long long>();
    A.counters = out_counters ? d_state.as<unsigned long long>() + 1 : nullptr;

    const int64_t max_grid = (int64_t)ctx->prop.multiProcessorCount * 8;
    {
        ProfScope ps_all(ctx, "k12_walk");
        for (int c = 0; c < 2; ++c) {
            if (rows_cls[c].empty()) continue;
            A.rows = d_rows[c].as<int32_t>();
            A.n_rows = (int32_t)rows_cls[c].size();
            const dim3 grid((unsigned)std::min<int64_t>(A.n_rows, max_grid));
            const size_t lds = (size_t)A.n_sym1 * (c == 1 ? sizeof(uint64_t) : sizeof(uint32_t));
            if (c == 0) comp_launch_reg<uint32_t>(A, pl->idb, scorer, grid, lds, ctx->stream);
            else comp_launch_reg<uint64_t>(A, pl->idb, scorer, grid, lds, ctx->stream);
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
                set_error("pfz_lev_components: a string of %lld characters with %d alphabet symbols needs a %zu-byte match table",
                          (long long)longest, pl->n_sym, pm_per);
                return PFZ_ERR_UNSUPPORTED;
            }
            ProfScope ps(ctx, "k12_walk_general");
            const size_t col_bytes = (size_t)grid * (size_t)WA * 256 * sizeof(uint64_t);
            PFZ_TRY(d_pm.alloc(ctx, pm_per * (size_t)grid));
            PFZ_TRY(d_vp.alloc(ctx, col_bytes));
            PFZ_TRY(d_vn.alloc(ctx, col_bytes));
            PFZ_TRY(d_d0.alloc(ctx, col_bytes));
            PFZ_HIP(hipMemsetAsync(d_pm.p, 0, pm_per * (size_t)grid, ctx->stream));
#define PFZ_K12_GENERAL(IDB, OSA)                                                                                                  \
    hipLaunchKernelGGL((k12_walk_general_kernel<IDB, OSA>), dim3((unsigned)grid), dim3(256), 0, ctx->stream, A, WA, d_pm.as<uint64_t>(), \
                       d_vp.as<uint64_t>(), d_vn.as<uint64_t>(), d_d0.as<uint64_t>())
            if (pl->idb == 8 && !scorer) PFZ_K12_GENERAL(8, false);
            else if (pl->idb == 8) PFZ_K12_GENERAL(8, true);
            else if (!scorer) PFZ_K12_GENERAL(16, false);
            else PFZ_K12_GENERAL(16, true);
#undef PFZ_K12_GENERAL
            PFZ_HIP(hipGetLastError());
        }
    }
    {
        ProfScope ps(ctx, "k12_flatten");
        hipLaunchKernelGGL(k12_flatten, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_parent.as<int32_t>(), (int32_t)n,
                           d_label.as<int32_t>(), d_state.as<unsigned long long>() + 4);
        PFZ_HIP(hipGetLastError());
    }
    unsigned long long state[5];
    PFZ_TRY(copy_d2h(ctx, state, d_state.p, sizeof(state)));
    PFZ_TRY(copy_d2h(ctx, out_label, d_label.p, (size_t)n * sizeof(int32_t)));
    PFZ_HIP(hipStreamSynchronize(ctx->stream));
    *out_pairs = (int64_t)state[0];
    *out_components = (int64_t)state[4];
    if (out_counters)
        for (int k = 0; k < 3; ++k) out_counters[k] = (int64_t)state[k + 1];
    return PFZ_OK;
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
