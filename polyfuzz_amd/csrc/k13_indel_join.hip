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
// The views, the match-table helpers, the ownership rule, the counters, the row classes and the general launches' grid and
// buffers are edit_walk.h's, used as they are.  The window search and the two walks are here and not there: edit_walk.h's carry
// K9's state and kmax[max(la, lb)] in their signatures.  Both walks take the hit sink as a parameter (IndelAppend for the join,
// IndelHook for the components), so each is written once.  K11 / K12 wrote their register walk out twice because a common body
// cost them registers; here the state is one word, and the shared body's instances take 27 .. 44 VGPRs, no scratch (DESIGN.md,
// K13, has the figures; tests/test_indel_join_cpu.py holds them to 64).
#include "edit_walk.h"
#include "k12_core.h"
#include "k13_core.h"

#include <algorithm>
#include <cmath>
#include <limits.h>

namespace pfz {

struct IndelWalkArgs : EditView {
    const int32_t *rows;       // from-rows of this launch
    int32_t n_rows;
    int32_t n_to;
    const int32_t *lmin;       // [longest from-string + longest to-string + 1] indel_lmin of the threshold by S = |a| + |b|
    unsigned long long *total;      // every hit
    unsigned long long *counters;   // optional [3], LEV_JOIN_COUNTERS' meaning: in the window, not abandoned, steps of live lanes
};

struct IndelJoinArgs : IndelWalkArgs {
    int32_t self;              // self-join: the plan is the from-list's own
    uint64_t *keys;            // [capacity] the hits, in the order the waves got there
    unsigned long long capacity;
};

struct IndelCompArgs : IndelWalkArgs {   // (n_to: the list's own length)
    int32_t *parent;           // [n] the forest (k12_core.h)
};

// the join's hit sink (K11's JoinAppend with the LCS in the key): one atomic for the hits of a wave and group, written while
// there is room
struct IndelAppend {
    const IndelJoinArgs &A;
    __device__ void operator()(bool hit, int row, int orig, int lcs) const
    {
        const unsigned long long m = __ballot(hit);
        if (m == 0) return;
        const int lane = threadIdx.x & 63;
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(A.total, (unsigned long long)__popcll(m));
        base = __shfl(base, 0, 64);
        const unsigned long long pos = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
        if (hit && pos < A.capacity) A.keys[pos] = A.self ? join_pack(min(row, orig), max(row, orig), lcs) : join_pack(row, orig, lcs);
    }
};

// parent as the walk kernels touch it (K12's rule): relaxed, agent scope, nothing else
struct IndelUfOps {
    __device__ static int32_t load(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ static void store(int32_t *p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ static int32_t cas(int32_t *p, int32_t expected, int32_t desired)
    {
        __hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return expected;
    }
};

// the finished forest, behind the kernel boundary: plain loads
struct IndelUfPlain {
    __device__ static int32_t load(const int32_t *p) { return *p; }
};

// the components' hit sink: the hits counted as the join counts them, and each hit lane hooks its pair into the forest
struct IndelHook {
    const IndelCompArgs &A;
    __device__ void operator()(bool hit, int row, int orig, int) const
    {
        const unsigned long long m = __ballot(hit);
        if (m == 0) return;
        if ((threadIdx.x & 63) == 0) atomicAdd(A.total, (unsigned long long)__popcll(m));
        if (hit) uf_unite<IndelUfOps>(A.parent, row, orig);
    }
};

// the run of groups [lo, hi) a from-string of la characters can have a hit in (join_window's shape, the Indel predicate);
// wave-uniform.  A to-string of la characters is always inside (the bound is 1.0), so the run is around length la.
__device__ inline void indel_window(const IndelWalkArgs &A, bool self, int la, int *lo_out, int *hi_out)
{
    // the first group whose LONGEST string is long enough (a self-join owns nothing shorter than la)
    int lo = 0, hi = A.n_groups;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int last = min(A.n_to, (mid + 1) * 64) - 1;
        const int l = __builtin_amdgcn_readfirstlane(A.b_len[last]);
        if (l >= la || (!self && indel_in_window(A.lmin[la + l], la, l))) hi = mid;
        else lo = mid + 1;
    }
    *lo_out = lo;
    // the first group whose SHORTEST string is too long
    hi = A.n_groups;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int l = __builtin_amdgcn_readfirstlane(A.b_len[mid * 64]);
        if (l <= la || indel_in_window(A.lmin[la + l], la, l)) lo = mid + 1;
        else hi = mid;
    }
    *hi_out = lo;
}

// The register walk.  WORD: uint32_t (from-strings of <= 32 characters) or uint64_t (<= 64), against to-strings of any length.
// The padding behind a lane's end is symbol 0, whose table entry is empty: it leaves V as it is.
template <typename WORD, int IDB, bool TWO_LISTS, typename SINK>
__device__ __forceinline__ void indel_walk_reg_body(const IndelWalkArgs &A, bool self_arg, const SINK &sink)
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
            const int lm = A.lmin[la + lb];
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
__device__ __forceinline__ void indel_walk_general_body(const IndelWalkArgs &A, bool self_arg, const SINK &sink, int32_t WA,
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
            const int lm = A.lmin[la + lb];
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
__global__ __launch_bounds__(256) void k13_join_kernel(IndelJoinArgs A)
{
    indel_walk_reg_body<WORD, IDB, true>(A, A.self != 0, IndelAppend{A});
}

template <typename WORD, int IDB>
__global__ __launch_bounds__(256) void k13_comp_kernel(IndelCompArgs A)
{
    indel_walk_reg_body<WORD, IDB, false>(A, true, IndelHook{A});
}

template <int IDB>
__global__ __launch_bounds__(256) void k13_join_general_kernel(IndelJoinArgs A, int32_t WA, uint64_t *__restrict__ pm_all,
                                                                uint64_t *__restrict__ v_all)
{
    indel_walk_general_body<IDB, true>(A, A.self != 0, IndelAppend{A}, WA, pm_all, v_all);
}

template <int IDB>
__global__ __launch_bounds__(256) void k13_comp_general_kernel(IndelCompArgs A, int32_t WA, uint64_t *__restrict__ pm_all,
                                                                uint64_t *__restrict__ v_all)
{
    indel_walk_general_body<IDB, false>(A, true, IndelHook{A}, WA, pm_all, v_all);
}

// the cutoff of every S = |a| + |b| the two lists allow (the formula evaluated around a guess, k13_core.h), once per call; for
// the components also every position its own root (n_parent = 0: no forest)
__global__ __launch_bounds__(256) void k13_begin(double t, int32_t n_lmin, int32_t *__restrict__ lmin, int32_t n_parent,
                                                  int32_t *__restrict__ parent)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_lmin) lmin[i] = indel_lmin(t, (int)i);
    if (i < n_parent) parent[i] = (int32_t)i;
}

// the sorted keys -> CSR: hit p of the row-major order, and the row pointers of every row that begins between hit p - 1 and hit p
__global__ __launch_bounds__(256) void k13_unpack(const uint64_t *__restrict__ keys, int64_t total, int64_t n_from,
                                                   const int64_t *__restrict__ f_off, const int64_t *__restrict__ t_off,
                                                   int64_t *__restrict__ row_ptr, int32_t *__restrict__ out_idx,
                                                   int32_t *__restrict__ out_dist, double *__restrict__ out_sim)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= total) return;
    const uint64_t key = keys[p];
    const int row = join_key_row(key), to = join_key_to(key), lcs = join_key_dist(key);
    const int la = (int)(f_off[row + 1] - f_off[row]), lb = (int)(t_off[to + 1] - t_off[to]);
    out_idx[p] = to;
    out_dist[p] = indel_distance(lcs, la, lb);
    out_sim[p] = indel_similarity(lcs, la, lb);
    const int prev = p > 0 ? join_key_row(keys[p - 1]) : -1;
    for (int64_t r = (int64_t)prev + 1; r <= row; ++r) row_ptr[r] = p;
    if (p == total - 1)
        for (int64_t r = (int64_t)row + 1; r <= n_from; ++r) row_ptr[r] = total;
}

// after the walk, behind the kernel boundary: label[i] = the root of i's tree, and the roots counted (one atomic per wave)
__global__ __launch_bounds__(256) void k13_flatten(const int32_t *__restrict__ parent, int32_t n, int32_t *__restrict__ label,
                                                    unsigned long long *__restrict__ n_roots)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int32_t root = -1;
    if (i < n) {
        root = uf_root<IndelUfPlain>(parent, (int32_t)i);
        label[i] = root;
    }
    const unsigned long long m = __ballot(root == (int32_t)i);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_roots, (unsigned long long)__popcll(m));
}

// f(std::integral_constant<int, IDB>) for the plan's symbol width
template <typename F> static inline void dispatch_idb(int idb, F &&f)
{
    if (idb == 8) f(std::integral_constant<int, 8>{});
    else f(std::integral_constant<int, 16>{});
}

// the three launches of a call over the row classes (<= 32, 33 .. 64, the general kernel's); COMP: the components' kernels
template <bool COMP, typename ARGS>
static int indel_walk_launch(pfz_ctx *ctx, const pfz_indel_plan *pl, const RowClasses &rc, DevBuf (&d_rows)[3], ARGS &A, const char *entry,
                             const char *what)
{
    const int64_t max_grid = (int64_t)ctx->prop.multiProcessorCount * 8;
    for (int c = 0; c < 2; ++c) {
        if (rc.rows[c].empty()) continue;
        A.rows = d_rows[c].as<int32_t>();
        A.n_rows = (int32_t)rc.rows[c].size();
        const dim3 grid((unsigned)std::min<int64_t>(A.n_rows, max_grid));
        const size_t lds = (size_t)A.n_sym1 * (c == 1 ? sizeof(uint64_t) : sizeof(uint32_t));
        dispatch_idb(pl->idb, [&](auto IDB) {
            constexpr int B = decltype(IDB)::value;
            if constexpr (COMP) {
                if (c == 0) hipLaunchKernelGGL((k13_comp_kernel<uint32_t, B>), grid, dim3(256), lds, ctx->stream, A);
                else hipLaunchKernelGGL((k13_comp_kernel<uint64_t, B>), grid, dim3(256), lds, ctx->stream, A);
            }
            else {
                if (c == 0) hipLaunchKernelGGL((k13_join_kernel<uint32_t, B>), grid, dim3(256), lds, ctx->stream, A);
                else hipLaunchKernelGGL((k13_join_kernel<uint64_t, B>), grid, dim3(256), lds, ctx->stream, A);
            }
        });
        PFZ_HIP(hipGetLastError());
    }
    if (!rc.rows[2].empty()) {
        A.rows = d_rows[2].as<int32_t>();
        A.n_rows = (int32_t)rc.rows[2].size();
        const int32_t WA = (int32_t)((rc.longest + 63) / 64);
        int64_t grid = std::min<int64_t>(A.n_rows, max_grid);
        PFZ_TRY(general_grid(&grid, A.n_sym1, WA, entry, what, rc.longest));
        ProfScope ps(ctx, COMP ? "k13_comp_general" : "k13_join_general");
        GeneralBufs gb;
        PFZ_TRY(general_bufs_alloc(ctx, &gb, grid, A.n_sym1, WA, {WA, 0, 0}, 256));      // one column, V
        dispatch_idb(pl->idb, [&](auto IDB) {
            constexpr int B = decltype(IDB)::value;
            if constexpr (COMP)
                hipLaunchKernelGGL((k13_comp_general_kernel<B>), dim3((unsigned)grid), dim3(256), 0, ctx->stream, A, WA, gb.pm.as<uint64_t>(),
                                   gb.col[0].as<uint64_t>());
            else
                hipLaunchKernelGGL((k13_join_general_kernel<B>), dim3((unsigned)grid), dim3(256), 0, ctx->stream, A, WA, gb.pm.as<uint64_t>(),
                                   gb.col[0].as<uint64_t>());
        });
        PFZ_HIP(hipGetLastError());
    }
    return PFZ_OK;
}

static int indel_join_run(pfz_ctx *ctx, const pfz_strings *F, const pfz_strings *T, bool self, double t, int64_t capacity,
                          int64_t *out_row_ptr, int32_t *out_idx, int32_t *out_dist, double *out_sim, int64_t *out_total,
                          int64_t *out_counters)
{
    PFZ_HIP(hipSetDevice(ctx->device));
    if (T->n > kJoinMaxStrings || F->n > kJoinMaxStrings || T->max_len > kJoinMaxLength || F->max_len > kJoinMaxLength) {
        set_error("pfz_indel_join: a list of more than %lld strings or a string of more than %lld characters does not fit the packed "
                  "hit (24-bit indices, 16-bit LCS)", (long long)kJoinMaxStrings, (long long)kJoinMaxLength);
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
    const RowClasses rc = classify_rows(F, 0, n_from, lds_table_fits(pl));

    DevBuf d_rows[3], d_lmin, d_keys, d_sorted, d_state, d_ptr, d_idx, d_dist, d_sim;
    for (int c = 0; c < 3; ++c)
        if (!rc.rows[c].empty()) PFZ_TRY(d_rows[c].upload(ctx, rc.rows[c]));
    PFZ_TRY(d_keys.alloc(ctx, (size_t)capacity * sizeof(uint64_t)));
    const int32_t n_lmin = (int32_t)(F->max_len + T->max_len) + 1;
    PFZ_TRY(d_lmin.alloc(ctx, (size_t)n_lmin * sizeof(int32_t)));
    hipLaunchKernelGGL(k13_begin, dim3((unsigned)((n_lmin + 255) / 256)), dim3(256), 0, ctx->stream, t, n_lmin, d_lmin.as<int32_t>(), 0,
                       (int32_t *)nullptr);
    PFZ_HIP(hipGetLastError());
    PFZ_TRY(d_state.alloc(ctx, 4 * sizeof(unsigned long long)));      // the total, then the three counters
    PFZ_HIP(hipMemsetAsync(d_state.p, 0, 4 * sizeof(unsigned long long), ctx->stream));

    IndelJoinArgs A;
    static_cast<EditView &>(A) = edit_view(F, pl);
    A.n_to = (int32_t)n_to;
    A.self = self ? 1 : 0;
    A.lmin = d_lmin.as<int32_t>();
    A.keys = d_keys.as<uint64_t>();
    A.capacity = (unsigned long long)capacity;
    A.total = d_state.as<unsigned long long>();
    A.counters = out_counters ? d_state.as<unsigned long long>() + 1 : nullptr;

    unsigned long long state[4];
    {
        ProfScope ps_all(ctx, "k13_join");
        PFZ_TRY(indel_walk_launch<false>(ctx, pl, rc, d_rows, A, "pfz_indel_join", "a from-string"));
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
        ProfScope ps(ctx, "k13_sort_unpack");
        PFZ_TRY(d_sorted.alloc(ctx, (size_t)sort_codes_capacity(total) * sizeof(uint64_t)));
        PFZ_TRY(sort_codes_u64(ctx, d_keys.as<uint64_t>(), d_sorted.as<uint64_t>(), total));
        PFZ_TRY(d_ptr.alloc(ctx, (size_t)(n_from + 1) * sizeof(int64_t)));
        PFZ_TRY(d_idx.alloc(ctx, (size_t)total * sizeof(int32_t)));
        PFZ_TRY(d_dist.alloc(ctx, (size_t)total * sizeof(int32_t)));
        PFZ_TRY(d_sim.alloc(ctx, (size_t)total * sizeof(double)));
        hipLaunchKernelGGL(k13_unpack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, d_sorted.as<uint64_t>(), total,
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

static int indel_comp_run(pfz_ctx *ctx, const pfz_strings *F, double t, int32_t *out_label, int64_t *out_pairs, int64_t *out_components,
                          int64_t *out_counters)
{
    PFZ_HIP(hipSetDevice(ctx->device));
    *out_pairs = *out_components = 0;
    if (out_counters) out_counters[0] = out_counters[1] = out_counters[2] = 0;
    const int64_t n = F->n;
    if (n == 0) return PFZ_OK;
    if (n > (int64_t)INT_MAX - 64 || F->max_len > ((int64_t)INT_MAX - 1) / 2) {
        set_error("pfz_indel_components: %lld strings, the longest of %lld characters: positions (padded to groups of 64) and the sum "
                  "of two lengths are 32-bit", (long long)n, (long long)F->max_len);
        return PFZ_ERR_UNSUPPORTED;
    }
    const pfz_indel_plan *pl;
    PFZ_TRY(indel_plan_get(ctx, F, &pl));
    const RowClasses rc = classify_rows(F, 0, n, lds_table_fits(pl));

    DevBuf d_rows[3], d_lmin, d_parent, d_label, d_state;
    for (int c = 0; c < 3; ++c)
        if (!rc.rows[c].empty()) PFZ_TRY(d_rows[c].upload(ctx, rc.rows[c]));
    const int32_t n_lmin = (int32_t)(2 * F->max_len) + 1;
    PFZ_TRY(d_lmin.alloc(ctx, (size_t)n_lmin * sizeof(int32_t)));
    PFZ_TRY(d_parent.alloc(ctx, (size_t)n * sizeof(int32_t)));
    PFZ_TRY(d_label.alloc(ctx, (size_t)n * sizeof(int32_t)));
    PFZ_TRY(d_state.alloc(ctx, 5 * sizeof(unsigned long long)));      // the hits, the three counters, the roots
    PFZ_HIP(hipMemsetAsync(d_state.p, 0, 5 * sizeof(unsigned long long), ctx->stream));
    const int64_t n_begin = std::max<int64_t>(n, n_lmin);
    hipLaunchKernelGGL(k13_begin, dim3((unsigned)((n_begin + 255) / 256)), dim3(256), 0, ctx->stream, t, n_lmin, d_lmin.as<int32_t>(),
                       (int32_t)n, d_parent.as<int32_t>());
    PFZ_HIP(hipGetLastError());

    IndelCompArgs A;
    static_cast<EditView &>(A) = edit_view(F, pl);
    A.n_to = (int32_t)n;
    A.lmin = d_lmin.as<int32_t>();
    A.parent = d_parent.as<int32_t>();
    A.total = d_state.as<unsigned long long>();
    A.counters = out_counters ? d_state.as<unsigned long long>() + 1 : nullptr;
    {
        ProfScope ps_all(ctx, "k13_comp");
        PFZ_TRY(indel_walk_launch<true>(ctx, pl, rc, d_rows, A, "pfz_indel_components", "a string"));
    }
    {
        ProfScope ps(ctx, "k13_flatten");
        hipLaunchKernelGGL(k13_flatten, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_parent.as<int32_t>(), (int32_t)n,
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
