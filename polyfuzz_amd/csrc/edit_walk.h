// What the edit-distance kernels on K4's to-side plan have in common -- K8 (k8_jaro.hip), K9 (k9_levenshtein.hip), K10
// (k10_pairs.hip), K11 (k11_join.hip), K12 (k12_components.hip), K13 (k13_indel_join.hip), K20 (k20_jaro_join.hip: the view, the
// table, the ownership rule, the row classes and their launches) -- each thing once:
//   the view      FromView (the from-strings and the plan's code unit -> symbol table) and EditView (+ the plan's packed groups),
//                 which every argument block begins with, filled by from_view() / edit_view();
//   the table     the symbol look-up, the LDS OR, and the set / clear of the workgroup's match table in its register form (one
//                 LDS word per symbol) and its global form (WA 64-bit words per symbol), barriers and fences included;
//   the best      one (score, index) best, its record, the workgroup's first maximum, the merge over a row's records (K8, K9), and
//                 the wave sum behind one atomic add for the work counters;
//   the walk      K11's threshold walk -- argument block, window, ownership rule, counters, and the general body with the hit sink
//                 and "is there a second list" as parameters.  The REGISTER walk is written out in k11_join_kernel and in
//                 k12_walk_kernel: behind a common body the same source compiled to more registers and a slower step loop
//                 (DESIGN.md, K12).  K13's two walks (another recurrence, another cutoff) are its own;
//   the sinks     what a threshold walk does with a hit, for K11, K12 and K13 alike: KeyAppend (a join: one 64-bit key behind one
//                 atomic per wave and group) and ForestHook (components: the pair united in K12's forest), each the sub-block of
//                 the argument block that holds its fields;
//   the ends      the set-up kernel (the cutoff table and, for components, every position its own root, one launch) and the
//                 unpack kernel (sorted keys -> CSR), templates over the family's cutoff and its payload -> (distance, similarity);
//   the host      the three row classes, the general kernels' grid (cap or refusal) and scratch (match tables, column buffers),
//                 the symbol width x scorer dispatch, the launches over the row classes (walk_launch) and the whole host side
//                 of a join call (edit_join_run) and of a components call (edit_comp_run, on pfz_internal.h's ForestRun).
// The multi-word column the general kernels walk (lev_column_begin / lev_column_step) is k9_core.h's, beside the recurrence; the
// grid cap is k4_plan.h's, where K4 finds it too.
#pragma once

#include "k11_core.h"
#include "k12_core.h"
#include "k4_plan.h"

#include <algorithm>
#include <limits.h>
#include <type_traits>

namespace pfz {

struct FromView {
    const void *a_chars;       // from-strings: code units of a_width bytes
    int32_t a_width;
    const int64_t *a_off;      // [n_from + 1]
    const uint16_t *lut;       // code unit -> symbol rank (0 = not in the to-list's alphabet), lut_len entries
    uint32_t lut_len;
    int32_t n_sym1;            // alphabet size + 1 (symbol 0 = padding, an empty table entry)
};

struct EditView : FromView {
    const uint32_t *b_packed;  // to-strings, groups of 64, [t/PER][lane]
    const int64_t *g_off;      // [n_groups] dword offset of each group
    const int32_t *g_steps;    // [n_groups] dwords per lane
    const int32_t *b_len;      // [n_groups*64]
    const int32_t *b_orig;     // [n_groups*64] original to-index, -1 = padding lane
    int32_t n_groups;
};

inline FromView from_view(const pfz_strings *F, const pfz_indel_plan *pl)
{
    return FromView{F->chars, F->char_width, F->offsets, pl->lut, pl->lut_len, pl->n_sym + 1};
}

inline EditView edit_view(const pfz_strings *F, const pfz_indel_plan *pl)
{
    EditView v;
    static_cast<FromView &>(v) = from_view(F, pl);
    v.b_packed = pl->packed;
    v.g_off = pl->g_off;
    v.g_steps = pl->g_steps;
    v.b_len = pl->b_len;
    v.b_orig = pl->b_orig;
    v.n_groups = (int32_t)pl->n_groups;
    return v;
}

// ---- the match table ----------------------------------------------------------------------------------------------------------

// the symbol of code unit `at` of a list (the from-side's, or K10's raw to-list)
__device__ inline int edit_symbol(const FromView &V, const void *chars, int width, int64_t at)
{
    const uint32_t c = width == 1 ? (uint32_t)((const uint8_t *)chars)[at] : ((const uint32_t *)chars)[at];
    return c < V.lut_len ? (int)V.lut[c] : 0;
}

__device__ inline void lds_or(uint32_t *p, uint32_t v) { atomicOr(p, v); }
__device__ inline void lds_or(uint64_t *p, uint64_t v) { atomicOr((unsigned long long *)p, (unsigned long long)v); }

// Register form: PM[symbol] is one LDS word, bit i: a[i] == symbol; thread i of the workgroup brings character i.
template <typename WORD> __device__ __forceinline__ void pm_reg_zero(const FromView &V, WORD *pm, int tid, int lanes)
{
    for (int p = tid; p < V.n_sym1; p += lanes) pm[p] = 0;
    __syncthreads();
}

// returns the thread's symbol (0: none), which pm_reg_clear takes
template <typename WORD> __device__ __forceinline__ int pm_reg_set(const FromView &V, WORD *pm, int64_t a0, int la, int tid)
{
    const int my_sym = tid < la ? edit_symbol(V, V.a_chars, V.a_width, a0 + tid) : 0;
    if (my_sym) lds_or(&pm[my_sym], (WORD)1 << tid);
    __syncthreads();
    return my_sym;
}

template <typename WORD> __device__ __forceinline__ void pm_reg_clear(WORD *pm, int my_sym)
{
    if (my_sym) pm[my_sym] = 0;      // clear the entries of this from-string
    __syncthreads();
}

// Global form: PM[symbol] is WA 64-bit words of the workgroup's own table, zero on entry and zero again after every row.
__device__ __forceinline__ void pm_global_set(const FromView &V, uint64_t *pm, int WA, int64_t a0, int la, int tid, int lanes)
{
    for (int p = tid; p < la; p += lanes) {
        const int sy = edit_symbol(V, V.a_chars, V.a_width, a0 + p);
        if (sy) atomicOr((unsigned long long *)&pm[(int64_t)sy * WA + p / 64], 1ull << (p % 64));
    }
    __threadfence_block();
    __syncthreads();
}

__device__ __forceinline__ void pm_global_clear(const FromView &V, uint64_t *pm, int WA, int64_t a0, int la, int tid, int lanes)
{
    for (int p = tid; p < la; p += lanes) {
        const int sy = edit_symbol(V, V.a_chars, V.a_width, a0 + p);
        if (sy) pm[(int64_t)sy * WA + p / 64] = 0ull;
    }
    __threadfence_block();
    __syncthreads();
}

// ---- the best of a row (K8, K9) -----------------------------------------------------------------------------------------------

struct BestRec {
    double score;
    int32_t idx, pad;      // idx < 0: no candidate
};

struct ScoreBest {
    double score;        // -1: nothing yet
    int idx;
};

__device__ inline void best_take(ScoreBest &b, double score, int idx)
{
    if (score > b.score || (score == b.score && idx < b.idx)) {
        b.score = score;
        b.idx = idx;
    }
}

// first maximum of the workgroup: (score desc, original index asc); thread 0 writes the record
__device__ inline void best_of_block(ScoreBest best, double *red_s, int *red_i, BestRec *dst)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) best_take(best, __shfl_xor(best.score, d, 64), __shfl_xor(best.idx, d, 64));
    if (lane == 0) {
        red_s[wave] = best.score;
        red_i[wave] = best.idx;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) best_take(best, red_s[w], red_i[w]);
        dst->score = best.score;
        dst->idx = best.idx == INT_MAX ? -1 : best.idx;
    }
}

// the first maximum of every from-string over the records its launches left (the body of k8_merge and k9_merge)
__device__ __forceinline__ void best_merge(const BestRec *__restrict__ rec, int32_t n_slots, int64_t n_rows, int32_t *__restrict__ out_idx,
                                           double *__restrict__ out_score)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rows) return;
    ScoreBest b = {-1.0, INT_MAX};
    for (int s = 0; s < n_slots; ++s) {
        const BestRec e = rec[r * n_slots + s];
        if (e.idx >= 0) best_take(b, e.score, e.idx);
    }
    out_idx[r] = b.idx == INT_MAX ? -1 : b.idx;
    out_score[r] = b.idx == INT_MAX ? 0.0 : b.score;
}

// a work counter: the wave's sum behind one atomic add (counter == NULL: nobody counts)
template <typename T> __device__ inline void wave_count(unsigned long long *counter, T mine)
{
    if (!counter) return;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(counter, (unsigned long long)mine);
}

// ---- the threshold walk (K11, K12, K13) ---------------------------------------------------------------------------------------

struct WalkArgs : EditView {
    const int32_t *rows;       // from-rows of this launch
    int32_t n_rows;
    int32_t n_to;
    const int32_t *cut;        // the threshold as integer cutoffs, all the kernels know of it: join_kmax by M = max(|a|, |b|)
                               // [longest string + 1] (K11, K12), indel_lmin by S = |a| + |b| [longest sum + 1] (K13)
    unsigned long long *counters;   // optional [3]: pairs in the window, pairs not abandoned, recurrence steps of live lanes
};

// A join's hit sink and the fields it needs: the hits of one wave and group behind one atomic for all of them, each one 64-bit key
// (k11_core.h join_pack: row, to-index, the family's payload -- K11's distance, K13's LCS) written while there is room
struct KeyAppend {
    unsigned long long *total; // every hit
    int32_t self;              // self-join: the plan is the from-list's own, a pair is reported as (min, max)
    uint64_t *keys;            // [capacity] the hits, in the order the waves got there
    unsigned long long capacity;
    __device__ void operator()(bool hit, int row, int orig, int payload) const
    {
        const unsigned long long m = __ballot(hit);
        if (m == 0) return;
        const int lane = threadIdx.x & 63;
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(total, (unsigned long long)__popcll(m));
        base = __shfl(base, 0, 64);
        const unsigned long long pos = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
        if (hit && pos < capacity) keys[pos] = self ? join_pack(min(row, orig), max(row, orig), payload) : join_pack(row, orig, payload);
    }
};

// The components' hit sink: the hits counted as the join counts them (one atomic per wave and group), and each hit lane hooks its
// pair into the forest
struct ForestHook {
    unsigned long long *total; // every hit
    int32_t *parent;           // [n] the forest (k12_core.h)
    __device__ void operator()(bool hit, int row, int orig, int) const
    {
        const unsigned long long m = __ballot(hit);
        if (m == 0) return;
        if ((threadIdx.x & 63) == 0) atomicAdd(total, (unsigned long long)__popcll(m));
        if (hit) uf_unite<UfDeviceOps>(parent, row, orig);
    }
};

struct JoinArgs : WalkArgs {
    KeyAppend sink;
};

struct CompArgs : WalkArgs {   // (n_to: the list's own length)
    ForestHook sink;
};

// the run of groups [lo, hi) a from-string of la characters can have a hit in; wave-uniform
__device__ inline void join_window(const WalkArgs &A, bool self, int la, int *lo_out, int *hi_out)
{
    // the first group whose LONGEST string is long enough: nothing shorter than that passes (a self-join owns nothing shorter than la)
    int lo = 0, hi = A.n_groups;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int last = min(A.n_to, (mid + 1) * 64) - 1;
        const int l = __builtin_amdgcn_readfirstlane(A.b_len[last]);
        if (l >= la || (!self && join_in_window(A.cut[la], la, l))) hi = mid;
        else lo = mid + 1;
    }
    *lo_out = lo;
    // the first group whose SHORTEST string is too long
    hi = A.n_groups;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int l = __builtin_amdgcn_readfirstlane(A.b_len[mid * 64]);
        if (l <= la || join_in_window(A.cut[l], la, l)) lo = mid + 1;
        else hi = mid;
    }
    *hi_out = lo;
}

// is this lane's to-string the row's to walk?  (self-join: the plan's order -- shorter first, then the lower index)
__device__ inline bool join_owned(bool self, int row, int la, int orig, int lb)
{
    return orig >= 0 && (!self || lb > la || (lb == la && orig > row));
}

// a wave's work counts, once, when it has served its last row (three atomics per wave: per row they would queue up on three words)
__device__ inline void join_count(unsigned long long *counters, unsigned long long w, unsigned long long f, unsigned long long s)
{
    if (!counters) return;
    wave_count(counters + 0, w);
    wave_count(counters + 1, f);
    wave_count(counters + 2, s);
}

// The general walk: any from-length, any alphabet.  The match table of the workgroup's from-string (WA words per symbol) and every
// lane's column (VP, VN and, for OSA, the previous D0: WA words each) are in global memory; every group is visited, a lane walks
// its own to-string alone and stops where it is dead.
template <int IDB, bool OSA, bool TWO_LISTS, typename SINK>
__device__ __forceinline__ void walk_general_body(const WalkArgs &A, bool self_arg, const SINK &sink, int32_t WA,
                                                  uint64_t *__restrict__ pm_all, uint64_t *__restrict__ vp_all,
                                                  uint64_t *__restrict__ vn_all, uint64_t *__restrict__ d0_all)
{
    constexpr int PER = 32 / IDB;
    const bool self = !TWO_LISTS || self_arg;
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
        pm_global_set(A, pm, WA, a0, la, tid, 256);
        const uint64_t last = la > 0 ? 1ull << ((la - 1) % 64) : 0ull;
        for (int g = wave; g < A.n_groups; g += 4) {
            const int slot = g * 64 + lane;
            const int orig = A.b_orig[slot];
            const int lb = A.b_len[slot];
            const int km = A.cut[max(la, lb)];
            bool alive = join_owned(self, row, la, orig, lb) && join_in_window(km, la, lb);
            if (!__any(alive)) continue;
            n_win += alive;
            int dist = la;
            if (alive) {
                const uint32_t *gp = A.b_packed + A.g_off[g] + lane;
                lev_column_begin(vp, vn, d0, W, la, 256);
                uint32_t c_prev = 0;                                    // (symbol 0: an empty table entry)
                for (int j = 0; j < lb; ++j) {
                    const uint32_t pk = gp[(int64_t)(j / PER) * 64];
                    const uint32_t c = (pk >> ((j % PER) * IDB)) & ((1u << IDB) - 1u);
                    dist += lev_column_step<OSA>(vp, vn, d0, pm + (int64_t)c * WA, pm + (int64_t)c_prev * WA, W, last, 256);
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
            sink(alive && d <= km, row, orig, d);
        }
        __syncthreads();                                              // every wave is done with the match table
        pm_global_clear(A, pm, WA, a0, la, tid, 256);
    }
    join_count(A.counters, n_win, n_fin, n_steps);
}

// ---- the two ends of a call (K11, K12, K13) -----------------------------------------------------------------------------------

// K11's and K12's cutoff: K9's formula evaluated around a guess, by M = max(|a|, |b|) (k11_core.h); K13 has its own, by S
struct KmaxByM {
    __device__ static int at(double t, int m) { return join_kmax(t, m, m); }
};

// Before the walk, one launch: the cutoff CUT::at(t, i) of every i < n_cut the two lists allow and, where a forest is wanted,
// every position i < n its own root (n = 0: no forest; n_cut = 0: no table)
template <typename CUT>
__global__ __launch_bounds__(256) void walk_begin_kernel(double t, int32_t n_cut, int32_t *__restrict__ cut, int32_t n, int32_t *__restrict__ parent)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_cut) cut[i] = CUT::at(t, (int)i);
    if (i < n) parent[i] = (int32_t)i;
}

template <typename CUT> inline int walk_begin(pfz_ctx *ctx, double t, int32_t n_cut, int32_t *cut, int32_t n, int32_t *parent)
{
    const int64_t n_begin = std::max<int64_t>(n, n_cut);
    hipLaunchKernelGGL(walk_begin_kernel<CUT>, dim3((unsigned)((n_begin + 255) / 256)), dim3(256), 0, ctx->stream, t, n_cut, cut, n, parent);
    PFZ_HIP(hipGetLastError());
    return PFZ_OK;
}
using WalkBegin = int (*)(pfz_ctx *, double, int32_t, int32_t *, int32_t, int32_t *);

// K11's and K12's instance (k12_components.hip has it, once)
int lev_walk_begin(pfz_ctx *ctx, double t, int32_t n_kmax, int32_t *kmax, int32_t n, int32_t *parent);

// a key's payload as K11 reports it: the distance itself
struct LevScore {
    __device__ static int distance(int d, int, int) { return d; }
    __device__ static double similarity(int d, int la, int lb) { return lev_similarity(d, la, lb); }
};

// Behind the sort: the sorted keys -> CSR.  Hit p of the row-major order with SCORE's distance and similarity of its payload, and
// p's share of the row pointers (k11_core.h rows_fill)
template <typename SCORE>
__global__ __launch_bounds__(256) void edit_unpack_kernel(const uint64_t *__restrict__ keys, int64_t total, int64_t n_from,
                                                          const int64_t *__restrict__ f_off, const int64_t *__restrict__ t_off,
                                                          int64_t *__restrict__ row_ptr, int32_t *__restrict__ out_idx,
                                                          int32_t *__restrict__ out_dist, double *__restrict__ out_sim)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= total) return;
    const uint64_t key = keys[p];
    const int row = join_key_row(key), to = join_key_to(key), payload = join_key_dist(key);
    const int la = (int)(f_off[row + 1] - f_off[row]), lb = (int)(t_off[to + 1] - t_off[to]);
    out_idx[p] = to;
    out_dist[p] = SCORE::distance(payload, la, lb);
    out_sim[p] = SCORE::similarity(payload, la, lb);
    rows_fill(p > 0 ? join_key_row(keys[p - 1]) : -1, row, p, total, n_from, row_ptr);
}
using EditUnpack = void (*)(const uint64_t *, int64_t, int64_t, const int64_t *, const int64_t *, int64_t *, int32_t *, int32_t *, double *);

// ---- the host side ------------------------------------------------------------------------------------------------------------

// the register kernels' match table -- a 64-bit word per symbol -- fits 60 KiB of LDS (K4's limit)
inline bool lds_table_fits(const pfz_indel_plan *pl) { return (size_t)(pl->n_sym + 1) * sizeof(uint64_t) <= 60 * 1024; }

// The from-rows [begin, end) by the kernel that serves them: rows[0] of <= 32 characters (32-bit words), rows[1] of 33 .. 64 (64-bit
// words), rows[2] the general kernel's -- every longer row, and every row when the table does not fit LDS; longest: of rows[2].
struct RowClasses {
    std::vector<int32_t> rows[3];
    int64_t longest = 1;
};

inline RowClasses classify_rows(const pfz_strings *F, int64_t begin, int64_t end, bool lds_fits)
{
    RowClasses rc;
    for (int64_t i = begin; i < end; ++i) {
        const int64_t la = F->h_off[(size_t)i + 1] - F->h_off[(size_t)i];
        const int cls = !lds_fits || la > 64 ? 2 : (la > 32 ? 1 : 0);
        rc.rows[cls].push_back((int32_t)i);
        if (cls == 2) rc.longest = std::max(rc.longest, la);
    }
    return rc;
}

// The grid of a general launch (k4_plan.h general_grid_cap: in as wanted, out capped), or the refusal of a match table beyond the
// cap in the words of `entry` ("pfz_lev"), `what` being "a from-string" or "a string"
inline int general_grid(int64_t *grid, int32_t n_sym1, int32_t WA, const char *entry, const char *what, int64_t longest)
{
    const size_t pm_per = (size_t)n_sym1 * (size_t)WA * sizeof(uint64_t);
    if (general_grid_cap(grid, pm_per)) return PFZ_OK;
    set_error("%s: %s of %lld characters with %d alphabet symbols needs a %zu-byte match table", entry, what, (long long)longest, n_sym1 - 1,
              pm_per);
    return PFZ_ERR_UNSUPPORTED;
}

// The global memory of that launch: a match table of n_sym1 x WA words per workgroup, zeroed, and up to three buffers of words[k]
// 64-bit words per lane (0: none), `lanes` lanes per workgroup
struct GeneralBufs {
    DevBuf pm, col[3];
};

inline int general_bufs_alloc(pfz_ctx *ctx, GeneralBufs *b, int64_t grid, int32_t n_sym1, int32_t WA, const int32_t (&words)[3], int lanes)
{
    const size_t pm_bytes = (size_t)n_sym1 * (size_t)WA * sizeof(uint64_t) * (size_t)grid;
    PFZ_TRY(b->pm.alloc(ctx, pm_bytes));
    for (int k = 0; k < 3; ++k)
        if (words[k] > 0) PFZ_TRY(b->col[k].alloc(ctx, (size_t)grid * (size_t)words[k] * (size_t)lanes * sizeof(uint64_t)));
    PFZ_HIP(hipMemsetAsync(b->pm.p, 0, pm_bytes, ctx->stream));
    return PFZ_OK;
}

// f(std::integral_constant<int, IDB>, std::integral_constant<bool, OSA>) for the plan's symbol width (8 or 16 bits) and the scorer
template <typename F> inline void dispatch_idb_osa(int idb, bool osa, F &&f)
{
    if (idb == 8 && !osa) f(std::integral_constant<int, 8>{}, std::false_type{});
    else if (idb == 8) f(std::integral_constant<int, 8>{}, std::true_type{});
    else if (!osa) f(std::integral_constant<int, 16>{}, std::false_type{});
    else f(std::integral_constant<int, 16>{}, std::true_type{});
}

// f(std::integral_constant<int, IDB>) for the plan's symbol width alone
template <typename F> inline void dispatch_idb(int idb, F &&f)
{
    if (idb == 8) f(std::integral_constant<int, 8>{});
    else f(std::integral_constant<int, 16>{});
}

// The launches of a threshold call over the row classes, on the context's stream, A.rows / A.n_rows set for each:
//   reg(WORD{}, grid, lds)   launches the register kernel of word type WORD -- uint32_t for rc.rows[0], uint64_t for rc.rows[1];
//   gen(grid, WA, bufs)      launches the general kernel for rc.rows[2] under the scope `scope_general`, bufs being the match tables
//                            and cols[k] * WA words per lane in column buffer k (general_bufs_alloc).
// entry, what: general_grid's, for the refusal.
template <typename ARGS, typename REG, typename GEN>
inline int walk_launch(pfz_ctx *ctx, const RowClasses &rc, DevBuf (&d_rows)[3], ARGS &A, const int32_t (&cols)[3], const char *entry,
                       const char *what, const char *scope_general, REG &&reg, GEN &&gen)
{
    const int64_t max_grid = (int64_t)ctx->prop.multiProcessorCount * 8;
    for (int c = 0; c < 2; ++c) {
        if (rc.rows[c].empty()) continue;
        A.rows = d_rows[c].as<int32_t>();
        A.n_rows = (int32_t)rc.rows[c].size();
        const dim3 grid((unsigned)std::min<int64_t>(A.n_rows, max_grid));
        if (c == 0) reg(uint32_t{}, grid, (size_t)A.n_sym1 * sizeof(uint32_t));
        else reg(uint64_t{}, grid, (size_t)A.n_sym1 * sizeof(uint64_t));
        PFZ_HIP(hipGetLastError());
    }
    if (!rc.rows[2].empty()) {
        A.rows = d_rows[2].as<int32_t>();
        A.n_rows = (int32_t)rc.rows[2].size();
        const int32_t WA = (int32_t)((rc.longest + 63) / 64);
        int64_t grid = std::min<int64_t>(A.n_rows, max_grid);
        PFZ_TRY(general_grid(&grid, A.n_sym1, WA, entry, what, rc.longest));
        ProfScope ps(ctx, scope_general);
        GeneralBufs gb;
        PFZ_TRY(general_bufs_alloc(ctx, &gb, grid, A.n_sym1, WA, {cols[0] * WA, cols[1] * WA, cols[2] * WA}, 256));
        gen(dim3((unsigned)grid), WA, gb);
        PFZ_HIP(hipGetLastError());
    }
    return PFZ_OK;
}

// the from-rows of each class on the device
inline int rows_upload(pfz_ctx *ctx, const RowClasses &rc, DevBuf (&d_rows)[3])
{
    for (int c = 0; c < 3; ++c)
        if (!rc.rows[c].empty()) PFZ_TRY(d_rows[c].upload(ctx, rc.rows[c]));
    return PFZ_OK;
}

// What a join entry is called: in messages, its key's payload there ("distance"), and its two profiling scopes
struct JoinNames {
    const char *entry, *payload, *scope, *scope_sort_unpack;
};

// The host side of a join call (K11, K13): limits, the empty result, the plan, the row classes, keys and state, the cutoff table
// (`begin` over n_cut entries), the walk -- launch(pl, rc, d_rows, A): the family's walk_launch -- the total and the counters read
// back, the capacity verdict, and behind it the sort, `unpack` and the four downloads.
template <typename LAUNCH>
inline int edit_join_run(pfz_ctx *ctx, const JoinNames &nm, const pfz_strings *F, const pfz_strings *T, bool self, double t, int64_t capacity,
                         int64_t n_cut, WalkBegin begin, LAUNCH &&launch, EditUnpack unpack, int64_t *out_row_ptr, int32_t *out_idx,
                         int32_t *out_dist, double *out_sim, int64_t *out_total, int64_t *out_counters)
{
    PFZ_HIP(hipSetDevice(ctx->device));
    if (T->n > kJoinMaxStrings || F->n > kJoinMaxStrings || T->max_len > kJoinMaxLength || F->max_len > kJoinMaxLength) {
        set_error("%s: a list of more than %lld strings or a string of more than %lld characters does not fit the packed hit "
                  "(24-bit indices, 16-bit %s)", nm.entry, (long long)kJoinMaxStrings, (long long)kJoinMaxLength, nm.payload);
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

    DevBuf d_rows[3], d_cut, d_keys, d_sorted, d_state, d_ptr, d_idx, d_dist, d_sim;
    PFZ_TRY(rows_upload(ctx, rc, d_rows));
    PFZ_TRY(d_keys.alloc(ctx, (size_t)capacity * sizeof(uint64_t)));
    PFZ_TRY(d_cut.alloc(ctx, (size_t)n_cut * sizeof(int32_t)));
    PFZ_TRY(begin(ctx, t, (int32_t)n_cut, d_cut.as<int32_t>(), 0, nullptr));
    PFZ_TRY(d_state.alloc(ctx, 4 * sizeof(unsigned long long)));      // the total, then the three counters
    PFZ_HIP(hipMemsetAsync(d_state.p, 0, 4 * sizeof(unsigned long long), ctx->stream));

    JoinArgs A;
    static_cast<EditView &>(A) = edit_view(F, pl);
    A.n_to = (int32_t)n_to;
    A.cut = d_cut.as<int32_t>();
    A.counters = out_counters ? d_state.as<unsigned long long>() + 1 : nullptr;
    A.sink = KeyAppend{d_state.as<unsigned long long>(), self ? 1 : 0, d_keys.as<uint64_t>(), (unsigned long long)capacity};

    unsigned long long state[4];
    {
        ProfScope ps_all(ctx, nm.scope);
        PFZ_TRY(launch(pl, rc, d_rows, A));
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
        ProfScope ps(ctx, nm.scope_sort_unpack);
        PFZ_TRY(d_sorted.alloc(ctx, (size_t)sort_codes_capacity(total) * sizeof(uint64_t)));
        PFZ_TRY(sort_codes_u64(ctx, d_keys.as<uint64_t>(), d_sorted.as<uint64_t>(), total));
        PFZ_TRY(d_ptr.alloc(ctx, (size_t)(n_from + 1) * sizeof(int64_t)));
        PFZ_TRY(d_idx.alloc(ctx, (size_t)total * sizeof(int32_t)));
        PFZ_TRY(d_dist.alloc(ctx, (size_t)total * sizeof(int32_t)));
        PFZ_TRY(d_sim.alloc(ctx, (size_t)total * sizeof(double)));
        hipLaunchKernelGGL(unpack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, d_sorted.as<uint64_t>(), total, n_from,
                           F->offsets, T->offsets, d_ptr.as<int64_t>(), d_idx.as<int32_t>(), d_dist.as<int32_t>(), d_sim.as<double>());
        PFZ_HIP(hipGetLastError());
    }
    PFZ_TRY(copy_d2h(ctx, out_row_ptr, d_ptr.p, (size_t)(n_from + 1) * sizeof(int64_t)));
    PFZ_TRY(copy_d2h(ctx, out_idx, d_idx.p, (size_t)total * sizeof(int32_t)));
    PFZ_TRY(copy_d2h(ctx, out_dist, d_dist.p, (size_t)total * sizeof(int32_t)));
    PFZ_TRY(copy_d2h(ctx, out_sim, d_sim.p, (size_t)total * sizeof(double)));
    PFZ_HIP(hipStreamSynchronize(ctx->stream));
    return PFZ_OK;
}

// What a components entry is called: in messages, what of its strings' lengths must fit 32 bits, and its two profiling scopes
struct CompNames {
    const char *entry, *lengths, *scope, *scope_flatten;
};

// The host side of a components call (K12, K13): the empty result, limits, the plan, the row classes, the forest and the state,
// `begin` (the cutoff table over n_cut entries and the forest's roots, one launch), the walk -- launch(pl, rc, d_rows, A) -- the
// flattening, and the state and the labels read back.
template <typename LAUNCH>
inline int edit_comp_run(pfz_ctx *ctx, const CompNames &nm, const pfz_strings *F, double t, int64_t n_cut, WalkBegin begin, LAUNCH &&launch,
                         int32_t *out_label, int64_t *out_pairs, int64_t *out_components, int64_t *out_counters)
{
    PFZ_HIP(hipSetDevice(ctx->device));
    *out_pairs = *out_components = 0;
    if (out_counters) out_counters[0] = out_counters[1] = out_counters[2] = 0;
    const int64_t n = F->n;
    if (n == 0) return PFZ_OK;
    if (n > (int64_t)INT_MAX - 64 || n_cut > (int64_t)INT_MAX) {
        set_error("%s: %lld strings, the longest of %lld characters: positions (padded to groups of 64) and %s are 32-bit", nm.entry,
                  (long long)n, (long long)F->max_len, nm.lengths);
        return PFZ_ERR_UNSUPPORTED;
    }
    const pfz_indel_plan *pl;
    PFZ_TRY(indel_plan_get(ctx, F, &pl));
    const RowClasses rc = classify_rows(F, 0, n, lds_table_fits(pl));      // (the join's three classes)

    DevBuf d_rows[3], d_cut, d_state;
    ForestRun forest;
    PFZ_TRY(rows_upload(ctx, rc, d_rows));
    PFZ_TRY(d_cut.alloc(ctx, (size_t)n_cut * sizeof(int32_t)));
    PFZ_TRY(forest.alloc(ctx, n));
    PFZ_TRY(d_state.alloc(ctx, 5 * sizeof(unsigned long long)));      // the hits, the three counters, the roots
    PFZ_HIP(hipMemsetAsync(d_state.p, 0, 5 * sizeof(unsigned long long), ctx->stream));
    PFZ_TRY(begin(ctx, t, (int32_t)n_cut, d_cut.as<int32_t>(), forest.n, forest.parent.as<int32_t>()));

    CompArgs A;
    static_cast<EditView &>(A) = edit_view(F, pl);
    A.n_to = (int32_t)n;
    A.cut = d_cut.as<int32_t>();
    A.counters = out_counters ? d_state.as<unsigned long long>() + 1 : nullptr;
    A.sink = ForestHook{d_state.as<unsigned long long>(), forest.parent.as<int32_t>()};
    {
        ProfScope ps_all(ctx, nm.scope);
        PFZ_TRY(launch(pl, rc, d_rows, A));
    }
    {
        ProfScope ps(ctx, nm.scope_flatten);
        PFZ_TRY(forest.flatten(ctx, d_state.as<unsigned long long>() + 4));
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

}  // namespace pfz
