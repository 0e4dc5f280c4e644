// K15 -- the threshold forms of K3: every pair of TF-IDF rows whose sparse cosine is >= t (pfz_cossim_join, what TFIDF.join runs),
// and the connected components of that relation over one list (pfz_cossim_components).  K11 / K12 ask the same two questions of
// an edit distance, K14 of the dense cosine; here the score is K3's and the work is K3's row walk over the inverted index.
//
// Mapping to CDNA4: the row-major K3 (k3_cossim_topn.hip) with another end, the way K14 is another end of K5's tile loop.
//   * one one-wave workgroup per from-row at a time, the to-blocks in the inner loop; a lane owns an n-gram of the row and its
//     (k, b) posting list; the scatter is scatter_pieces of k3_core.h, called; the two table entries of the next block are one
//     block ahead in flight; rows of more than 64 n-grams go through the chunk loop.  int acc[C] sits at LDS address 0 (checked).
//     The arithmetic is K3's, so the integer sum of a pair is the one pfz_cossim_topn gets.
//     The row loop below repeats some forty lines of k3_cossim_topn_kernel ON PURPOSE: hoisting them out would move the headline
//     kernel's code, which is held to its measured time.  A change to one of the two loops is to be made in the other.
//   * an integer cutoff instead of a running threshold: the host finds smin, the smallest sum whose float32 score passes
//     (k15_core.h), and the kernel compares integers.  No candidate buffer, no compaction, no warm start.
//   * the sweep reads and clears the accumulators as sweep_block does (int4 pairs, v_max3_i32 pre-test against smin - 1).  A step
//     in which no lane has a hit touches no memory.  A step with hits counts them per lane (0 .. 8), takes one wave prefix sum,
//     reserves room for all of them with ONE atomic add (K14's append) and writes row << 32 | col with the float32 score bits
//     beside it -- (float)sum * inv_scale, the expression of k3_cossim_topn_kernel's last lines -- while there is room: hits
//     beyond the capacity are counted, never written.  Components (kComp): each hit lane unites row and col in K12's forest
//     (uf_unite<UfDeviceOps>) and nothing is stored.
//   * the self-join walks every unordered pair once: K3's sums are symmetric bit for bit (the scale is a power of two and the
//     fp32 product commutes), so row i starts at its own block i / C, does not wrap, and keeps only columns j > i.  The rows are
//     uneven (the first ones walk every block, the last ones one); the hardware dispatcher balances them, as it does for K3.
//   * an exact upper bound skips whole blocks (k15_core.h): one wave reduction of the squared values whose list is non-empty,
//     and neither scatter nor sweep when no sum of the block can reach smin.  Rows of at most 64 n-grams only.
//   * counters, kept in wave-uniform registers and added once per from-row: (row, block) visits that had postings, those of
//     them the bound skipped, sweep steps that contained a hit.  The adds of the rows go round 256 lines of counters that the
//     host sums: every row adding to the same word cost more than the counters are worth.
//   * pfz_cossim_join_dev leaves the join on the device: the same launch (k15_launch<false>, called) and sort_pairs_u64, the sorted
//     keys and scores owned by a pfz_pairs handle that K16's key entries walk (k16_pairs_join.hip, K17); the capacity is handled
//     inside -- a first launch with room for the caller's hint, one repeat with the exact total when that was too little.
// LDS: 4 C + 256 bytes (the accumulators and the scatter's 64 markers), below the 4 C + 768 of k3_cossim_topn_kernel<C, 96>, so
// the 18 workgroups per CU at C = 2048 are kept.  Large to-sides run this form too: there is no lock-step variant.
#include "k3_core.h"
#include "k12_core.h"
#include "k15_core.h"

#include <algorithm>
#include <cmath>

namespace pfz {

// The call's state words: [0] the hits, [1] the components' roots; from kCounterBase on kCounterSlots lines of 64 bytes, each
// [0] visits, [1] visits skipped, [2] sweep steps with a hit, which the host adds up (k15_counters).
constexpr int kCounterBase = 8, kCounterSlots = 256, kStateWords = kCounterBase + kCounterSlots * 8;

struct SparseJoinArgs {
    const int32_t *a_indptr, *a_idx;   // the from-rows (CSR)
    const float *a_val;
    int32_t n_a;
    const int32_t *tab;                // the to-side's inverted index (pfz_index)
    const int2 *post;
    int32_t nb;
    int32_t self;                      // the from-rows ARE the indexed rows: blocks from row / C on, columns > row only
    int32_t smin;                      // hit iff sum >= smin (>= 1)
    float scale, inv_scale, max_norm;  // K3's fixed point; the index's bound of a to-row's norm
    unsigned long long *state;         // [kStateWords]: [0] hits, [1] (components) roots, then the counter slots
    uint64_t *keys;                    // join: [capacity] row << 32 | col, in the order the waves got there ...
    float *vals;                       // ... and the scores beside them
    unsigned long long capacity;
    int32_t *parent;                   // components: [n_a] the forest (k12_core.h)
};

// the wave's sum of a float (lane 63 of a DPP prefix sum, as dpp_max_scan: a lane without a source adds 0)
__device__ inline float wave_sum_f32(float v)
{
#define PFZ_FADD_STEP(ctrl, rmask) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, rmask, 0xf, false));
    PFZ_FADD_STEP(0x111, 0xf)
    PFZ_FADD_STEP(0x112, 0xf)
    PFZ_FADD_STEP(0x114, 0xf)
    PFZ_FADD_STEP(0x118, 0xf)
    PFZ_FADD_STEP(0x142, 0xa)
    PFZ_FADD_STEP(0x143, 0xc)
#undef PFZ_FADD_STEP
    return readlane_f(v, 63);
}

// Read, clear and test one block of accumulators against smin: int4 slots [0, N4) of the block whose first column is col0.
// Returns the number of steps that held a hit.
template <int N4, bool kComp>
__device__ inline int k15_sweep(int4 *acc4, const SparseJoinArgs &P, int row, int col0, int lane, int zero)
{
    static_assert(N4 % 128 == 0, "a wave sweeps whole 128-slot steps");
    const int below = P.smin - 1;
    const int first = P.self ? row + 1 : 0;      // the smallest column that counts
    int hit_steps = 0;
#pragma unroll 2
    for (int t = 0; t < N4 / 128; ++t) {
        const int i0 = t * 128 + lane, i1 = i0 + 64;
        const int4 v0 = acc4[i0], v1 = acc4[i1];
        acc4[i0] = make_int4(zero, zero, zero, zero);
        acc4[i1] = make_int4(zero, zero, zero, zero);
        const int mx = max3i(max3i(v0.x, v0.y, v0.z), max3i(v0.w, v1.x, v1.y), max3i(v1.z, v1.w, v1.w));
        if (__ballot(mx > below) == 0) continue;
        // (a column beyond the to-side has no postings: its sum is 0 < smin)
        const int vv[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
        const int j0 = col0 + i0 * 4, j1 = col0 + i1 * 4;
        uint32_t mask = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int j = (c < 4 ? j0 : j1) + (c & 3);
            mask |= (uint32_t)(vv[c] > below && j >= first) << c;
        }
        if (__ballot(mask != 0) == 0) continue;      // (a self-join: the sums at or below the diagonal)
        ++hit_steps;
        const int mine = __popc(mask), upto = dpp_add_scan(mine), all = __builtin_amdgcn_readlane(upto, 63);
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(P.state, (unsigned long long)all);
        if (kComp) {
#pragma unroll
            for (int c = 0; c < 8; ++c)
                if ((mask >> c) & 1) uf_unite<UfDeviceOps>(P.parent, row, (c < 4 ? j0 : j1) + (c & 3));
            continue;
        }
        base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32)) << 32) |
               (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
        unsigned long long pos = base + (unsigned long long)(upto - mine);
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if ((mask >> c) & 1) {
                if (pos < P.capacity) {
                    P.keys[pos] = (uint64_t)(uint32_t)row << 32 | (uint64_t)(uint32_t)((c < 4 ? j0 : j1) + (c & 3));
                    P.vals[pos] = (float)vv[c] * P.inv_scale;
                }
                ++pos;
            }
    }
    return hit_steps;
}

// C to-rows per block; the (one-wave) workgroup owns one from-row at a time
template <int C, bool kComp>
__global__ __launch_bounds__(64) void k15_sparse_join_kernel(SparseJoinArgs P)
{
    // accumulators first: this struct is the kernel's only LDS object, so they land at LDS address 0 and a posting's byte
    // offset IS its LDS address (run_steps of k3_core.h)
    __shared__ __attribute__((aligned(16))) struct {
        int acc[C];
        int mark[64];     // the scatter's marker scratch
    } sm;
    int *const acc = sm.acc;
    int *const mark = sm.mark;
    if ((uint32_t)(uintptr_t)sm.acc != 0u) __builtin_trap();   // layout assumption of run_steps()
    const int lane = threadIdx.x;
    int4 *acc4 = (int4 *)acc;
    constexpr int N4 = C / 4;
    int zero;
    asm volatile("v_mov_b32 %0, 0" : "=v"(zero));
    for (int t = lane; t < C / 4; t += 64) acc4[t] = make_int4(0, 0, 0, 0);
    wave_sync();
    const char *post_bytes = (const char *)P.post;
    const int src4 = (4 * (lane & 15) + (lane >> 4)) * 4;
    const int sub8 = (lane & 15) * 8;
    const int dummy_addr = 0;
    const int32_t *__restrict__ a_indptr = P.a_indptr, *__restrict__ a_idx = P.a_idx, *__restrict__ tab = P.tab;
    const float *__restrict__ a_val = P.a_val;
    const int nb = P.nb;
    const float scale = P.scale;

    for (int row = blockIdx.x; row < P.n_a; row += gridDim.x) {
        const int p0 = a_indptr[row], p1 = a_indptr[row + 1];
        const int nnz = p1 - p0;
        // a self-join starts with the block that holds the row itself and does not wrap: the blocks in front of it hold columns
        // j < i only, pairs that row j reports
        const int b_first = P.self ? row / C : 0;
        if (b_first >= nb) continue;
        const bool prune = nnz <= 64;
        int visits = 0, skipped = 0, hit_steps = 0;
        // ---- from here to the sweep: the row loop of k3_cossim_topn_kernel (see the header) ----
        int cur0 = 0, nxt0 = 0;
        float as0 = 0.f;
        const bool have0 = lane < nnz;
        const int32_t *trow = tab;
        if (have0) {
            as0 = a_val[p0 + lane] * scale;
            trow = tab + (int64_t)a_idx[p0 + lane] * nb;
            cur0 = trow[b_first];
            nxt0 = trow[b_first + 1];
        }
        for (int b = b_first; b < nb; ++b) {
            const int s = cur0, e = have0 ? nxt0 : cur0;
            bool touched = __ballot(e > s) != 0;
            bool skip = false;
            if (touched && prune) {
                skip = k15_block_skippable(wave_sum_f32(e > s ? as0 * as0 : 0.f), P.max_norm, P.smin);
                visits += 1;
                skipped += skip;
                touched = !skip;
            }
            if (touched) scatter_pieces(acc, post_bytes, mark, e - s, s, as0, lane, src4, sub8, dummy_addr);
            // prefetch of the next block's table entries (tab has V*nb+2 slots), issued behind the block's posting loads
            if (have0 && b + 1 < nb) {
                cur0 = trow[b + 1];
                nxt0 = trow[b + 2];
            }
            for (int c0 = p0 + 64; c0 < p1; c0 += 64) {  // rows with more than 64 n-grams (unpruned)
                int s2 = 0, e2 = 0;
                float as2 = 0.f;
                if (c0 + lane < p1) {
                    const int k = a_idx[c0 + lane];
                    as2 = a_val[c0 + lane] * scale;
                    s2 = tab[(int64_t)k * nb + b];
                    e2 = tab[(int64_t)k * nb + b + 1];
                }
                if (__ballot(e2 > s2)) {
                    touched = true;
                    scatter_pieces(acc, post_bytes, mark, e2 - s2, s2, as2, lane, src4, sub8, dummy_addr);
                }
            }
            if (!prune) visits += touched;
            if (touched) {
                wave_sync();      // the wave's LDS operations execute in order: the block's updates are in acc
                hit_steps += k15_sweep<N4, kComp>(acc4, P, row, b * C, lane, zero);
                wave_sync();      // acc is zero again
            }
        }
        if (lane == 0) {
            // once per from-row, into one of kCounterSlots 64-byte lines: 100 000 rows adding to ONE word took longer than a
            // counter's worth (the adds of a word are served one after the other)
            unsigned long long *ctr = P.state + kCounterBase + (size_t)(blockIdx.x % kCounterSlots) * 8;
            if (visits) atomicAdd(ctr, (unsigned long long)visits);
            if (skipped) atomicAdd(ctr + 1, (unsigned long long)skipped);
            if (hit_steps) atomicAdd(ctr + 2, (unsigned long long)hit_steps);
        }
    }
}

template <bool kComp> static int k15_launch(pfz_ctx *ctx, const pfz_index *ix, const SparseJoinArgs &P)
{
    const int64_t max_grid = (int64_t)ctx->prop.multiProcessorCount * 16 * 64 * 8;
    const unsigned grid = (unsigned)(P.n_a < max_grid ? P.n_a : max_grid);
#define PFZ_K15_CASE(CC) \
    case CC: hipLaunchKernelGGL((k15_sparse_join_kernel<CC, kComp>), dim3(grid), dim3(64), 0, ctx->stream, P); break;
    switch (ix->block_cols) {
        PFZ_K15_CASE(1024)
        PFZ_K15_CASE(1536)
        PFZ_K15_CASE(2048)
        PFZ_K15_CASE(4096)
    default:
        set_error("pfz_cossim_join: no kernel for block size %d", ix->block_cols);
        return PFZ_ERR_INVALID;
    }
#undef PFZ_K15_CASE
    PFZ_HIP(hipGetLastError());
    return PFZ_OK;
}

// the counter slots added up into the caller's int64[3] (NULL: not wanted)
static void k15_counters(const std::vector<unsigned long long> &state, int64_t *out_counters)
{
    if (!out_counters) return;
    for (int c = 0; c < 3; ++c) {
        out_counters[c] = 0;
        for (int slot = 0; slot < kCounterSlots; ++slot) out_counters[c] += (int64_t)state[(size_t)kCounterBase + (size_t)slot * 8 + c];
    }
}

// the argument block of a call; false: no sum below 2^31 passes, there is nothing to launch
static bool k15_args(const pfz_index *ix, const pfz_csr *A, bool self, double t, SparseJoinArgs *P)
{
    float scale, inv_scale;
    int32_t thr0;
    k3_fixed_point(A, ix, 0.f, &scale, &inv_scale, &thr0);
    *P = SparseJoinArgs{};
    P->a_indptr = A->indptr;
    P->a_idx = A->indices;
    P->a_val = A->data;
    P->n_a = (int32_t)A->n_rows;
    P->tab = ix->tab;
    P->post = ix->post;
    P->nb = ix->n_blocks;
    P->self = self ? 1 : 0;
    P->smin = k15_cutoff(inv_scale, t);
    P->scale = scale;
    P->inv_scale = inv_scale;
    P->max_norm = ix->max_norm;
    return P->smin >= 1;
}

static int sparse_join_run(pfz_ctx *ctx, const pfz_index *ix, const pfz_csr *A, bool self, double t, int64_t capacity,
                           int64_t *out_row_ptr, int32_t *out_idx, float *out_sim, int64_t *out_total, int64_t *out_counters)
{
    PFZ_HIP(hipSetDevice(ctx->device));
    *out_total = 0;
    if (out_counters) out_counters[0] = out_counters[1] = out_counters[2] = 0;
    const int64_t n_from = A->n_rows;
    SparseJoinArgs P;
    if (n_from == 0 || ix->n_rows == 0 || !k15_args(ix, A, self, t, &P)) {
        for (int64_t r = 0; r <= n_from; ++r) out_row_ptr[r] = 0;
        return PFZ_OK;
    }
    DevBuf d_keys, d_vals, d_state;
    PFZ_TRY(d_keys.alloc(ctx, (size_t)capacity * sizeof(uint64_t)));
    PFZ_TRY(d_vals.alloc(ctx, (size_t)capacity * sizeof(float)));
    PFZ_TRY(d_state.alloc(ctx, kStateWords * sizeof(unsigned long long)));
    PFZ_HIP(hipMemsetAsync(d_state.p, 0, kStateWords * sizeof(unsigned long long), ctx->stream));
    P.keys = d_keys.as<uint64_t>();
    P.vals = d_vals.as<float>();
    P.capacity = (unsigned long long)capacity;
    P.state = d_state.as<unsigned long long>();
    std::vector<unsigned long long> state(kStateWords);
    {
        ProfScope ps(ctx, "k15_join");
        PFZ_TRY(k15_launch<false>(ctx, ix, P));
        PFZ_TRY(copy_d2h(ctx, state.data(), d_state.p, kStateWords * sizeof(unsigned long long)));      // (waits for the kernel)
    }
    const int64_t total = (int64_t)state[0];
    *out_total = total;
    k15_counters(state, out_counters);
    if (total > capacity) return PFZ_OK;       // the caller's buffers stay as they are: it repeats the call with room for `total`
    return join_sort_unpack(ctx, "k15_sort_unpack", d_keys.as<uint64_t>(), d_vals.as<uint32_t>(), total, n_from, out_row_ptr, out_idx,
                            out_sim);
}

// The hits a first launch of pfz_cossim_join_dev has room for when its caller gives no hint: pfz_cossim_join's callers' guess
constexpr int64_t kJoinDevDefaultRoom = 4096, kJoinDevDefaultPerRow = 4;

static void pairs_handle_free(pfz_pairs *h)
{
    if (!h) return;
    if (h->keys) pool_free(h->keys);
    if (h->vals) pool_free(h->vals);
    delete h;
}

// The join with its result left in HBM: the walk (at most twice: the capacity is handled here) and the sort; nothing is unpacked,
// nothing but the state words comes to the host.
static int sparse_join_dev_run(pfz_ctx *ctx, const pfz_index *ix, const pfz_csr *A, bool self, double t, int64_t hint, pfz_pairs **out,
                               int64_t *out_counters)
{
    PFZ_HIP(hipSetDevice(ctx->device));
    if (out_counters) out_counters[0] = out_counters[1] = out_counters[2] = 0;
    Owner<pfz_pairs, pairs_handle_free> h(new pfz_pairs);
    h->ctx = ctx;
    h->n_from = A->n_rows;
    h->n_to = ix->n_rows;
    h->self = self;
    SparseJoinArgs P;
    if (h->n_from == 0 || h->n_to == 0 || !k15_args(ix, A, self, t, &P)) {
        *out = h.release();
        return PFZ_OK;
    }
    DevBuf d_keys, d_vals, d_state;
    PFZ_TRY(d_state.alloc(ctx, kStateWords * sizeof(unsigned long long)));
    P.state = d_state.as<unsigned long long>();
    std::vector<unsigned long long> state(kStateWords);
    int64_t room = hint > 0 ? hint : std::max(kJoinDevDefaultRoom, kJoinDevDefaultPerRow * h->n_from), total = 0;
    for (int pass = 0; pass < 2; ++pass) {
        PFZ_TRY(d_keys.alloc(ctx, (size_t)room * sizeof(uint64_t)));
        PFZ_TRY(d_vals.alloc(ctx, (size_t)room * sizeof(float)));
        PFZ_HIP(hipMemsetAsync(d_state.p, 0, kStateWords * sizeof(unsigned long long), ctx->stream));
        P.keys = d_keys.as<uint64_t>();
        P.vals = d_vals.as<float>();
        P.capacity = (unsigned long long)room;
        {
            ProfScope ps(ctx, "k15_join");
            PFZ_TRY(k15_launch<false>(ctx, ix, P));
            PFZ_TRY(copy_d2h(ctx, state.data(), d_state.p, kStateWords * sizeof(unsigned long long)));      // (waits for the kernel)
        }
        total = (int64_t)state[0];
        if (total >= ((int64_t)1 << 31)) {
            set_error("pfz_cossim_join_dev: %lld pairs are more than the limit of 2^31 - 1 (the scan of the kernels that walk them is 32-bit)",
                      (long long)total);
            return PFZ_ERR_UNSUPPORTED;
        }
        if (total <= room) break;
        room = total;      // the ONE repeat, with the exact total
    }
    k15_counters(state, out_counters);
    if (total > 0) {
        ProfScope ps(ctx, "k15_sort");
        DevBuf d_skeys, d_svals;
        const size_t cap = (size_t)sort_codes_capacity(total);
        PFZ_TRY(d_skeys.alloc(ctx, cap * sizeof(uint64_t)));
        PFZ_TRY(d_svals.alloc(ctx, cap * sizeof(uint32_t)));
        PFZ_TRY(sort_pairs_u64(ctx, d_keys.as<uint64_t>(), d_vals.as<uint32_t>(), d_skeys.as<uint64_t>(), d_svals.as<uint32_t>(), total));
        h->keys = (uint64_t *)d_skeys.release();
        h->vals = (uint32_t *)d_svals.release();
        h->count = total;
    }
    *out = h.release();
    return PFZ_OK;
}

static int sparse_comp_run(pfz_ctx *ctx, const pfz_index *ix, const pfz_csr *A, double t, int32_t *out_label, int64_t *out_pairs,
                           int64_t *out_components, int64_t *out_counters)
{
    PFZ_HIP(hipSetDevice(ctx->device));
    *out_pairs = *out_components = 0;
    if (out_counters) out_counters[0] = out_counters[1] = out_counters[2] = 0;
    const int64_t n = A->n_rows;
    if (n == 0) return PFZ_OK;
    SparseJoinArgs P;
    const bool any = k15_args(ix, A, true, t, &P);
    ForestRun forest;
    DevBuf d_state;
    PFZ_TRY(forest.alloc(ctx, n));
    PFZ_TRY(d_state.alloc(ctx, kStateWords * sizeof(unsigned long long)));
    PFZ_HIP(hipMemsetAsync(d_state.p, 0, kStateWords * sizeof(unsigned long long), ctx->stream));
    P.parent = forest.parent.as<int32_t>();
    P.state = d_state.as<unsigned long long>();
    {
        ProfScope ps(ctx, "k15_components");
        PFZ_TRY(forest.begin(ctx));
        if (any) PFZ_TRY(k15_launch<true>(ctx, ix, P));
        PFZ_TRY(forest.flatten(ctx, P.state + 1));
    }
    std::vector<unsigned long long> state(kStateWords);
    PFZ_TRY(copy_d2h(ctx, state.data(), d_state.p, kStateWords * sizeof(unsigned long long)));
    PFZ_TRY(forest.download(ctx, out_label));
    *out_pairs = (int64_t)state[0];
    *out_components = (int64_t)state[1];
    k15_counters(state, out_counters);
    return PFZ_OK;
}

static int sparse_join_operands(const char *who, const pfz_index *ix, const pfz_csr *A, double t, bool self)
{
    PFZ_REQUIRE(!std::isnan(t) && t >= 0.0 && t <= 1.0, "%s: min_similarity %g is not a number in [0, 1]", who, t);
    PFZ_REQUIRE(A->n_cols == ix->n_cols, "%s: from-matrix has %lld columns, index has %lld", who, (long long)A->n_cols,
                (long long)ix->n_cols);
    PFZ_REQUIRE(!self || A->serial == ix->src_serial,
                "%s: the self-join takes the matrix the index was built from (every unordered pair once needs one list)", who);
    if (A->n_rows >= ((int64_t)1 << 31) || ix->n_rows >= ((int64_t)1 << 31)) {
        set_error("%s: %lld x %lld rows exceed the 32-bit positions", who, (long long)A->n_rows, (long long)ix->n_rows);
        return PFZ_ERR_UNSUPPORTED;
    }
    return PFZ_OK;
}

}  // namespace pfz

using namespace pfz;

extern "C" {

int pfz_cossim_join(pfz_ctx *ctx, const pfz_index *to_index, const pfz_csr *from_matrix, int32_t self_join, double min_similarity,
                    int64_t capacity, int64_t *out_row_ptr, int32_t *out_idx, float *out_sim, int64_t *out_total, int64_t *out_counters)
{
    PFZ_REQUIRE(ctx && to_index && from_matrix, "pfz_cossim_join: NULL argument");
    PFZ_REQUIRE(capacity >= 0, "pfz_cossim_join: capacity %lld < 0", (long long)capacity);
    PFZ_REQUIRE(out_row_ptr && out_total, "pfz_cossim_join: NULL out_row_ptr / out_total");
    PFZ_REQUIRE(capacity == 0 || (out_idx && out_sim), "pfz_cossim_join: NULL output with capacity %lld", (long long)capacity);
    PFZ_TRY(sparse_join_operands("pfz_cossim_join", to_index, from_matrix, min_similarity, self_join != 0));
    return sparse_join_run(ctx, to_index, from_matrix, self_join != 0, min_similarity, capacity, out_row_ptr, out_idx, out_sim, out_total,
                           out_counters);
}

int pfz_cossim_join_dev(pfz_ctx *ctx, const pfz_index *to_index, const pfz_csr *from_matrix, int32_t self_join, double min_similarity,
                        int64_t capacity_hint, pfz_pairs **out, int64_t *out_counters)
{
    PFZ_REQUIRE(ctx && to_index && from_matrix && out, "pfz_cossim_join_dev: NULL argument");
    PFZ_REQUIRE(capacity_hint >= 0, "pfz_cossim_join_dev: capacity_hint %lld < 0", (long long)capacity_hint);
    PFZ_TRY(sparse_join_operands("pfz_cossim_join_dev", to_index, from_matrix, min_similarity, self_join != 0));
    return sparse_join_dev_run(ctx, to_index, from_matrix, self_join != 0, min_similarity, capacity_hint, out, out_counters);
}

void pfz_pairs_free(pfz_pairs *pairs) { pairs_handle_free(pairs); }

int pfz_pairs_count(const pfz_pairs *pairs, int64_t *out_count)
{
    PFZ_REQUIRE(pairs && out_count, "pfz_pairs_count: NULL argument");
    *out_count = pairs->count;
    return PFZ_OK;
}

int pfz_pairs_shape(const pfz_pairs *pairs, int64_t *out_n_from, int64_t *out_n_to, int32_t *out_self_join)
{
    PFZ_REQUIRE(pairs, "pfz_pairs_shape: NULL argument");
    if (out_n_from) *out_n_from = pairs->n_from;
    if (out_n_to) *out_n_to = pairs->n_to;
    if (out_self_join) *out_self_join = pairs->self ? 1 : 0;
    return PFZ_OK;
}

int pfz_pairs_download(pfz_ctx *ctx, const pfz_pairs *pairs, int64_t *out_row_ptr, int32_t *out_idx, float *out_sim)
{
    PFZ_REQUIRE(ctx && pairs && out_row_ptr, "pfz_pairs_download: NULL argument");
    PFZ_REQUIRE(pairs->ctx == ctx, "pfz_pairs_download: the pair list belongs to another context");
    PFZ_REQUIRE(pairs->count == 0 || (out_idx && out_sim), "pfz_pairs_download: NULL output for %lld pairs", (long long)pairs->count);
    if (pairs->count == 0) {
        for (int64_t r = 0; r <= pairs->n_from; ++r) out_row_ptr[r] = 0;
        return PFZ_OK;
    }
    PFZ_HIP(hipSetDevice(ctx->device));
    DevBuf d_ptr, d_idx;
    PFZ_TRY(join_unpack(ctx, pairs->keys, pairs->count, pairs->n_from, &d_ptr, &d_idx));
    return join_download(ctx, d_ptr, d_idx, pairs->vals, pairs->count, pairs->n_from, out_row_ptr, out_idx, out_sim);
}

int pfz_cossim_components(pfz_ctx *ctx, const pfz_index *index, const pfz_csr *matrix, double min_similarity, int32_t *out_label,
                          int64_t *out_pairs, int64_t *out_components, int64_t *out_counters)
{
    PFZ_REQUIRE(ctx && index && matrix, "pfz_cossim_components: NULL argument");
    PFZ_REQUIRE(out_pairs && out_components, "pfz_cossim_components: NULL out_pairs / out_components");
    PFZ_REQUIRE(matrix->n_rows == 0 || out_label, "pfz_cossim_components: NULL out_label");
    PFZ_TRY(sparse_join_operands("pfz_cossim_components", index, matrix, min_similarity, true));
    return sparse_comp_run(ctx, index, matrix, min_similarity, out_label, out_pairs, out_components, out_counters);
}

}  // extern "C"
