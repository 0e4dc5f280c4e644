// K14 -- the threshold forms of K5 for fp32 operands: every pair of embedding rows whose cosine is >= t (pfz_dense_join, what
// Embeddings.join runs), and the connected components of that relation over one list (pfz_dense_components).  K11 / K12 ask the
// same two questions of an edit distance; here the score is the dense cosine and the work is a GEMM.
//
// Mapping to CDNA4: K5's fp32 tile program as it is -- k5_tile_loop of k5_core.h, 128 x 128 workgroup tiles, 4 waves of 2 x 2
// v_mfma_f32_32x32x2_f32, operands double-buffered in LDS -- with another end.  k5_gemm_panel_pipe stores its tile of the score
// panel and a second kernel reads the panel back to find the few scores that matter; with a threshold nearly every tile holds
// none, so here the comparison is made on the accumulators in registers:
//   score(row, col) = acc * inv_a[row] * inv_b[col], in that order: the float32 the panel would hold, bit for bit;
//   hit iff score >= t32, the smallest float32 >= the caller's float64 threshold: (double)score >= t, made exact in float32;
//   rows and columns beyond the matrices' edges are never hits (their operands are clamped copies of the last row).
// A wave whose 64 x 64 corner has no hit leaves without touching memory.  Otherwise, per half of the corner that has one,
//   join:        the wave's hits are counted, ONE atomic add for all of them reserves their places, and each hit goes out as
//                key = row << 32 | col and its score at the same position of two parallel arrays -- while there is room: hits
//                beyond the caller's capacity are counted, never written (K11's contract).  The keys are distinct; sorted with
//                their scores beside them (sort_u64.hip) they are CSR order, and the order of the appends leaves no trace;
//   components:  each hit lane unites its two positions in K12's forest (k12_core.h, the same agent-scope relaxed atomics) there
//                and then; no key, no capacity.  k12_flatten turns the forest into labels.
// No score panel, no block maxima, no LDS beyond the two operand buffers: device memory beyond the operands is O(hits), or O(n).
//
// Self-join (one list): score(i, j) and score(j, i) are the same pair, so only the tiles on or above the diagonal are launched,
// T (T + 1) / 2 of T^2, and inside a diagonal tile only col > row is a hit.  A pair (i < j) is reported as row i, column j with the
// score the panel holds at [i][j] ([j][i] multiplies the two inverse norms in the other order and may differ in the last bit; it
// is never computed).  (i, i) is never a pair; equal vectors at different positions are.
//
// Workgroup -> tile: as K5, 8 x 8 blocks of tiles dealt round-robin to the 8 XCDs (8 A tiles + 8 B tiles feed 64 tile products out
// of one L2).  Two lists: the blocks column by column.  Self-join: the blocks (bi <= bj) of the upper triangle, numbered
// g = bj (bj + 1) / 2 + bi and decoded in the kernel; of a diagonal block's 64 workgroups the 28 below the diagonal leave at once,
// as do those of tiles beyond the edge.  A deal of 2^24 workgroups or more goes out as several launches (k14_launch).
// The argument block, the deal, the corner's end and the launches are in k14_core.h: K22 (k22_dense_join16.hip) puts the same end
// behind the 16-bit main loop.
#include "k14_core.h"

namespace pfz {

// One workgroup's tile: the fp32 main loop, then the end of the wave's 64 x 64 corner (dense_corner_end of k14_core.h).
template <DenseSink kSink>
__device__ __forceinline__ void k14_body(const DenseJoinArgs &P)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int tm, tn;
    if (!k14_tile<8, 8>(P, &tm, &tn)) return;
    if (tid == 0) atomicAdd(P.state + 1, 1ull);
    const int64_t row0 = (int64_t)tm * kTile, col0 = (int64_t)tn * kTile;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    k5_tile_loop(P.A, P.B, row0, col0, P.n_a, P.n_b, P.d, tid, lane, wm, wn, acc);

    dense_corner_end<kSink>(acc, row0 + wm + 4 * (lane >> 5), col0 + wn + (lane & 31), P, lane);
}

__global__ __launch_bounds__(256, 2) void k14_join_kernel(DenseJoinArgs P) { k14_body<kSinkJoin>(P); }

// (a self-join always: the components of ONE list)
__global__ __launch_bounds__(256, 2) void k14_comp_kernel(DenseJoinArgs P) { k14_body<kSinkUnite>(P); }

// the sorted keys -> CSR: hit p of the row-major order and its share of the row pointers (k11_core.h rows_fill; the scores are
// already in place beside the keys)
__global__ __launch_bounds__(256) void k14_unpack(const uint64_t *__restrict__ keys, int64_t total, int64_t n_from,
                                                   int64_t *__restrict__ row_ptr, int32_t *__restrict__ out_idx)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= total) return;
    out_idx[p] = (int32_t)(uint32_t)keys[p];
    rows_fill(p > 0 ? (int64_t)(keys[p - 1] >> 32) : -1, (int64_t)(keys[p] >> 32), p, total, n_from, row_ptr);
}

// The tail of a threshold join (K14 here, K15 in k15_sparse_join.hip): the `total` appended hits -- distinct keys row << 32 | col,
// the float32 scores' bits beside them -- sorted, unpacked into CSR over n_from rows and downloaded into the caller's three host
// arrays.  total == 0: the row pointers are all zero and nothing else is written.  `scope` times the sort and the unpack.  Blocks.
int join_sort_unpack(pfz_ctx *ctx, const char *scope, const uint64_t *d_keys, const uint32_t *d_vals, int64_t total, int64_t n_from,
                     int64_t *out_row_ptr, int32_t *out_idx, float *out_sim)
{
    if (total == 0) {
        for (int64_t r = 0; r <= n_from; ++r) out_row_ptr[r] = 0;
        return PFZ_OK;
    }
    DevBuf d_skeys, d_svals, d_ptr, d_idx;
    {
        ProfScope ps(ctx, scope);
        const size_t cap = (size_t)sort_codes_capacity(total);
        PFZ_TRY(d_skeys.alloc(ctx, cap * sizeof(uint64_t)));
        PFZ_TRY(d_svals.alloc(ctx, cap * sizeof(uint32_t)));
        PFZ_TRY(sort_pairs_u64(ctx, d_keys, d_vals, d_skeys.as<uint64_t>(), d_svals.as<uint32_t>(), total));
        PFZ_TRY(join_unpack(ctx, d_skeys.as<uint64_t>(), total, n_from, &d_ptr, &d_idx));
    }
    return join_download(ctx, d_ptr, d_idx, d_svals.as<uint32_t>(), total, n_from, out_row_ptr, out_idx, out_sim);
}

int join_unpack(pfz_ctx *ctx, const uint64_t *d_skeys, int64_t total, int64_t n_from, DevBuf *d_ptr, DevBuf *d_idx)
{
    PFZ_TRY(d_ptr->alloc(ctx, (size_t)(n_from + 1) * sizeof(int64_t)));
    PFZ_TRY(d_idx->alloc(ctx, (size_t)total * sizeof(int32_t)));
    hipLaunchKernelGGL(k14_unpack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, d_skeys, total, n_from,
                       d_ptr->as<int64_t>(), d_idx->as<int32_t>());
    PFZ_HIP(hipGetLastError());
    return PFZ_OK;
}

int join_download(pfz_ctx *ctx, const DevBuf &d_ptr, const DevBuf &d_idx, const uint32_t *d_svals, int64_t total, int64_t n_from,
                  int64_t *out_row_ptr, int32_t *out_idx, float *out_sim)
{
    PFZ_TRY(copy_d2h(ctx, out_row_ptr, d_ptr.p, (size_t)(n_from + 1) * sizeof(int64_t)));
    PFZ_TRY(copy_d2h(ctx, out_idx, d_idx.p, (size_t)total * sizeof(int32_t)));
    PFZ_TRY(copy_d2h(ctx, out_sim, d_svals, (size_t)total * sizeof(float)));
    PFZ_HIP(hipStreamSynchronize(ctx->stream));
    return PFZ_OK;
}

static int dense_join_operand(const char *who, const char *side, const pfz_dense *m)
{
    PFZ_REQUIRE(m->dtype == PFZ_DENSE_F32, "%s: the %s are %s; the threshold kernels take fp32 operands only (pfz_dense_upload)", who, side,
                dense_dtype_name(m->dtype));
    PFZ_REQUIRE(m->normalize, "%s: the %s were uploaded without normalize: a threshold in [0, 1] means a cosine", who, side);
    if (m->n >= ((int64_t)1 << 31)) {
        set_error("%s: %lld rows exceed the 32-bit positions", who, (long long)m->n);
        return PFZ_ERR_UNSUPPORTED;
    }
    return PFZ_OK;
}

static int dense_join_run(pfz_ctx *ctx, const pfz_dense *F, const pfz_dense *T, bool self, double t, int64_t capacity,
                          int64_t *out_row_ptr, int32_t *out_idx, float *out_sim, int64_t *out_total, int64_t *out_counters)
{
    PFZ_HIP(hipSetDevice(ctx->device));
    *out_total = 0;
    if (out_counters) out_counters[0] = out_counters[1] = 0;
    const int64_t n_from = F->n, n_to = T->n;
    if (n_from == 0 || n_to == 0) {
        for (int64_t r = 0; r <= n_from; ++r) out_row_ptr[r] = 0;
        return PFZ_OK;
    }
    DenseJoinArgs P = {};
    P.A = F->x;
    P.B = T->x;
    P.inv_a = F->inv;
    P.inv_b = T->inv;
    P.n_a = n_from;
    P.n_b = n_to;
    P.d = F->ld;
    P.self = self ? 1 : 0;
    P.t32 = threshold32(t);
    P.capacity = (unsigned long long)capacity;
    int64_t grid;
    PFZ_TRY(dense_join_grid("pfz_dense_join", &P, kTile, 8, 8, &grid));

    DevBuf d_keys, d_vals, d_state;
    PFZ_TRY(d_keys.alloc(ctx, (size_t)capacity * sizeof(uint64_t)));
    PFZ_TRY(d_vals.alloc(ctx, (size_t)capacity * sizeof(float)));
    PFZ_TRY(d_state.alloc(ctx, 3 * sizeof(unsigned long long)));
    PFZ_HIP(hipMemsetAsync(d_state.p, 0, 3 * sizeof(unsigned long long), ctx->stream));
    P.keys = d_keys.as<uint64_t>();
    P.vals = d_vals.as<float>();
    P.state = d_state.as<unsigned long long>();
    unsigned long long state[3];
    {
        ProfScope ps(ctx, "k14_join");
        PFZ_TRY(k14_launch(ctx, k14_join_kernel, P, grid, 256, 8 * 64));
        PFZ_TRY(copy_d2h(ctx, state, d_state.p, sizeof(state)));      // (waits for the kernel)
    }
    const int64_t total = (int64_t)state[0];
    *out_total = total;
    if (out_counters) {
        out_counters[0] = (int64_t)state[1];
        out_counters[1] = (int64_t)state[2];
    }
    if (total > capacity) return PFZ_OK;       // the caller's buffers stay as they are: it repeats the call with room for `total`
    return join_sort_unpack(ctx, "k14_sort_unpack", d_keys.as<uint64_t>(), d_vals.as<uint32_t>(), total, n_from, out_row_ptr, out_idx,
                            out_sim);
}

static int dense_comp_run(pfz_ctx *ctx, const pfz_dense *V, double t, int32_t *out_label, int64_t *out_pairs, int64_t *out_components,
                          int64_t *out_counters)
{
    PFZ_HIP(hipSetDevice(ctx->device));
    *out_pairs = *out_components = 0;
    if (out_counters) out_counters[0] = out_counters[1] = 0;
    const int64_t n = V->n;
    if (n == 0) return PFZ_OK;
    DenseJoinArgs P = {};
    P.A = P.B = V->x;
    P.inv_a = P.inv_b = V->inv;
    P.n_a = P.n_b = n;
    P.d = V->ld;
    P.self = 1;
    P.t32 = threshold32(t);
    int64_t grid;
    PFZ_TRY(dense_join_grid("pfz_dense_components", &P, kTile, 8, 8, &grid));

    ForestRun forest;
    DevBuf d_state;
    PFZ_TRY(forest.alloc(ctx, n));
    PFZ_TRY(d_state.alloc(ctx, 4 * sizeof(unsigned long long)));      // the hits, the two counters, the roots
    PFZ_HIP(hipMemsetAsync(d_state.p, 0, 4 * sizeof(unsigned long long), ctx->stream));
    P.parent = forest.parent.as<int32_t>();
    P.state = d_state.as<unsigned long long>();
    {
        ProfScope ps(ctx, "k14_components");
        PFZ_TRY(forest.begin(ctx));
        PFZ_TRY(k14_launch(ctx, k14_comp_kernel, P, grid, 256, 8 * 64));
        PFZ_TRY(forest.flatten(ctx, P.state + 3));
    }
    unsigned long long state[4];
    PFZ_TRY(copy_d2h(ctx, state, d_state.p, sizeof(state)));
    PFZ_TRY(forest.download(ctx, out_label));
    *out_pairs = (int64_t)state[0];
    *out_components = (int64_t)state[3];
    if (out_counters) {
        out_counters[0] = (int64_t)state[1];
        out_counters[1] = (int64_t)state[2];
    }
    return PFZ_OK;
}

}  // namespace pfz

using namespace pfz;

extern "C" {

int pfz_dense_join(pfz_ctx *ctx, const pfz_dense *from, const pfz_dense *to, double min_similarity, int64_t capacity,
                   int64_t *out_row_ptr, int32_t *out_idx, float *out_sim, int64_t *out_total, int64_t *out_counters)
{
    PFZ_REQUIRE(ctx && from, "pfz_dense_join: NULL argument");
    PFZ_REQUIRE(!std::isnan(min_similarity) && min_similarity >= 0.0 && min_similarity <= 1.0,
                "pfz_dense_join: min_similarity %g is not a number in [0, 1]", min_similarity);
    PFZ_REQUIRE(capacity >= 0, "pfz_dense_join: capacity %lld < 0", (long long)capacity);
    PFZ_REQUIRE(out_row_ptr && out_total, "pfz_dense_join: NULL out_row_ptr / out_total");
    PFZ_REQUIRE(capacity == 0 || (out_idx && out_sim), "pfz_dense_join: NULL output with capacity %lld", (long long)capacity);
    const bool self = to == nullptr || to == from;
    const pfz_dense *T = self ? from : to;
    PFZ_TRY(dense_join_operand("pfz_dense_join", "from-vectors", from));
    PFZ_TRY(dense_join_operand("pfz_dense_join", "to-vectors", T));
    PFZ_REQUIRE(from->dim == T->dim, "pfz_dense_join: from-vectors have %lld columns, to-vectors %lld", (long long)from->dim,
                (long long)T->dim);
    return dense_join_run(ctx, from, T, self, min_similarity, capacity, out_row_ptr, out_idx, out_sim, out_total, out_counters);
}

int pfz_dense_components(pfz_ctx *ctx, const pfz_dense *vectors, double min_similarity, int32_t *out_label, int64_t *out_pairs,
                         int64_t *out_components, int64_t *out_counters)
{
    PFZ_REQUIRE(ctx && vectors, "pfz_dense_components: NULL argument");
    PFZ_REQUIRE(!std::isnan(min_similarity) && min_similarity >= 0.0 && min_similarity <= 1.0,
                "pfz_dense_components: min_similarity %g is not a number in [0, 1]", min_similarity);
    PFZ_REQUIRE(out_pairs && out_components, "pfz_dense_components: NULL out_pairs / out_components");
    PFZ_REQUIRE(vectors->n == 0 || out_label, "pfz_dense_components: NULL out_label");
    PFZ_TRY(dense_join_operand("pfz_dense_components", "vectors", vectors));
    return dense_comp_run(ctx, vectors, min_similarity, out_label, out_pairs, out_components, out_counters);
}

}  // extern "C"
