// K23 -- the threshold forms of the 1-bit tile program: every pair of packed binary codes within a Hamming distance
// (pfz_hamming_join, what Hamming.join runs), and the connected components of that relation over one list
// (pfz_hamming_components).  K14 asks the same two questions of the fp32 cosine; here the score is an exact function of one
// integer, the number h of differing bits, so the comparison is h <= hmax on the counts the tile program already holds: no
// division, no score panel, no block maxima, no margin and no rescoring, and the answer is exact by construction.
//
// Mapping to CDNA4: k5_hamming_panel's main loop as it is -- k5_hamming_loop of k5_core.h, 128 x 128 workgroup tiles on the
// vector ALU (v_xor_b32 / v_bcnt_u32_b32), both row sets in 36 864 B of LDS, thread (tx, ty) with 16 x 4 counts -- with another
// end (k23_tile_end of k23_core.h): each lane's hits as a 64-bit mask, a wave (32 rows x 128 columns) without a hit leaves
// without touching memory, otherwise one atomic per wave reserves the room and the hits are appended (key = row << 32 | col, h
// beside it) or united in K12's forest.  The panel's 32 floats of epilogue and its 64 KiB of stores per tile are gone.
// Workgroup -> tile, the self-join's upper triangle, the launches, the capacity protocol, the sort into CSR order and the
// counters are K14's (k14_core.h, join_sort_unpack): a self-join runs T (T + 1) / 2 of the T^2 tiles.
#include "k23_core.h"

namespace pfz {

template <DenseSink kSink>
__device__ __forceinline__ void k23_body(const DenseJoinArgs &P)
{
    const int tid = threadIdx.x, lane = tid & 63, tx = tid & 31, ty = tid >> 5;
    int tm, tn;
    if (!k14_tile<8, 8>(P, &tm, &tn)) return;
    if (tid == 0) atomicAdd(P.state + kK23Tiles, 1ull);
    const int64_t row0 = (int64_t)tm * kTile, col0 = (int64_t)tn * kTile;

    int h[16][4];
#pragma unroll
    for (int i = 0; i < 16; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) h[i][j] = 0;

    k5_hamming_loop(P.A, P.B, row0, col0, P.n_a, P.n_b, P.d, tid, tx, ty, h);

    k23_tile_end<kSink>(h, row0, col0, tx, ty, P, lane);
}

__global__ __launch_bounds__(256, 2) void k23_join_kernel(DenseJoinArgs P) { k23_body<kSinkJoin>(P); }

// (a self-join always: the components of ONE list)
__global__ __launch_bounds__(256, 2) void k23_comp_kernel(DenseJoinArgs P) { k23_body<kSinkUnite>(P); }

static int hamming_join_operand(const char *who, const char *side, const pfz_dense *m)
{
    PFZ_REQUIRE(m->dtype == PFZ_DENSE_B1, "%s: the %s are %s; the Hamming threshold kernels take binary operands only (pfz_dense_upload1)", who,
                side, dense_dtype_name(m->dtype));
    if (m->n >= ((int64_t)1 << 31)) {
        set_error("%s: %lld rows exceed the 32-bit positions", who, (long long)m->n);
        return PFZ_ERR_UNSUPPORTED;
    }
    return PFZ_OK;
}

static int hamming_join_args(const char *who, const pfz_dense *F, const pfz_dense *T, bool self, int64_t hmax, DenseJoinArgs *P, int64_t *grid)
{
    P->A = F->x;
    P->B = T->x;
    P->n_a = F->n;
    P->n_b = T->n;
    P->d = F->ld / 8;      // bytes a row: whole 16-byte pieces (pfz_dense_upload1)
    P->self = self ? 1 : 0;
    P->hmax = (int32_t)hmax;
    return dense_join_grid(who, P, kTile, 8, 8, grid);
}

int hamming_join_run(pfz_ctx *ctx, const pfz_dense *F, const pfz_dense *T, bool self, int64_t hmax, int64_t capacity,
                     int64_t *out_row_ptr, int32_t *out_idx, int32_t *out_dist, int64_t *out_total, int64_t *out_counters)
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
    int64_t grid;
    PFZ_TRY(hamming_join_args("pfz_hamming_join", F, T, self, hmax, &P, &grid));
    P.capacity = (unsigned long long)capacity;

    DevBuf d_keys, d_vals, d_state;
    PFZ_TRY(d_keys.alloc(ctx, (size_t)capacity * sizeof(uint64_t)));
    PFZ_TRY(d_vals.alloc(ctx, (size_t)capacity * sizeof(int32_t)));
    PFZ_TRY(d_state.alloc(ctx, kK23Words * sizeof(unsigned long long)));
    PFZ_HIP(hipMemsetAsync(d_state.p, 0, kK23Words * sizeof(unsigned long long), ctx->stream));
    P.keys = d_keys.as<uint64_t>();
    P.vals = d_vals.as<float>();
    P.state = d_state.as<unsigned long long>();
    unsigned long long state[kK23Words];
    {
        ProfScope ps(ctx, "k23_join");
        PFZ_TRY(k14_launch(ctx, k23_join_kernel, P, grid, 256, 8 * 64));
        PFZ_TRY(copy_d2h(ctx, state, d_state.p, sizeof(state)));      // (waits for the kernel)
    }
    const int64_t total = (int64_t)state[kK23Hits];
    *out_total = total;
    if (out_counters) {
        out_counters[0] = (int64_t)state[kK23Tiles];
        out_counters[1] = (int64_t)state[kK23HitWaves];
    }
    if (total > capacity) return PFZ_OK;       // the caller's buffers stay as they are: it repeats the call with room for `total`
    // (the 32-bit payload beside a key is the distance here: join_sort_unpack moves its bits, whatever they mean)
    return join_sort_unpack(ctx, "k23_sort_unpack", d_keys.as<uint64_t>(), d_vals.as<uint32_t>(), total, n_from, out_row_ptr, out_idx,
                            reinterpret_cast<float *>(out_dist));
}

int hamming_comp_run(pfz_ctx *ctx, const pfz_dense *V, int64_t hmax, int32_t *out_label, int64_t *out_pairs, int64_t *out_components,
                     int64_t *out_counters)
{
    PFZ_HIP(hipSetDevice(ctx->device));
    *out_pairs = *out_components = 0;
    if (out_counters) out_counters[0] = out_counters[1] = 0;
    const int64_t n = V->n;
    if (n == 0) return PFZ_OK;
    DenseJoinArgs P = {};
    int64_t grid;
    PFZ_TRY(hamming_join_args("pfz_hamming_components", V, V, true, hmax, &P, &grid));

    ForestRun forest;
    DevBuf d_state;
    PFZ_TRY(forest.alloc(ctx, n));
    PFZ_TRY(d_state.alloc(ctx, kK23Words * sizeof(unsigned long long)));      // the hits, the two counters, the roots: a line each
    PFZ_HIP(hipMemsetAsync(d_state.p, 0, kK23Words * sizeof(unsigned long long), ctx->stream));
    P.parent = forest.parent.as<int32_t>();
    P.state = d_state.as<unsigned long long>();
    {
        ProfScope ps(ctx, "k23_components");
        PFZ_TRY(forest.begin(ctx));
        PFZ_TRY(k14_launch(ctx, k23_comp_kernel, P, grid, 256, 8 * 64));
        PFZ_TRY(forest.flatten(ctx, P.state + kK23Roots));
    }
    unsigned long long state[kK23Words];
    PFZ_TRY(copy_d2h(ctx, state, d_state.p, sizeof(state)));
    PFZ_TRY(forest.download(ctx, out_label));
    *out_pairs = (int64_t)state[kK23Hits];
    *out_components = (int64_t)state[kK23Roots];
    if (out_counters) {
        out_counters[0] = (int64_t)state[kK23Tiles];
        out_counters[1] = (int64_t)state[kK23HitWaves];
    }
    return PFZ_OK;
}

}  // namespace pfz

using namespace pfz;

extern "C" {

int pfz_hamming_join(pfz_ctx *ctx, const pfz_dense *from, const pfz_dense *to, int64_t max_distance, int64_t capacity,
                     int64_t *out_row_ptr, int32_t *out_idx, int32_t *out_dist, int64_t *out_total, int64_t *out_counters)
{
    PFZ_REQUIRE(ctx && from, "pfz_hamming_join: NULL argument");
    PFZ_REQUIRE(capacity >= 0, "pfz_hamming_join: capacity %lld < 0", (long long)capacity);
    PFZ_REQUIRE(out_row_ptr && out_total, "pfz_hamming_join: NULL out_row_ptr / out_total");
    PFZ_REQUIRE(capacity == 0 || (out_idx && out_dist), "pfz_hamming_join: NULL output with capacity %lld", (long long)capacity);
    const bool self = to == nullptr || to == from;
    const pfz_dense *T = self ? from : to;
    PFZ_TRY(hamming_join_operand("pfz_hamming_join", "from-codes", from));
    PFZ_TRY(hamming_join_operand("pfz_hamming_join", "to-codes", T));
    PFZ_REQUIRE(from->dim == T->dim, "pfz_hamming_join: from-codes have %lld bits, to-codes %lld", (long long)from->dim, (long long)T->dim);
    PFZ_REQUIRE(max_distance >= 0 && max_distance <= from->dim, "pfz_hamming_join: max_distance %lld is outside [0, %lld]",
                (long long)max_distance, (long long)from->dim);
    return hamming_join_run(ctx, from, T, self, max_distance, capacity, out_row_ptr, out_idx, out_dist, out_total, out_counters);
}

int pfz_hamming_components(pfz_ctx *ctx, const pfz_dense *codes, int64_t max_distance, int32_t *out_label, int64_t *out_pairs,
                           int64_t *out_components, int64_t *out_counters)
{
    PFZ_REQUIRE(ctx && codes, "pfz_hamming_components: NULL argument");
    PFZ_REQUIRE(out_pairs && out_components, "pfz_hamming_components: NULL out_pairs / out_components");
    PFZ_REQUIRE(codes->n == 0 || out_label, "pfz_hamming_components: NULL out_label");
    PFZ_TRY(hamming_join_operand("pfz_hamming_components", "codes", codes));
    PFZ_REQUIRE(max_distance >= 0 && max_distance <= codes->dim, "pfz_hamming_components: max_distance %lld is outside [0, %lld]",
                (long long)max_distance, (long long)codes->dim);
    return hamming_comp_run(ctx, codes, max_distance, out_label, out_pairs, out_components, out_counters);
}

int pfz_hamming_max_distance(int64_t dim_bits, double min_similarity, int64_t *out_max_distance)
{
    PFZ_REQUIRE(out_max_distance, "pfz_hamming_max_distance: NULL out_max_distance");
    PFZ_REQUIRE(dim_bits >= 1 && dim_bits < ((int64_t)1 << 24), "pfz_hamming_max_distance: %lld bits are outside [1, 2^24)", (long long)dim_bits);
    PFZ_REQUIRE(!std::isnan(min_similarity) && min_similarity >= 0.0 && min_similarity <= 1.0,
                "pfz_hamming_max_distance: min_similarity %g is not a number in [0, 1]", min_similarity);
    *out_max_distance = hamming_cutoff(dim_bits, min_similarity);
    return PFZ_OK;
}

}  // extern "C"
