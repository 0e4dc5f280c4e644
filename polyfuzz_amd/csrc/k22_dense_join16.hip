// K22 -- K14's two questions (every pair of embedding rows whose cosine is >= t; the connected components of that relation)
// answered on the 16-bit matrix cores: a search on float16 / bfloat16 copies of the vectors finds candidates, and the fp32 vectors
// decide.  pfz_dense_join16 and pfz_dense_components16; what Embeddings.join / .components run with search_dtype set.
//
// A threshold makes the two stages exact, which a top-n does not: rounding a unit vector to 16 bits moves its cosine with anything
// by at most eps (dense_search_margin below), so every pair whose exact score is >= t has a 16-bit score >= t - eps, and scoring
// those candidates exactly returns the pairs at or above t -- there is no multiplier to guess.
//
// Stage 1, k22_search_kernel<f16 | bf16>: K5's 16-bit tile program (k5_tile_loop16 of k5_core.h: 256 x 256 workgroup tiles, 8 waves
// of 128 x 64 on v_mfma_f32_32x32x16_{f16,bf16}) with K14's end (dense_corner_end of k14_core.h), called for the wave's two 64 x 64
// corners: score = acc * inv_a[row] * inv_b[col], the float32 k5_gemm16_panel would store; candidate iff score >= ts32, the
// largest float32 <= t - eps; one atomic per half corner that has one; the key row << 32 | col goes out, no score; candidates
// beyond the buffer are counted, never written.  Two lists: the panel's blocks of 8 x 4 tiles per XCD.  One list: only the tiles on
// or above the diagonal, in square blocks of 8 x 8 over the upper triangle (k14_tile, as K14 deals them).
// Stage 2, k22_rescore_kernel: a wave takes 64 candidate keys at a time and scores each pair on the fp32 rows with k5_pair_score
// (float64 sum in one fixed order, rounded once: k5_rescore_topn's score, symmetric in its two rows); hit iff s >= t32, K14's
// threshold.  Join: ONE atomic per batch reserves the places of its hits, key and score go out into the caller-capacity buffers,
// and K14's join_sort_unpack makes the CSR.  Components: each hit lane unites its two positions in K12's forest; nothing is stored.
// The candidate buffer is the library's: when stage 1 counts more candidates than it holds, a buffer of the exact count is made
// and stage 1 runs once more -- two runs at most.  Device memory beyond the operands is O(candidates) for both entries.
//
// from32 == NULL: the plain 16-bit join -- margin 0, stage 1 keeps its scores beside the keys (the 16-bit panel's float32, bit for
// bit), no stage 2; for a corpus that exists only in 16 bits.
#include "k14_core.h"

namespace pfz {

// The edge, in tiles, of a self-join's square block: the tiles one XCD works on together.  Measured at 100 000 x 768 (DESIGN.md
// section 4, K22): edges 4, 6 and 8 give the same self-join and components times within the spread of five rounds, so the edge is
// K14's.
constexpr int kSelfEdge = 8;

template <typename T>
__global__ __launch_bounds__(512, 1) void k22_search_kernel(DenseJoinArgs P)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int tm, tn;
    if (!(P.self ? k14_tile<kSelfEdge, kSelfEdge>(P, &tm, &tn) : k14_tile<8, 4>(P, &tm, &tn))) return;
    if (tid == 0) atomicAdd(P.state + 1, 1ull);
    const int64_t row0 = (int64_t)tm * kTile16, col0 = (int64_t)tn * kTile16;
    // a wave owns 128 x 64 of the tile: rows 128 vr .., columns 128 vc + wn .., as two 64 x 64 corners
    const int vr = wave >> 2, vc = (wave >> 1) & 1, wn = (wave & 1) * 64;

    typename T::acc_t acc[2][2][2];           // [half][i][j]
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[h][i][j][r] = 0;

    k5_tile_loop16<T>(P.A, P.B, row0, col0, P.n_a, P.n_b, P.d, tid, lane, vr, vc, wn, acc);

#pragma unroll
    for (int h = 0; h < 2; ++h)
        dense_corner_end<kSinkKeys>(acc[h], row0 + vr * 128 + h * 64 + 4 * (lane >> 5), col0 + vc * 128 + wn + (lane & 31), P, lane);
}

struct RescoreArgs {
    const uint64_t *cand;              // [n_cand] row << 32 | col, distinct, in any order
    int64_t n_cand;
    const float *A, *B;                // [n_a][ld], [n_b][ld] float32 (a self-join: the same matrix)
    const float *inv_a, *inv_b;
    int64_t ld;                        // a multiple of 32
    float t32;
    unsigned long long *hits;
    uint64_t *keys;                    // join: [capacity], and the scores beside them
    float *vals;
    unsigned long long capacity;
    int32_t *parent;                   // components: the forest
};

template <bool kComp>
__global__ __launch_bounds__(256) void k22_rescore_kernel(RescoreArgs R)
{
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * 4 * 64;
    for (int64_t b0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; b0 < R.n_cand; b0 += stride) {
        const int cnt = (int)min((int64_t)64, R.n_cand - b0);
        const uint64_t key = lane < cnt ? R.cand[b0 + lane] : 0ull;
        float mine = 0.f;
        for (int c = 0; c < cnt; ++c) {      // the wave scores the batch's pairs one after another; lane c keeps pair c's score
            const int64_t row = (int64_t)(uint32_t)__builtin_amdgcn_readlane((int)(key >> 32), c);
            const int64_t col = (int64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)key, c);
            const float s = k5_pair_score(R.A + row * R.ld, R.B + col * R.ld, R.ld, (double)R.inv_a[row], (double)R.inv_b[col], lane);
            if (lane == c) mine = s;
        }
        const bool hit = lane < cnt && mine >= R.t32;
        const uint64_t m = __ballot(hit);
        if (m == 0ull) continue;
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(R.hits, (unsigned long long)__popcll(m));      // ONE atomic per batch
        if (kComp) {
            if (hit) uf_unite<UfDeviceOps>(R.parent, (int32_t)(key >> 32), (int32_t)(uint32_t)key);
            continue;
        }
        base = __shfl(base, 0, 64);
        const unsigned long long pos = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
        if (hit && pos < R.capacity) {
            R.keys[pos] = key;
            R.vals[pos] = mine;
        }
    }
}

// eps of the header: how far the float32 score of the search copies may lie below the exact cosine
static double search_margin(int32_t dtype, int64_t ld)
{
    const double u = dtype == PFZ_DENSE_BF16 ? 0x1p-8 : 0x1p-11;
    return 2.0 * asin(u + 0x1p-24 + sqrt((double)ld) * 0x1p-25) + (double)(ld + 8) * 0x1p-23;
}

// the largest float32 <= t - eps
static float search_threshold32(double t, double eps)
{
    const double d = t - eps;
    float f = (float)d;
    if ((double)f > d) f = nextafterf(f, -INFINITY);
    return f;
}

static int search16_operand(const char *who, const char *side, const pfz_dense *m)
{
    PFZ_REQUIRE(m->dtype == PFZ_DENSE_F16 || m->dtype == PFZ_DENSE_BF16, "%s: the %s are %s; the 16-bit search takes float16 / bfloat16 "
                "operands (pfz_dense_derive16, pfz_dense_upload16)", who, side, dense_dtype_name(m->dtype));
    PFZ_REQUIRE(m->normalize, "%s: the %s were uploaded without normalize: a threshold in [0, 1] means a cosine", who, side);
    if (m->n >= ((int64_t)1 << 31)) {
        set_error("%s: %lld rows exceed the 32-bit positions", who, (long long)m->n);
        return PFZ_ERR_UNSUPPORTED;
    }
    return PFZ_OK;
}

static int exact_operand(const char *who, const char *side, const pfz_dense *m16, const pfz_dense *m32)
{
    PFZ_REQUIRE(m32->dtype == PFZ_DENSE_F32 && m32->normalize, "%s: the exact %s are %s, uploaded with normalize = %d; the candidates are "
                "scored on fp32 vectors uploaded with normalize = 1 (pfz_dense_upload)", who, side, dense_dtype_name(m32->dtype), m32->normalize);
    PFZ_REQUIRE(m16->n == m32->n && m16->dim == m32->dim, "%s: the 16-bit %s are %lld x %lld, the exact ones %lld x %lld", who, side,
                (long long)m16->n, (long long)m16->dim, (long long)m32->n, (long long)m32->dim);
    return PFZ_OK;
}

// Stage 1 over the 16-bit operands into `keys` (and `vals`, or NULL) of `capacity`; state: device [3], zeroed by the caller.
static int search_launch(pfz_ctx *ctx, const char *who, const pfz_dense *F, const pfz_dense *T, bool self, float t32, uint64_t *keys,
                         float *vals, int64_t capacity, unsigned long long *d_state)
{
    DenseJoinArgs P = {};
    P.A = F->x;
    P.B = T->x;
    P.inv_a = F->inv;
    P.inv_b = T->inv;
    P.n_a = F->n;
    P.n_b = T->n;
    P.d = F->ld;
    P.self = self ? 1 : 0;
    P.t32 = t32;
    P.capacity = (unsigned long long)capacity;
    P.keys = keys;
    P.vals = vals;
    P.state = d_state;
    const int bm = self ? kSelfEdge : 8, bn = self ? kSelfEdge : 4;
    int64_t grid;
    PFZ_TRY(dense_join_grid(who, &P, kTile16, bm, bn, &grid));
    return k14_launch(ctx, F->dtype == PFZ_DENSE_F16 ? k22_search_kernel<f16> : k22_search_kernel<bf16>, P, grid, 512, 8 * bm * bn);
}

// Stage 1 into a candidate buffer of the library's: `cand_capacity` keys (0: a guess, four per from-row), and when the exact count
// exceeds it a buffer of that count and a second run.  counters [0], [1] add up over the runs, [2] is the number of candidates.
static int search_candidates(pfz_ctx *ctx, const char *who, const pfz_dense *F, const pfz_dense *T, bool self, float ts32,
                             int64_t cand_capacity, DevBuf *d_cand, int64_t *n_cand, int64_t *counters)
{
    int64_t cap = cand_capacity > 0 ? cand_capacity : std::max<int64_t>(4096, 4 * F->n);
    DevBuf d_state;
    PFZ_TRY(d_state.alloc(ctx, 3 * sizeof(unsigned long long)));
    counters[0] = counters[1] = counters[2] = 0;
    ProfScope ps(ctx, "k22_search");
    for (int run = 0; run < 2; ++run) {
        PFZ_TRY(d_cand->alloc(ctx, (size_t)cap * sizeof(uint64_t)));
        PFZ_HIP(hipMemsetAsync(d_state.p, 0, 3 * sizeof(unsigned long long), ctx->stream));
        PFZ_TRY(search_launch(ctx, who, F, T, self, ts32, d_cand->as<uint64_t>(), nullptr, cap, d_state.as<unsigned long long>()));
        unsigned long long state[3];
        PFZ_TRY(copy_d2h(ctx, state, d_state.p, sizeof(state)));      // (waits for the kernel)
        counters[0] += (int64_t)state[1];
        counters[1] += (int64_t)state[2];
        counters[2] = (int64_t)state[0];
        if ((int64_t)state[0] <= cap || run == 1) break;      // (the same search counts the same candidates: the second run had room)
        cap = (int64_t)state[0];
    }
    *n_cand = std::min(counters[2], cap);
    return PFZ_OK;
}

static int rescore_launch(pfz_ctx *ctx, bool comp, RescoreArgs R)
{
    if (R.n_cand == 0) return PFZ_OK;
    const int64_t blocks = std::min<int64_t>((R.n_cand + 255) / 256, 8192);
    hipLaunchKernelGGL(comp ? k22_rescore_kernel<true> : k22_rescore_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, R);
    PFZ_HIP(hipGetLastError());
    return PFZ_OK;
}

static RescoreArgs rescore_args(const DevBuf &d_cand, int64_t n_cand, const pfz_dense *F, const pfz_dense *T, double t)
{
    RescoreArgs R = {};
    R.cand = d_cand.as<uint64_t>();
    R.n_cand = n_cand;
    R.A = (const float *)F->x;
    R.B = (const float *)T->x;
    R.inv_a = F->inv;
    R.inv_b = T->inv;
    R.ld = F->ld;
    R.t32 = threshold32(t);
    return R;
}

static int join16_run(pfz_ctx *ctx, const pfz_dense *F16, const pfz_dense *T16, const pfz_dense *F32, const pfz_dense *T32, bool self,
                      double t, int64_t capacity, int64_t cand_capacity, int64_t *out_row_ptr, int32_t *out_idx, float *out_sim,
                      int64_t *out_total, int64_t *out_counters)
{
    PFZ_HIP(hipSetDevice(ctx->device));
    *out_total = 0;
    int64_t counters[3] = {0, 0, 0};
    if (out_counters) out_counters[0] = out_counters[1] = out_counters[2] = 0;
    const int64_t n_from = F16->n;
    if (n_from == 0 || T16->n == 0) {
        for (int64_t r = 0; r <= n_from; ++r) out_row_ptr[r] = 0;
        return PFZ_OK;
    }
    DevBuf d_keys, d_vals, d_state;
    PFZ_TRY(d_keys.alloc(ctx, (size_t)capacity * sizeof(uint64_t)));
    PFZ_TRY(d_vals.alloc(ctx, (size_t)capacity * sizeof(float)));
    PFZ_TRY(d_state.alloc(ctx, 3 * sizeof(unsigned long long)));
    PFZ_HIP(hipMemsetAsync(d_state.p, 0, 3 * sizeof(unsigned long long), ctx->stream));
    int64_t total;
    if (!F32) {
        // the plain 16-bit join: stage 1 is the whole call, its hits go straight into the caller-capacity buffers with their scores
        unsigned long long state[3];
        {
            ProfScope ps(ctx, "k22_search");
            PFZ_TRY(search_launch(ctx, "pfz_dense_join16", F16, T16, self, threshold32(t), d_keys.as<uint64_t>(), d_vals.as<float>(), capacity,
                                  d_state.as<unsigned long long>()));
            PFZ_TRY(copy_d2h(ctx, state, d_state.p, sizeof(state)));      // (waits for the kernel)
        }
        total = (int64_t)state[0];
        counters[0] = (int64_t)state[1];
        counters[1] = (int64_t)state[2];
        counters[2] = total;
    }
    else {
        DevBuf d_cand;
        int64_t n_cand;
        PFZ_TRY(search_candidates(ctx, "pfz_dense_join16", F16, T16, self, search_threshold32(t, search_margin(F16->dtype, F16->ld)),
                                  cand_capacity, &d_cand, &n_cand, counters));
        RescoreArgs R = rescore_args(d_cand, n_cand, F32, T32, t);
        R.hits = d_state.as<unsigned long long>();
        R.keys = d_keys.as<uint64_t>();
        R.vals = d_vals.as<float>();
        R.capacity = (unsigned long long)capacity;
        unsigned long long hits;
        {
            ProfScope ps(ctx, "k22_rescore");
            PFZ_TRY(rescore_launch(ctx, false, R));
            PFZ_TRY(copy_d2h(ctx, &hits, d_state.p, sizeof(hits)));      // (waits for the kernel)
        }
        total = (int64_t)hits;
    }
    *out_total = total;
    if (out_counters) std::copy(counters, counters + 3, out_counters);
    if (total > capacity) return PFZ_OK;       // the caller's buffers stay as they are: it repeats the call with room for `total`
    return join_sort_unpack(ctx, "k22_sort_unpack", d_keys.as<uint64_t>(), d_vals.as<uint32_t>(), total, n_from, out_row_ptr, out_idx,
                            out_sim);
}

static int comp16_run(pfz_ctx *ctx, const pfz_dense *V16, const pfz_dense *V32, double t, int64_t cand_capacity, int32_t *out_label,
                      int64_t *out_pairs, int64_t *out_components, int64_t *out_counters)
{
    PFZ_HIP(hipSetDevice(ctx->device));
    *out_pairs = *out_components = 0;
    int64_t counters[3] = {0, 0, 0};
    if (out_counters) out_counters[0] = out_counters[1] = out_counters[2] = 0;
    const int64_t n = V16->n;
    if (n == 0) return PFZ_OK;
    DevBuf d_cand, d_state;
    int64_t n_cand;
    PFZ_TRY(search_candidates(ctx, "pfz_dense_components16", V16, V16, true, search_threshold32(t, search_margin(V16->dtype, V16->ld)),
                              cand_capacity, &d_cand, &n_cand, counters));
    ForestRun forest;
    PFZ_TRY(forest.alloc(ctx, n));
    PFZ_TRY(d_state.alloc(ctx, 2 * sizeof(unsigned long long)));      // the hits, the roots
    PFZ_HIP(hipMemsetAsync(d_state.p, 0, 2 * sizeof(unsigned long long), ctx->stream));
    RescoreArgs R = rescore_args(d_cand, n_cand, V32, V32, t);
    R.hits = d_state.as<unsigned long long>();
    R.parent = forest.parent.as<int32_t>();
    {
        ProfScope ps(ctx, "k22_rescore");
        PFZ_TRY(forest.begin(ctx));
        PFZ_TRY(rescore_launch(ctx, true, R));
        PFZ_TRY(forest.flatten(ctx, R.hits + 1));
    }
    unsigned long long state[2];
    PFZ_TRY(copy_d2h(ctx, state, d_state.p, sizeof(state)));
    PFZ_TRY(forest.download(ctx, out_label));
    *out_pairs = (int64_t)state[0];
    *out_components = (int64_t)state[1];
    if (out_counters) std::copy(counters, counters + 3, out_counters);
    return PFZ_OK;
}

}  // namespace pfz

using namespace pfz;

extern "C" {

int pfz_dense_search_margin(int32_t dtype, int64_t ld, double *out_eps)
{
    PFZ_REQUIRE(out_eps, "pfz_dense_search_margin: NULL out_eps");
    PFZ_REQUIRE(dtype == PFZ_DENSE_F16 || dtype == PFZ_DENSE_BF16,
                "pfz_dense_search_margin: dtype %d is neither PFZ_DENSE_F16 nor PFZ_DENSE_BF16", dtype);
    PFZ_REQUIRE(ld >= 1, "pfz_dense_search_margin: ld %lld < 1", (long long)ld);
    *out_eps = search_margin(dtype, ld);
    return PFZ_OK;
}

int pfz_dense_join16(pfz_ctx *ctx, const pfz_dense *from16, const pfz_dense *to16, const pfz_dense *from32, const pfz_dense *to32,
                     double min_similarity, int64_t capacity, int64_t cand_capacity, int64_t *out_row_ptr, int32_t *out_idx,
                     float *out_sim, int64_t *out_total, int64_t *out_counters)
{
    PFZ_REQUIRE(ctx && from16, "pfz_dense_join16: NULL argument");
    PFZ_REQUIRE(!std::isnan(min_similarity) && min_similarity >= 0.0 && min_similarity <= 1.0,
                "pfz_dense_join16: min_similarity %g is not a number in [0, 1]", min_similarity);
    PFZ_REQUIRE(capacity >= 0, "pfz_dense_join16: capacity %lld < 0", (long long)capacity);
    PFZ_REQUIRE(cand_capacity >= 0, "pfz_dense_join16: cand_capacity %lld < 0", (long long)cand_capacity);
    PFZ_REQUIRE(out_row_ptr && out_total, "pfz_dense_join16: NULL out_row_ptr / out_total");
    PFZ_REQUIRE(capacity == 0 || (out_idx && out_sim), "pfz_dense_join16: NULL output with capacity %lld", (long long)capacity);
    const bool self = to16 == nullptr || to16 == from16;
    const pfz_dense *T16 = self ? from16 : to16;
    PFZ_TRY(search16_operand("pfz_dense_join16", "from-vectors", from16));
    PFZ_TRY(search16_operand("pfz_dense_join16", "to-vectors", T16));
    PFZ_REQUIRE(from16->dtype == T16->dtype, "pfz_dense_join16: from-vectors are %s, to-vectors %s: derive both with one type",
                dense_dtype_name(from16->dtype), dense_dtype_name(T16->dtype));
    PFZ_REQUIRE(from16->dim == T16->dim, "pfz_dense_join16: from-vectors have %lld columns, to-vectors %lld", (long long)from16->dim,
                (long long)T16->dim);
    const pfz_dense *T32 = nullptr;
    if (from32) {
        PFZ_REQUIRE(self ? (to32 == nullptr || to32 == from32) : to32 != nullptr,
                    "pfz_dense_join16: the exact to-vectors do not go with the 16-bit ones (a self-join has one exact handle, two lists "
                    "need the to-side's)");
        T32 = self ? from32 : to32;
        PFZ_TRY(exact_operand("pfz_dense_join16", "from-vectors", from16, from32));
        PFZ_TRY(exact_operand("pfz_dense_join16", "to-vectors", T16, T32));
    }
    else
        PFZ_REQUIRE(to32 == nullptr, "pfz_dense_join16: exact to-vectors without exact from-vectors");
    return join16_run(ctx, from16, T16, from32, T32, self, min_similarity, capacity, cand_capacity, out_row_ptr, out_idx, out_sim, out_total,
                      out_counters);
}

int pfz_dense_components16(pfz_ctx *ctx, const pfz_dense *v16, const pfz_dense *v32, double min_similarity, int64_t cand_capacity,
                           int32_t *out_label, int64_t *out_pairs, int64_t *out_components, int64_t *out_counters)
{
    PFZ_REQUIRE(ctx && v16 && v32, "pfz_dense_components16: NULL argument");
    PFZ_REQUIRE(!std::isnan(min_similarity) && min_similarity >= 0.0 && min_similarity <= 1.0,
                "pfz_dense_components16: min_similarity %g is not a number in [0, 1]", min_similarity);
    PFZ_REQUIRE(cand_capacity >= 0, "pfz_dense_components16: cand_capacity %lld < 0", (long long)cand_capacity);
    PFZ_REQUIRE(out_pairs && out_components, "pfz_dense_components16: NULL out_pairs / out_components");
    PFZ_REQUIRE(v16->n == 0 || out_label, "pfz_dense_components16: NULL out_label");
    PFZ_TRY(search16_operand("pfz_dense_components16", "vectors", v16));
    PFZ_TRY(exact_operand("pfz_dense_components16", "vectors", v16, v32));
    return comp16_run(ctx, v16, v32, min_similarity, cand_capacity, out_label, out_pairs, out_components, out_counters);
}

}  // extern "C"
