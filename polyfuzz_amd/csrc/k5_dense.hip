// K5 -- dense cosine top-n for embedding matrices (fp32 MFMA).
//
// Replaces the dense branches of the reference's cosine_similarity operator
// (polyfuzz/models/_utils.py:74-77,95-102; called with precomputed vectors from
// Embeddings.match, _embeddings.py:127-133): cosine = normalize(A) . normalize(B)^T
// (sklearn.metrics.pairwise.cosine_similarity), then the top-n of every row,
// diagonal excluded for self-match.
//
// Plan:
//   k5_inv_norms<T>     : 1/||row|| of the stored values, for every operand type T (wave per row).
//   k5_gemm_panel_pipe  : S[P x n_to] = A_panel . B^T scaled by both inverse norms (matrices are stored with their
//                         width padded to a multiple of 32); 128x128x32 workgroup tiles, 4 waves x (2x2)
//                         v_mfma_f32_32x32x2_f32 -- exact fp32 products at the fp32 peak rate -- software-pipelined
//                         through two LDS buffers, and the maximum of every row over each 64-column block on the
//                         side (M).  The score panel IS written to HBM (two panels of <= 4 GiB): at d = 768 that is
//                         4 B per 1536 flops, far below the machine balance.
//   k5_gemm16_panel<T>  : the same panel and block maxima from float16 / bfloat16 operands (pfz_dense_upload16, opt-in):
//                         256x256x64 tiles, 8 waves x (4x2) v_mfma_f32_32x32x16_f16 / _bf16, fp32 accumulation; with
//                         k5_round16 (float32 input, nearest even).
//   k5_gemm8_panel      : the same tile program on int8 operands (pfz_dense_upload8, opt-in): v_mfma_i32_32x32x32_i8, a
//                         k-chunk of 128 values, int32 accumulation (exact, order-independent); with k5_quantize8
//                         (float32 input, symmetric per row).
//   k5_hamming_panel    : the same panel and block maxima from 1-bit operands (pfz_dense_upload1, opt-in: binary embeddings,
//                         np.packbits(x > 0)): no matrix instruction does XOR / popcount, so 128x128 tiles on the vector ALU,
//                         16 x 4 running bit counts per lane; score float(d - 2 h) / float(d), exact; with k5_pack_signs
//                         (float32 input, one ballot per 64 values).
//   k5_row_topn         : wave per row; with M it selects the ntop-th largest block maximum and reads only the
//                         blocks that reach it, without M it streams the row (float4); threshold filter, 64-bit
//                         keys score_bits<<32 | ~col, compaction by wave-max rounds (same scheme as K3), writes
//                         (idx, score) by (score desc, col asc).
//   k5_rescore_topn     : the companion of the 16-bit / int8 / 1-bit operands (pfz_dense_rescore_topn, opt-in): workgroup per
//                         from-row, wave per candidate column of a coarse top-m; the exact score of the fp32 vectors
//                         (float64 sum in a fixed order, rounded once), the same keys, ranked in LDS.
//   k5_mixed_rescore    : its sibling for a to-side kept only as int8 values or bits (pfz_dense_rescore_topn_mixed, opt-in):
//                         the float32 from-row against the quantised to-rows themselves, four candidates per wave.
#include "k5_core.h"

#include <algorithm>
#include <stdlib.h>

namespace pfz {

// Row maxima of a wave's 64 x 64 corner.  x[q] (q = 16 i + r) is the lane's maximum over its two columns of
// accumulator row-slot q; the maximum over the 32 lanes of a half-wave is wanted for all 32 slots.  Halving
// exchange: each step pairs lanes (row_mirror, row_half_mirror, quad xor 2, quad xor 1 by DPP, then lane ^ 16 by
// ds_swizzle), a lane keeps one half of its slots, hands the other half to its partner and folds in what it gets --
// 16 + 8 + 4 + 2 + 1 exchanges instead of 32 x 5, and every lane ends with ONE slot's maximum:
// slot(lane) = bit3 bit2 bit1 bit0 bit4 of the lane id (most significant first).
template <int CTRL>
__device__ inline float dpp_f32(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
__device__ inline float block_row_max(float (&x)[32], int lane)
{
    const bool p3 = lane & 8, p2 = lane & 4, p1 = lane & 2, p0 = lane & 1, p4 = lane & 16;
    float y[16], z[8], u[4], w[2];
#pragma unroll
    for (int t = 0; t < 16; ++t) y[t] = fmaxf(p3 ? x[16 + t] : x[t], dpp_f32<0x140>(p3 ? x[t] : x[16 + t]));     // row_mirror
#pragma unroll
    for (int t = 0; t < 8; ++t) z[t] = fmaxf(p2 ? y[8 + t] : y[t], dpp_f32<0x141>(p2 ? y[t] : y[8 + t]));        // row_half_mirror
#pragma unroll
    for (int t = 0; t < 4; ++t) u[t] = fmaxf(p1 ? z[4 + t] : z[t], dpp_f32<0x4E>(p1 ? z[t] : z[4 + t]));         // quad_perm 2,3,0,1
#pragma unroll
    for (int t = 0; t < 2; ++t) w[t] = fmaxf(p0 ? u[2 + t] : u[t], dpp_f32<0xB1>(p0 ? u[t] : u[2 + t]));         // quad_perm 1,0,3,2
    const float other = __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(p4 ? w[0] : w[1]), 0x401F));   // lane ^ 16
    return fmaxf(p4 ? w[1] : w[0], other);
}
__device__ inline int block_row_slot(int lane)
{
    return ((lane >> 3) & 1) << 4 | ((lane >> 2) & 1) << 3 | ((lane >> 1) & 1) << 2 | (lane & 1) << 1 | ((lane >> 4) & 1);
}

// The tile programs' common end: scale by both inverse norms, store the 128 x 128 tile of S, leave the block maxima in M.
__device__ __forceinline__ void tile_epilogue(f32x16 (&acc)[2][2], const float *__restrict__ inv_a, const float *__restrict__ inv_b,
                                              int64_t a0, int64_t a1, int64_t n_b, float *__restrict__ S, int64_t ld,
                                              float *__restrict__ M, int64_t ldm, int64_t row0, int64_t col0, int wm, int wn, int lane)
{
    // Epilogue.  MFMA 32x32 accumulator r of lane l = row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31.
    // Besides the scores, every wave leaves the maximum of each of its 64 rows over its 64 columns in M[row][col / 64]:
    // the row top-n reads those block maxima (1/64 of the panel) and then only the few blocks that can hold a winner.
    const int cb = (int)((col0 + wn) >> 6);
    if (row0 + kTile <= a1) {
        // interior tile (all but the last row tile of the last panel; ld is a whole number of tiles): the 1/|a| factors
        // come as eight float4 loads issued together, the 64 stores go out back to back from a wave-uniform base plus
        // one 32-bit lane offset.  (Row-by-row predicated code makes the compiler wait for EVERYTHING in flight,
        // the previous store included, before each element: 5.5 us per tile, 13 % of a tile's MFMA time.)
        const int uwm = __builtin_amdgcn_readfirstlane(wm), uwn = __builtin_amdgcn_readfirstlane(wn);
        const float4 *ia = (const float4 *)(inv_a + row0 + uwm) + (lane >> 5);
        float4 sa[2][4];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) sa[i][q] = ia[i * 8 + q * 2];
        float sb[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int64_t col = col0 + uwn + j * 32 + (lane & 31);
            sb[j] = col < n_b ? inv_b[col] : 0.f;
        }
        float *tile = S + (row0 - a0 + uwm) * ld + col0 + uwn;
        const uint32_t lane_off = (uint32_t)(4 * (lane >> 5)) * (uint32_t)ld + (uint32_t)(lane & 31);
        float x[32];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float f = f4c(sa[i][r / 4], r % 4);
                float *rowp = tile + (int64_t)(i * 32 + (r & 3) + 8 * (r >> 2)) * ld;
                const float v0 = acc[i][0][r] * f * sb[0], v1 = acc[i][1][r] * f * sb[1];
                rowp[lane_off] = v0;
                (rowp + 32)[lane_off] = v1;
                x[i * 16 + r] = fmaxf(v0, v1);
            }
        if (M) {
            const float m = block_row_max(x, lane);
            const int q = block_row_slot(lane), rl = (q >> 4) * 32 + (q & 3) + 8 * ((q & 15) >> 2) + 4 * (lane >> 5);
            M[(row0 - a0 + uwm + rl) * ldm + cb] = m;
        }
        return;
    }
    const float sb0 = col0 + wn + (lane & 31) < n_b ? inv_b[col0 + wn + (lane & 31)] : 0.f;
    const float sb1 = col0 + wn + 32 + (lane & 31) < n_b ? inv_b[col0 + wn + 32 + (lane & 31)] : 0.f;
    float xe[32];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = row0 + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            const bool ok = row < a1;
            const float f = ok ? inv_a[row] : 0.f;
            const float v0 = acc[i][0][r] * f * sb0, v1 = acc[i][1][r] * f * sb1;
            if (ok) {
                float *rowp = S + (row - a0) * ld + col0 + wn + (lane & 31);
                rowp[0] = v0;
                rowp[32] = v1;
            }
            xe[i * 16 + r] = ok ? fmaxf(v0, v1) : 0.f;
        }
    }
    if (M) {
        const float m = block_row_max(xe, lane);
        const int q = block_row_slot(lane);
        const int64_t row = row0 + wm + (q >> 4) * 32 + (q & 3) + 8 * ((q & 15) >> 2) + 4 * (lane >> 5);
        if (row < a1) M[(row - a0) * ldm + cb] = m;
    }
}

// The tile program for d % 32 == 0 (embedding widths: 128 ... 768 ... 4096): the software-pipelined main loop of k5_core.h
// (k5_tile_loop, which K14's threshold kernels run too), then the common end.
__global__ __launch_bounds__(256, 2) void k5_gemm_panel_pipe(const void *__restrict__ A, const void *__restrict__ B,
                                                              const float *__restrict__ inv_a, const float *__restrict__ inv_b,
                                                              int64_t a0, int64_t a1, int64_t n_b, int64_t d,
                                                              float *__restrict__ S, int64_t ld, int tiles_m, int tiles_n,
                                                              float *__restrict__ M, int64_t ldm)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // Workgroup -> tile.  Consecutive workgroup ids go round-robin over the 8 XCDs and each XCD has its own L2, so the
    // 64 workgroups an XCD runs at a time (32 CUs x 2) get one 8 x 8 block of tiles: 8 A + 8 B tiles feed 64 tile
    // products out of that L2 (a 1-D sweep over row tiles gives every XCD 32 A tiles + 2 B tiles for the same 64).
    // The grid is a whole number of 8-block rounds; workgroups of blocks or tiles that do not exist leave at once.
    const int w = blockIdx.x, xcd = w & 7, idx = w >> 3, pos = idx & 63;
    const int g = (idx >> 6) * 8 + xcd, bm = (tiles_m + 7) >> 3;
    const int tm = (g % bm) * 8 + (pos & 7), tn = (g / bm) * 8 + (pos >> 3);
    if (tm >= tiles_m || tn >= tiles_n) return;
    const int64_t row0 = a0 + (int64_t)tm * kTile;
    const int64_t col0 = (int64_t)tn * kTile;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    k5_tile_loop(A, B, row0, col0, a1, n_b, d, tid, lane, wm, wn, acc);

    tile_epilogue(acc, inv_a, inv_b, a0, a1, n_b, S, ld, M, ldm, row0, col0, wm, wn, lane);
}

// The norm of the values as stored: the cosine is that of the vectors the GEMM multiplies.  The sum is float64 (for int8
// exact: integer squares, at most 2^14 ld), zero rows stay zero (sklearn normalize).  normalize == 0: raw dot products are
// wanted and every factor is 1 -- unless keep_scale: an int8 row quantised from float32 keeps the scale k5_quantize8 left
// in inv[].
template <typename T>
__global__ __launch_bounds__(256) void k5_inv_norms(const void *__restrict__ x, int64_t n, int64_t d, float *__restrict__ inv,
                                                     int32_t normalize, int32_t keep_scale)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    if (!normalize) {
        if (lane == 0 && !keep_scale) inv[row] = 1.f;
        return;
    }
    const typename T::store_t *p = (const typename T::store_t *)x + row * d;
    double ss = 0.0;
    for (int64_t k = lane; k < d; k += 64) {
        const double v = (double)T::widen(p[k]);
        ss += v * v;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) ss += __shfl_xor(ss, o, 64);
    if (lane == 0) inv[row] = ss > 0.0 ? (float)(1.0 / sqrt(ss)) : 0.f;
}

// fp32 [n][src_ld] -> T [n][ld], round to nearest even, the columns beyond dim zero (16-bit compute asked for float32 input).
// scale: NULL, or a factor per row that is applied first (one fp32 product, rounded to nearest even): with the row's 1 / ||row||
// every value lies in [-1, 1] before it is rounded (pfz_dense_derive16, the search copy of K22).
template <typename T>
__global__ __launch_bounds__(256) void k5_round16(const float *__restrict__ src, int64_t n, int64_t dim, int64_t src_ld, int64_t ld,
                                                   const float *__restrict__ scale, uint16_t *__restrict__ dst)
{
    const int64_t total = n * ld;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / ld, col = i - row * ld;
        float v = 0.f;
        if (col < dim) {
            v = src[row * src_ld + col];
            if (scale) v = __fmul_rn(v, scale[row]);
        }
        dst[i] = col < dim ? T::narrow(v) : (uint16_t)0;
    }
}

// The tile program for 16-bit and 8-bit operands: the workgroup -> tile deal, the main loop of k5_core.h (k5_tile_loop16, which
// K22's threshold search runs too: 256 x 256 tiles, 8 waves of 128 x 64), then the common end, which sees a wave's 128 x 64 as the
// halves wm = 0, 64 of a 128 x 128 tile.  d: the row pitch in values, a multiple of the k-chunk.
template <typename T>
__device__ __forceinline__ void lp_gemm_tile(const void *__restrict__ A, const void *__restrict__ B,
                                             const float *__restrict__ inv_a, const float *__restrict__ inv_b,
                                             int64_t a0, int64_t a1, int64_t n_b, int64_t d,
                                             float *__restrict__ S, int64_t ld, int tiles_m, int tiles_n,
                                             float *__restrict__ M, int64_t ldm)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // workgroup -> tile: consecutive workgroup ids go round-robin over the 8 XCDs; the 32 workgroups an XCD runs at a time (one
    // per CU) get one block of 8 x 4 tiles: 8 A + 4 B tiles (4.7 MB at d = 768 16-bit values) feed 32 tile products out of
    // that XCD's L2
    const int w = blockIdx.x, xcd = w & 7, idx = w >> 3, pos = idx & 31;
    const int g = (idx >> 5) * 8 + xcd, bm = (tiles_m + 7) >> 3;
    const int tm = (g % bm) * 8 + (pos & 7), tn = (g / bm) * 4 + (pos >> 3);
    if (tm >= tiles_m || tn >= tiles_n) return;
    const int64_t row0 = a0 + (int64_t)tm * kTile16;
    const int64_t col0 = (int64_t)tn * kTile16;
    // a wave owns 128 x 64 of the tile: rows 128 vr .., columns 128 vc + wn ..; as seen by the epilogue, the two 64 x 64
    // halves wm = 0, 64 of the 128 x 128 tile (vr, vc)
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

    k5_tile_loop16<T>(A, B, row0, col0, a1, n_b, d, tid, lane, vr, vc, wn, acc);

#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if constexpr (T::kBytes == 1) {
            // int32 sums -> float (exact up to 2^24, to nearest even beyond), then the common end
            f32x16 facc[2][2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) facc[i][j] = __builtin_convertvector(acc[h][i][j], f32x16);
            tile_epilogue(facc, inv_a, inv_b, a0, a1, n_b, S, ld, M, ldm, row0 + vr * 128, col0 + vc * 128, h * 64, wn, lane);
        }
        else
            tile_epilogue(acc[h], inv_a, inv_b, a0, a1, n_b, S, ld, M, ldm, row0 + vr * 128, col0 + vc * 128, h * 64, wn, lane);
    }
}

template <typename T>
__global__ __launch_bounds__(512, 1) void k5_gemm16_panel(const void *__restrict__ A, const void *__restrict__ B,
                                                           const float *__restrict__ inv_a, const float *__restrict__ inv_b,
                                                           int64_t a0, int64_t a1, int64_t n_b, int64_t d,
                                                           float *__restrict__ S, int64_t ld, int tiles_m, int tiles_n,
                                                           float *__restrict__ M, int64_t ldm)
{
    lp_gemm_tile<T>(A, B, inv_a, inv_b, a0, a1, n_b, d, S, ld, tiles_m, tiles_n, M, ldm);
}

// ---- 8-bit integer operands (scalar-quantised embeddings) -----------------------------------------------------------
// The same tile program on int8 values: a k-chunk is 128 values, the sums are int32 and exact (|dot| <= 2^14 dim fits for
// dim <= 131071, which dense_create holds), and the epilogue scales float(sum) by the two per-row factors: 1 / ||q||
// for the cosine; for raw dot products the row's quantisation scale, or 1 for int8 given as it is.
template <typename T>
__global__ __launch_bounds__(512, 1) void k5_gemm8_panel(const void *__restrict__ A, const void *__restrict__ B,
                                                          const float *__restrict__ inv_a, const float *__restrict__ inv_b,
                                                          int64_t a0, int64_t a1, int64_t n_b, int64_t d,
                                                          float *__restrict__ S, int64_t ld, int tiles_m, int tiles_n,
                                                          float *__restrict__ M, int64_t ldm)
{
    lp_gemm_tile<T>(A, B, inv_a, inv_b, a0, a1, n_b, d, S, ld, tiles_m, tiles_n, M, ldm);
}

// fp32 [n][dim] -> int8 [n][ld], symmetric per row: m = max |x|, q = rint((x / m) * 127) -- an fp32 division and an fp32
// product, each rounded to nearest even, then round-half-even to the integer -- and the row's scale m / 127 in scale[row];
// a row of zeros gives zeros and scale 0, the columns beyond dim are zero.  Wave per row.  Non-finite input is outside the
// contract (a NaN or an infinity in a row makes that row's values unspecified).
__global__ __launch_bounds__(256) void k5_quantize8(const float *__restrict__ src, int64_t n, int64_t dim, int64_t ld,
                                                    int8_t *__restrict__ dst, float *__restrict__ scale)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float *p = src + row * dim;
    float m = 0.f;
    for (int64_t k = lane; k < dim; k += 64) m = fmaxf(m, fabsf(p[k]));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    int8_t *q = dst + row * ld;
    for (int64_t k = lane; k < ld; k += 64) {
        float v = 0.f;
        if (k < dim && m > 0.f) v = rintf(__fmul_rn(__fdiv_rn(p[k], m), 127.0f));
        q[k] = (int8_t)(int)v;
    }
    if (lane == 0) scale[row] = __fdiv_rn(m, 127.0f);
}

// ---- 1-bit operands (binary embeddings: np.packbits(x > 0)) ---------------------------------------------------------
// A row is dim bits in np.packbits order (bit k of the row = bit 7 - k % 8 of byte k / 8), stored with a pitch of whole
// 16-byte pieces, the bits beyond dim zero: padding adds no distance.  h = the number of differing bits of two rows; the
// score is that of the +-1 vectors the bits stand for: their dot product dim - 2 h, or -- normalised -- their cosine
// float(dim - 2 h) / float(dim), ONE correctly rounded fp32 division.  dim < 2^24: both are exact functions of h.
constexpr int kB1PitchBits = 128;          // a row's pitch: whole 16-byte pieces
constexpr int64_t kB1MaxBits = (int64_t)1 << 24;

// fp32 [n][dim] -> packed rows [n][pitch bytes], bit = x > 0 (NaN and +-0 give 0).  The test is made on the value's bits --
// positive as an integer and not beyond infinity's -- so that a denormal counts as what it is under any denormal mode.
// Wave per row, one ballot per 64 values: bit l of the ballot is value k0 + l, so byte b of the eight is the bit-reversed b-th
// byte of the mask; lanes 0..7 write it.
__global__ __launch_bounds__(256) void k5_pack_signs(const float *__restrict__ src, int64_t n, int64_t dim, int64_t pitch,
                                                     unsigned char *__restrict__ dst)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float *p = src + row * dim;
    unsigned char *q = dst + row * pitch;
    for (int64_t k0 = 0; k0 < pitch * 8; k0 += 64) {      // (pitch * 8 is a multiple of 128: the eight bytes are inside the row)
        const int64_t k = k0 + lane;
        const int32_t v = k < dim ? __float_as_int(p[k]) : 0;
        const uint64_t mask = __ballot(v > 0 && v <= 0x7f800000);
        if (lane < 8) q[(k0 >> 3) + lane] = (unsigned char)(__brev((uint32_t)(mask >> (8 * lane)) & 0xffu) >> 24);
    }
}

// What k5_hamming_panel gets in the tile programs' `d` argument: the bit count, and bit 32 set for the normalised score.
__host__ __device__ inline int64_t b1_arg(int64_t dim_bits, int32_t normalize) { return dim_bits | ((int64_t)(normalize ? 1 : 0) << 32); }

// The tile program of two 1-bit operands: k5_hamming_loop of k5_core.h (the vector ALU's XOR / popcount loop over a 128 x 128
// tile; thread (tx = tid & 31, ty = tid >> 5) gets the 16 x 4 counts of rows ty + 8 i and columns tx + 32 j), then this end.  The
// epilogue turns a count into the score (see above; columns beyond n_b score 0, as in tile_epilogue), stores
// it -- lanes 0..31 of a store cover one 128-B line of a row -- and leaves the block maxima M[row][col / 64] through the same
// halving exchange as the matrix programs: slot q = 2 i + (j >> 1) of lane (tx, .) is the maximum of row ty + 8 i over the
// thread's two columns of that 64-column block.
__global__ __launch_bounds__(256, 2) void k5_hamming_panel(const void *__restrict__ A, const void *__restrict__ B,
                                                            const float *__restrict__, const float *__restrict__,
                                                            int64_t a0, int64_t a1, int64_t n_b, int64_t d,
                                                            float *__restrict__ S, int64_t ld, int tiles_m, int tiles_n,
                                                            float *__restrict__ M, int64_t ldm)
{
    const int tid = threadIdx.x, lane = tid & 63;
    // workgroup -> tile: as k5_gemm_panel_pipe (8 x 8 tile blocks dealt round-robin to the XCDs)
    const int w = blockIdx.x, xcd = w & 7, idx = w >> 3, pos = idx & 63;
    const int g = (idx >> 6) * 8 + xcd, bm = (tiles_m + 7) >> 3;
    const int tm = (g % bm) * 8 + (pos & 7), tn = (g / bm) * 8 + (pos >> 3);
    if (tm >= tiles_m || tn >= tiles_n) return;
    const int64_t row0 = a0 + (int64_t)tm * kTile;
    const int64_t col0 = (int64_t)tn * kTile;
    const int32_t bits = (int32_t)(d & 0xffffffff);
    const bool normalize = (d >> 32) & 1;
    const int64_t pitch = ((int64_t)bits + kB1PitchBits - 1) / kB1PitchBits * (kB1PitchBits / 8);      // bytes per operand row
    const int tx = tid & 31, ty = tid >> 5;

    int h[16][4];
#pragma unroll
    for (int i = 0; i < 16; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) h[i][j] = 0;
    k5_hamming_loop(A, B, row0, col0, a1, n_b, pitch, tid, tx, ty, h);

    const float fd = (float)bits;
    bool col_ok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) col_ok[j] = col0 + tx + 32 * j < n_b;
    float x[32];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int64_t row = row0 + ty + 8 * i;
        const bool ok = row < a1;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float dot = (float)(bits - 2 * h[i][j]);
            v[j] = col_ok[j] ? (normalize ? __fdiv_rn(dot, fd) : dot) : 0.f;
        }
        if (ok) {
            float *rowp = S + (row - a0) * ld + col0 + tx;
#pragma unroll
            for (int j = 0; j < 4; ++j) rowp[32 * j] = v[j];
        }
        x[2 * i] = ok ? fmaxf(v[0], v[1]) : 0.f;
        x[2 * i + 1] = ok ? fmaxf(v[2], v[3]) : 0.f;
    }
    if (M) {
        const float m = block_row_max(x, lane);
        const int q = block_row_slot(lane);
        const int64_t row = row0 + ty + 8 * (q >> 1);
        if (row < a1) M[(row - a0) * ldm + (col0 >> 6) + (q & 1)] = m;
    }
}

__device__ inline uint64_t wave_max_u64_5(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        uint32_t lo = __shfl_xor((uint32_t)v, d, 64);
        uint32_t hi = __shfl_xor((uint32_t)(v >> 32), d, 64);
        uint64_t o = ((uint64_t)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

// One wave per score row: top-n of the scores > thr.  kCap5: candidate keys per wave (>= ntop + 1 + 64).
// kDeep (round 6: top_n beyond the 1024 keys one pass keeps -- the reference clips top_n to the number of distinct to-strings
// only, _utils.py:54-56): a PASS of a deep top-n.  It keeps the `ntop` best keys strictly BELOW ub[row] (keys are distinct:
// score bits << 32 | ~column), writes them at columns col0 .. of the row's out_ld-wide result and leaves its last key in ub[row]
// for the pass that follows (0 when the row has run out of candidates: nothing is below 0).  The scheme of K3's deep passes.
template <int kCap5, bool kDeep = false>
__global__ __launch_bounds__(256) void k5_row_topn(const float *__restrict__ S, int64_t ld, int64_t a0, int64_t a1,
                                                    int64_t n_b, int32_t ntop, float lower_bound, int32_t exclude_diag,
                                                    int64_t diag_offset, int32_t *__restrict__ out_idx,
                                                    float *__restrict__ out_val, const float *__restrict__ M, int64_t ldm,
                                                    int32_t out_ld = 0, int32_t col0 = 0, uint64_t *__restrict__ ub = nullptr)
{
    __shared__ __attribute__((aligned(16))) uint64_t cand_all[4][kCap5];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = a0 + (int64_t)blockIdx.x * 4 + wave;
    if (row >= a1) return;
    uint64_t *cand = cand_all[wave];
    const float *s = S + (row - a0) * ld;
    const int64_t self_col = exclude_diag ? row + diag_offset : -1;
    int cnt = 0;
    float thr = lower_bound;
    int want = ntop;            // how many keys a compaction keeps
    const uint64_t ubk = kDeep ? ub[row - a0] : ~0ull;

    // sorted == false (intermediate compactions) and a large top_n: select the ntop-th largest key bit by bit
    // (64 ballot steps) instead of one wave-max round per kept key -- the same scheme as K3's compact()
    auto compact = [&](bool sorted) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        uint64_t e[kCap5 / 64];
#pragma unroll
        for (int i = 0; i < kCap5 / 64; ++i) e[i] = lane + 64 * i < cnt ? cand[lane + 64 * i] : 0ull;
        __builtin_amdgcn_wave_barrier();
        if (!sorted && want > 16) {
            if (cnt <= want) return;
            uint64_t T = 0ull;
            for (int bit = 62; bit >= 0; --bit) {   // positive floats: bit 63 is never set
                const uint64_t c = T | (1ull << bit);
                int n = 0;
#pragma unroll
                for (int i = 0; i < kCap5 / 64; ++i) n += __popcll(__ballot(e[i] >= c));
                T = n >= want ? c : T;
            }
            int base = 0;
#pragma unroll
            for (int i = 0; i < kCap5 / 64; ++i) {
                const bool keep_it = e[i] >= T;
                const uint64_t mk = __ballot(keep_it);
                if (keep_it) cand[base + __popcll(mk & ((1ull << lane) - 1ull))] = e[i];
                base += __popcll(mk);
            }
            cnt = base;
            const float t = __uint_as_float((uint32_t)(T >> 32) - 1u);
            thr = t > thr ? t : thr;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            return;
        }
        const int keep = cnt < want ? cnt : want;
        uint64_t best = 0;
        for (int r = 0; r < keep; ++r) {
            uint64_t m = e[0];
#pragma unroll
            for (int i = 1; i < kCap5 / 64; ++i) m = e[i] > m ? e[i] : m;
            best = wave_max_u64_5(m);
#pragma unroll
            for (int i = 0; i < kCap5 / 64; ++i)
                if (e[i] == best) e[i] = 0ull;
            if (lane == 0) cand[r] = best;
        }
        cnt = keep;
        if (keep == want) {
            const float t = __uint_as_float((uint32_t)(best >> 32) - 1u);   // accept >= the want-th score
            thr = t > thr ? t : thr;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };

    if (M) {
        // With block maxima (M[row][b] = max of the row's scores in columns 64 b .. 64 b + 63, diagonal and padding
        // included): the ntop-th largest block maximum T is a lower bound of the ntop-th best score (ntop blocks hold
        // an element >= T each; one more when the diagonal is to be skipped), so only blocks with a maximum >= T can
        // hold a winner -- usually ntop of the n_b / 64.  Pass 1 selects T with the machinery below, pass 2 reads
        // those blocks' scores.
        const float *m = M + (row - a0) * ldm;
        const int64_t n_blocks = (n_b + 63) >> 6;
        want = ntop + (exclude_diag ? 1 : 0);
        for (int64_t b0 = 0; b0 < n_blocks; b0 += 64) {
            const int64_t b = b0 + lane;
            const float v = b < n_blocks ? m[b] : 0.f;
            const bool pred = v > thr;
            const uint64_t mk = __ballot(pred);
            if (!mk) continue;
            const int pos = cnt + __popcll(mk & ((1ull << lane) - 1ull));
            if (pred) cand[pos] = ((uint64_t)__float_as_uint(v) << 32) | (uint32_t)(~(uint32_t)b);
            cnt += __popcll(mk);
            if (cnt > kCap5 - 64) compact(false);
        }
        compact(true);              // cnt == want: thr is now just below the want-th largest block maximum
        cnt = 0;
        want = ntop;
        __builtin_amdgcn_wave_barrier();
        for (int64_t b0 = 0; b0 < n_blocks; b0 += 64) {
            const int64_t b = b0 + lane;
            uint64_t hot = __ballot(b < n_blocks && m[b] > thr);
            while (hot) {
                const int t = __builtin_ctzll(hot);
                hot &= hot - 1;
                const int64_t j = (b0 + t) * 64 + lane;
                const float v = s[j];                       // (j < ld: ld is a whole number of blocks)
                const bool pred = v > thr && j < n_b && j != self_col;
                const uint64_t mk = __ballot(pred);
                if (mk) {
                    const int pos = cnt + __popcll(mk & ((1ull << lane) - 1ull));
                    if (pred) cand[pos] = ((uint64_t)__float_as_uint(v) << 32) | (uint32_t)(~(uint32_t)j);
                    cnt += __popcll(mk);
                    if (cnt > kCap5 - 64) compact(false);
                }
            }
        }
    }
    else
    for (int64_t c0 = 0; c0 < ld; c0 += 256) {
        const int64_t c = c0 + lane * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < ld) v = *(const float4 *)(s + c);
        const float vv[4] = {v.x, v.y, v.z, v.w};
        const float mx = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
        if (!__ballot(mx > thr)) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t j = c + q;
            bool pred = vv[q] > thr && j < n_b && j != self_col;
            if (kDeep) pred = pred && (((uint64_t)__float_as_uint(vv[q]) << 32) | (uint32_t)(~(uint32_t)j)) < ubk;
            const uint64_t mk = __ballot(pred);
            if (mk) {
                const int pos = cnt + __popcll(mk & ((1ull << lane) - 1ull));
                if (pred) cand[pos] = ((uint64_t)__float_as_uint(vv[q]) << 32) | (uint32_t)(~(uint32_t)j);
                cnt += __popcll(mk);
                if (cnt > kCap5 - 64) compact(false);
            }
        }
    }
    compact(true);
    const int64_t o_ld = kDeep ? out_ld : ntop;
    for (int r = lane; r < ntop; r += 64) {
        const uint64_t key = r < cnt ? cand[r] : 0ull;
        out_idx[row * o_ld + col0 + r] = key ? (int32_t)(~(uint32_t)key) : -1;
        out_val[row * o_ld + col0 + r] = key ? __uint_as_float((uint32_t)(key >> 32)) : 0.f;
    }
    if (kDeep && lane == 0) ub[row - a0] = cnt >= ntop ? cand[ntop - 1] : 0ull;
}

// ---- exact rescoring of a coarse top-m ------------------------------------------------------------------------------
// The 16-bit and int8 operands return the ranking of the ROUNDED vectors.  This kernel takes such a result as a candidate
// table -- cand[row][0 .. m), column indices into B, anything outside [0, n_b) (the -1 of an empty slot) skipped wherever
// it stands, real indices distinct within a row -- and scores the candidates against the fp32 vectors:
// score = inv_a[row] inv_b[j] sum_k A[row][k] B[j][k].  One workgroup per from-row, whose vector is shared through LDS
// (kRowInLds: ld <= kRescoreLds floats) or re-read from L2; one wave per candidate at a time, a lane reading 16 B of every
// 1 KiB of the to-row (ld is a multiple of 32 floats: every row starts on a 128 B line and a float4 never crosses the end).
// The sum is float64 -- the product of two floats is exact in it -- in ONE order for a pair whichever wave or slot
// computes it: lane l adds its elements k = 4 l + 256 c + {0, 1, 2, 3} in ascending order, then a xor butterfly over the
// lanes (commutative steps: every lane ends with the same bits), and the product with the two factors is rounded to fp32
// once.  So equal to-rows give equal scores and a permuted candidate list gives the same result.  Gathering m rows of
// 4 ld bytes per from-row, the kernel is bandwidth-bound; the fp64 rate does not show.
// Keys as in k5_row_topn (score bits << 32 | ~column; 0: dropped, scores must be > max(lower_bound, 0)) go to LDS and are
// ranked there: a thread counts the keys above each of its own (m LDS broadcasts) and writes the key of rank r < ntop to
// column r; the columns from the number of keys on are filled with (-1, 0).
constexpr int kRescoreMax = 1024;      // candidates per row: 8 KiB of keys
constexpr int kRescoreLds = 4096;      // widest from-row kept in LDS: 16 KiB

template <bool kRowInLds>
__global__ __launch_bounds__(256) void k5_rescore_topn(const float *__restrict__ A, const float *__restrict__ inv_a, int64_t n_a,
                                                        const float *__restrict__ B, const float *__restrict__ inv_b, int64_t n_b,
                                                        int64_t ld, const int32_t *__restrict__ cand, int32_t m, int32_t ntop,
                                                        float lower_bound, int32_t *__restrict__ out_idx,
                                                        float *__restrict__ out_val)
{
    __shared__ __attribute__((aligned(16))) uint64_t keys[kRescoreMax];
    __shared__ __attribute__((aligned(16))) float xs[kRowInLds ? kRescoreLds : 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int64_t row = blockIdx.x; row < n_a; row += gridDim.x) {
        const float *xa = A + row * ld;
        if (kRowInLds) {
            for (int k = tid * 4; k < (int)ld; k += 1024) *(float4 *)(xs + k) = *(const float4 *)(xa + k);
            __syncthreads();
        }
        const double fa = (double)inv_a[row];
        const int32_t *c = cand + row * m;
        for (int slot = wave; slot < m; slot += 4) {
            const int32_t j = __builtin_amdgcn_readfirstlane(c[slot]);
            uint64_t key = 0ull;
            if (j >= 0 && j < n_b) {
                const float s = k5_pair_score(kRowInLds ? xs : xa, B + (int64_t)j * ld, ld, fa, (double)inv_b[j], lane);
                if (s > lower_bound) key = ((uint64_t)__float_as_uint(s) << 32) | (uint32_t)(~(uint32_t)j);
            }
            if (lane == 0) keys[slot] = key;
        }
        __syncthreads();
        uint64_t mine[kRescoreMax / 256];
        int rank[kRescoreMax / 256];
#pragma unroll
        for (int u = 0; u < kRescoreMax / 256; ++u) {
            mine[u] = tid + 256 * u < m ? keys[tid + 256 * u] : 0ull;
            rank[u] = 0;
        }
        int n_keys = 0;
        for (int q = 0; q < m; ++q) {
            const uint64_t k = keys[q];
            n_keys += k != 0ull;
#pragma unroll
            for (int u = 0; u < kRescoreMax / 256; ++u) rank[u] += k > mine[u];
        }
        int32_t *oi = out_idx + row * ntop;
        float *ov = out_val + row * ntop;
#pragma unroll
        for (int u = 0; u < kRescoreMax / 256; ++u)
            if (mine[u] && rank[u] < ntop) {
                oi[rank[u]] = (int32_t)(~(uint32_t)mine[u]);
                ov[rank[u]] = __uint_as_float((uint32_t)(mine[u] >> 32));
            }
        for (int r = n_keys + tid; r < ntop; r += 256) {
            oi[r] = -1;
            ov[r] = 0.f;
        }
        __syncthreads();      // the next row reuses keys and xs
    }
}

// ---- rescoring float32 from-vectors against the int8 / 1-bit to-operand itself --------------------------------------------
// The sibling of k5_rescore_topn for a to-side that exists only in its quantised form (pfz_dense_rescore_topn_mixed): the
// same candidate table, keys, bound, ranking and result, one workgroup per from-row whose float32 vector is shared through LDS
// (kRowInLds) or re-read from L2 -- but the to-row of a candidate is int8 values or packed sign bits, 768 or 96 bytes at
// d = 768 where the float32 row has 3 072.  A wave per candidate would leave most lanes without a byte to read, so a wave
// scores FOUR candidates at a time, 16 lanes each; lane g of a group reads one piece per step and the steps follow each other
// along the row:
//   int8: a piece is 16 B = values k = 256 c + 16 g + 0 .. 15 (a step is 256 B of the row: two 128 B lines per candidate);
//         term a[k] * q[k], an fma in float64 -- the product of a float and an int8 is exact in it.
//   bits: a piece is  8 B = bits   k = 1024 c + 64 g + 0 .. 63 (a step is 128 B: one line; a 96-byte row fills 12 of the 16
//         lanes); term a[k] or -a[k] as the bit says, exact: the sum is the dot product with the +-1 vector the Hamming
//         score speaks of.
// The three pitches differ: the float32 row ends at ld_a (a multiple of 32 values), the int8 row at a multiple of 128 values,
// the bit row at a multiple of 128 bits; a piece is read only when it starts inside the to-row's pitch, a float4 of the
// from-row only inside ld_a, and what lies between dim and either end is zero in the from-row, so it adds +-0.
// A lane takes the float4s of its piece in the order (t + r) mod n, r = g (bits: n = 16) or g / 4 (int8: n = 4): the 16 lanes
// of a group then read 16 different bank quads of LDS in every step instead of one.  The order of a pair's sum is therefore a
// function of k and the to-type alone -- g, c and r follow from k -- whichever wave, group or slot scores it: ascending steps
// within a lane, then a xor butterfly over the group's 16 lanes (commutative steps: every lane ends with the same bits).
// Equal to-rows give equal score bits and a permuted candidate list the same result, as k5_rescore_topn documents.
// score: int8 fp32(inv_a[row] inv_b[j] sum) with the handle's own factor (1 / ||q||, the row's scale, or 1); bits
// fp32(inv_a[row] sum / sqrt(dim)) -- the cosine of the float vector and the +-1 vector -- or fp32(sum) when not normalised.
template <bool kBits, bool kRowInLds>
__global__ __launch_bounds__(256) void k5_mixed_rescore(const float *__restrict__ A, const float *__restrict__ inv_a, int64_t n_a,
                                                         int64_t ld_a, const unsigned char *__restrict__ B,
                                                         const float *__restrict__ inv_b, int64_t n_b, int64_t pitch_b,
                                                         int64_t dim, int32_t normalize, const int32_t *__restrict__ cand, int32_t m,
                                                         int32_t ntop, float lower_bound, int32_t *__restrict__ out_idx,
                                                         float *__restrict__ out_val)
{
    __shared__ __attribute__((aligned(16))) uint64_t keys[kRescoreMax];
    __shared__ __attribute__((aligned(16))) float xs[kRowInLds ? kRescoreLds : 4];
    constexpr int kPiece = kBits ? 64 : 16;            // values of a lane's piece
    constexpr int kStep = 16 * kPiece;                 // values of a group's step
    constexpr int kSteps = kBits ? 2 : 4;              // steps whose loads are in flight together
    const int tid = threadIdx.x, wave = tid >> 6, grp = (tid >> 4) & 3, g = tid & 15;
    const int rot = kBits ? g : g >> 2;
    const int len_a = (int)ld_a, len_b = (int)(kBits ? pitch_b * 8 : pitch_b);      // the two rows' ends, in values
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const double root_dim = sqrt((double)dim);
    for (int64_t row = blockIdx.x; row < n_a; row += gridDim.x) {
        const float *xa = A + row * ld_a;
        if (kRowInLds) {
            for (int k = tid * 4; k < len_a; k += 1024) *(float4 *)(xs + k) = *(const float4 *)(xa + k);
            __syncthreads();
        }
        const float *pa = kRowInLds ? xs : xa;
        const double fa = (double)inv_a[row];
        const int32_t *c = cand + row * m;
        for (int slot0 = 0; slot0 < m; slot0 += 16) {
            const int slot = slot0 + wave * 4 + grp;
            const int32_t j = slot < m ? c[slot] : -1;
            const bool live = j >= 0 && j < n_b;
            double acc = 0.0;
            if (live) {
                const unsigned char *xb = B + (int64_t)j * pitch_b;
                for (int k0 = 0; k0 < len_b; k0 += kSteps * kStep) {
                    if (kBits) {
                        uint2 w[kSteps];
#pragma unroll
                        for (int u = 0; u < kSteps; ++u) {
                            const int k = k0 + u * kStep + g * kPiece;
                            w[u] = k < len_b ? *(const uint2 *)(xb + (k >> 3)) : make_uint2(0u, 0u);
                        }
#pragma unroll
                        for (int u = 0; u < kSteps; ++u) {
                            const int k = k0 + u * kStep + g * kPiece;
                            if (k >= len_b) continue;
                            const uint64_t bits = ((uint64_t)w[u].y << 32) | w[u].x;
#pragma unroll 4
                            for (int t = 0; t < 16; ++t) {
                                const int tt = (t + rot) & 15, ka = k + 4 * tt;
                                const float4 a = ka < len_a ? *(const float4 *)(pa + ka) : zero;
                                // values 4 tt .. 4 tt + 3 of the piece: byte tt / 2, its high nibble first, most significant bit first
                                const uint32_t nib = ~(uint32_t)(bits >> (8 * (tt >> 1) + 4 * (1 - (tt & 1))));
                                acc += (double)__uint_as_float(__float_as_uint(a.x) ^ ((nib << 28) & 0x80000000u));
                                acc += (double)__uint_as_float(__float_as_uint(a.y) ^ ((nib << 29) & 0x80000000u));
                                acc += (double)__uint_as_float(__float_as_uint(a.z) ^ ((nib << 30) & 0x80000000u));
                                acc += (double)__uint_as_float(__float_as_uint(a.w) ^ ((nib << 31) & 0x80000000u));
                            }
                        }
                    }
                    else {
                        u32x4 q[kSteps];
#pragma unroll
                        for (int u = 0; u < kSteps; ++u) {
                            const int k = k0 + u * kStep + g * kPiece;
                            const u32x4 none = {0u, 0u, 0u, 0u};
                            q[u] = k < len_b ? *(const u32x4 *)(xb + k) : none;
                        }
#pragma unroll
                        for (int u = 0; u < kSteps; ++u) {
                            const int k = k0 + u * kStep + g * kPiece;
                            if (k >= len_b) continue;
#pragma unroll
                            for (int t = 0; t < 4; ++t) {
                                const int tt = (t + rot) & 3, ka = k + 4 * tt;
                                const float4 a = ka < len_a ? *(const float4 *)(pa + ka) : zero;
                                const int32_t v = (int32_t)(tt == 0 ? q[u].x : tt == 1 ? q[u].y : tt == 2 ? q[u].z : q[u].w);
                                acc = fma((double)a.x, (double)((v << 24) >> 24), acc);
                                acc = fma((double)a.y, (double)((v << 16) >> 24), acc);
                                acc = fma((double)a.z, (double)((v << 8) >> 24), acc);
                                acc = fma((double)a.w, (double)(v >> 24), acc);
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int o = 8; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);      // (within the group of 16; every lane takes part)
            uint64_t key = 0ull;
            if (live) {
                const float s = kBits ? (normalize ? (float)(fa * acc / root_dim) : (float)acc) : (float)(fa * (double)inv_b[j] * acc);
                if (s > lower_bound) key = ((uint64_t)__float_as_uint(s) << 32) | (uint32_t)(~(uint32_t)j);
            }
            if (g == 0 && slot < m) keys[slot] = key;
        }
        __syncthreads();
        // the ranking of k5_rescore_topn: a thread counts the keys above each of its own and writes rank r < ntop to column r
        uint64_t mine[kRescoreMax / 256];
        int rank[kRescoreMax / 256];
#pragma unroll
        for (int u = 0; u < kRescoreMax / 256; ++u) {
            mine[u] = tid + 256 * u < m ? keys[tid + 256 * u] : 0ull;
            rank[u] = 0;
        }
        int n_keys = 0;
        for (int q = 0; q < m; ++q) {
            const uint64_t k = keys[q];
            n_keys += k != 0ull;
#pragma unroll
            for (int u = 0; u < kRescoreMax / 256; ++u) rank[u] += k > mine[u];
        }
        int32_t *oi = out_idx + row * ntop;
        float *ov = out_val + row * ntop;
#pragma unroll
        for (int u = 0; u < kRescoreMax / 256; ++u)
            if (mine[u] && rank[u] < ntop) {
                oi[rank[u]] = (int32_t)(~(uint32_t)mine[u]);
                ov[rank[u]] = __uint_as_float((uint32_t)(mine[u] >> 32));
            }
        for (int r = n_keys + tid; r < ntop; r += 256) {
            oi[r] = -1;
            ov[r] = 0.f;
        }
        __syncthreads();      // the next row reuses keys and xs
    }
}

}  // namespace pfz

using namespace pfz;

static int64_t dense_dtype_bytes(int32_t dtype)
{
    return dtype == PFZ_DENSE_F32 ? f32::kBytes : dtype == PFZ_DENSE_I8 ? i8::kBytes : f16::kBytes;
}

// host [n][dim] values of `elem` bytes -> device [n][ld], the columns beyond dim zero (padded in pieces of 32 MiB)
static int upload_rows_padded(pfz_ctx *ctx, void *dst, const void *src, int64_t n, int64_t dim, int64_t ld, int64_t elem)
{
    if (ld == dim) return copy_h2d(ctx, dst, src, (size_t)n * (size_t)dim * (size_t)elem);
    const int64_t rows_per = std::max<int64_t>(1, ((int64_t)32 << 20) / (ld * elem));
    std::vector<unsigned char> padded((size_t)std::min(rows_per, n) * (size_t)(ld * elem), (unsigned char)0);
    const unsigned char *v = (const unsigned char *)src;
    for (int64_t r0 = 0; r0 < n; r0 += rows_per) {
        const int64_t rows = std::min(rows_per, n - r0);
        for (int64_t r = 0; r < rows; ++r)
            std::copy(v + (r0 + r) * dim * elem, v + (r0 + r + 1) * dim * elem, padded.begin() + (size_t)(r * ld * elem));
        PFZ_TRY(copy_h2d(ctx, (unsigned char *)dst + r0 * ld * elem, padded.data(), (size_t)rows * (size_t)(ld * elem)));
    }
    return PFZ_OK;
}

// The one constructor of a K5 operand: `vec` holds values of `dtype` (PFZ_DENSE_SRC_SAME) or float32 values that are rounded
// / quantised to it on the device (PFZ_DENSE_SRC_F32).  `who`: the entry point, for the messages.
static int dense_create(pfz_ctx *ctx, const char *who, const void *vec, int64_t n, int64_t dim, int32_t normalize, int32_t dtype,
                        int32_t source, pfz_dense **out)
{
    PFZ_REQUIRE(ctx && out && (n == 0 || vec), "%s: NULL argument", who);
    PFZ_REQUIRE(n >= 0 && dim >= 1, "%s: bad shape %lld x %lld", who, (long long)n, (long long)dim);
    PFZ_REQUIRE(source == PFZ_DENSE_SRC_SAME || source == PFZ_DENSE_SRC_F32, "%s: unknown source %d", who, source);
    if (n >= ((int64_t)1 << 31) - 256) {
        set_error("%s: %lld rows exceed the int32 result indices", who, (long long)n);
        return PFZ_ERR_UNSUPPORTED;
    }
    constexpr int64_t kMaxDim8 = 131071;     // 128 * 128 * dim <= 2^31 - 1: a dot product of int8 rows fits its int32 sum
    if (dtype == PFZ_DENSE_I8 && dim > kMaxDim8) {
        set_error("%s: %lld columns exceed the %lld an int32 dot product of int8 rows can hold", who, (long long)dim,
                  (long long)kMaxDim8);
        return PFZ_ERR_UNSUPPORTED;
    }
    if (dtype == PFZ_DENSE_B1 && dim >= kB1MaxBits) {
        set_error("%s: %lld bits exceed the %lld up to which dim - 2 h is exact in float32", who, (long long)dim, (long long)kB1MaxBits - 1);
        return PFZ_ERR_UNSUPPORTED;
    }
    PFZ_HIP(hipSetDevice(ctx->device));
    Owner<pfz_dense, pfz_dense_free> m(new pfz_dense());
    m->ctx = ctx;
    m->n = n;
    m->dim = dim;
    m->dtype = dtype;
    if (dtype == PFZ_DENSE_B1) {
        // 1-bit rows: no k-chunk padding and no norms.  Packed rows of (dim + 7) / 8 bytes go up as they are, float32 rows are
        // packed on the device; either way the pitch is whole 16-byte pieces and the bits beyond dim are zero.
        const int64_t ld = m->ld = (dim + kB1PitchBits - 1) / kB1PitchBits * kB1PitchBits, pitch = ld / 8;
        m->normalize = normalize ? 1 : 0;
        PFZ_TRY(pool_alloc(ctx, &m->x, (size_t)(n > 0 ? n : 1) * (size_t)pitch));
        PFZ_TRY(pool_alloc(ctx, &m->inv, (size_t)(n > 0 ? n : 1) * sizeof(float)));
        if (n > 0) {
            const dim3 rows4((unsigned)((n + 3) / 4));
            if (source == PFZ_DENSE_SRC_F32) {
                DevBuf tmp;      // (freed at the end of this block: stream order keeps it alive until the kernel is done)
                PFZ_TRY(tmp.alloc(ctx, (size_t)n * (size_t)dim * sizeof(float)));
                PFZ_TRY(copy_h2d(ctx, tmp.p, vec, (size_t)n * (size_t)dim * sizeof(float)));
                hipLaunchKernelGGL(k5_pack_signs, rows4, dim3(256), 0, ctx->stream, (const float *)tmp.p, n, dim, pitch, (unsigned char *)m->x);
                PFZ_HIP(hipGetLastError());
            }
            else
                PFZ_TRY(upload_rows_padded(ctx, m->x, vec, n, (dim + 7) / 8, pitch, 1));
            hipLaunchKernelGGL(k5_inv_norms<f32>, rows4, dim3(256), 0, ctx->stream, (const void *)m->x, n, (int64_t)0, m->inv, 0, 0);
            PFZ_HIP(hipGetLastError());
        }
        *out = m.release();
        return PFZ_OK;
    }
    // Widths that are not a multiple of the GEMM's k-chunk (300-d word vectors) are padded with zero columns on the device:
    // dot products and norms do not change and every width takes the pipelined tile program.
    const int64_t bytes = dense_dtype_bytes(dtype), chunk = kChunkBytes / bytes;
    const int64_t ld = m->ld = (dim + chunk - 1) / chunk * chunk;
    m->normalize = normalize ? 1 : 0;
    PFZ_TRY(pool_alloc(ctx, &m->x, (size_t)(n > 0 ? n : 1) * (size_t)ld * (size_t)bytes));
    PFZ_TRY(pool_alloc(ctx, &m->inv, (size_t)(n > 0 ? n : 1) * sizeof(float)));
    if (n > 0) {
        const dim3 rows4((unsigned)((n + 3) / 4));
        const bool convert = source == PFZ_DENSE_SRC_F32 && dtype != PFZ_DENSE_F32;
        if (convert) {
            // float32 values: uploaded as they are, rounded or quantised (and padded) on the device; the row scales of
            // k5_quantize8 land in inv[]
            DevBuf tmp;      // (freed at the end of this block: stream order keeps it alive until the kernel is done)
            PFZ_TRY(tmp.alloc(ctx, (size_t)n * (size_t)dim * sizeof(float)));
            PFZ_TRY(copy_h2d(ctx, tmp.p, vec, (size_t)n * (size_t)dim * sizeof(float)));
            if (dtype == PFZ_DENSE_I8)
                hipLaunchKernelGGL(k5_quantize8, rows4, dim3(256), 0, ctx->stream, (const float *)tmp.p, n, dim, ld, (int8_t *)m->x, m->inv);
            else {
                const int64_t blocks = std::min<int64_t>((n * ld + 255) / 256, 65536);
                hipLaunchKernelGGL(dtype == PFZ_DENSE_F16 ? k5_round16<f16> : k5_round16<bf16>, dim3((unsigned)blocks), dim3(256), 0,
                                   ctx->stream, (const float *)tmp.p, n, dim, dim, ld, (const float *)nullptr, (uint16_t *)m->x);
            }
            PFZ_HIP(hipGetLastError());
        }
        else
            PFZ_TRY(upload_rows_padded(ctx, m->x, vec, n, dim, ld, bytes));
        auto *norms = dtype == PFZ_DENSE_F16 ? k5_inv_norms<f16> : dtype == PFZ_DENSE_BF16 ? k5_inv_norms<bf16>
                      : dtype == PFZ_DENSE_I8 ? k5_inv_norms<i8> : k5_inv_norms<f32>;
        hipLaunchKernelGGL(norms, rows4, dim3(256), 0, ctx->stream, (const void *)m->x, n, ld, m->inv, m->normalize,
                           (int32_t)(convert && dtype == PFZ_DENSE_I8));
        PFZ_HIP(hipGetLastError());
    }
    *out = m.release();
    return PFZ_OK;
}

// The tile program of an operand type: its kernel, the edge of its square workgroup tile, its workgroup size and how many
// tile columns the 8-row block has that one XCD works on at a time.
typedef void (*gemm_fn)(const void *, const void *, const float *, const float *, int64_t, int64_t, int64_t, int64_t, float *, int64_t,
                        int, int, float *, int64_t);
struct GemmPlan {
    gemm_fn kernel;
    int tile, threads, block_n;
};
static GemmPlan gemm_plan(int32_t dtype)
{
    switch (dtype) {
    case PFZ_DENSE_F16: return {k5_gemm16_panel<f16>, kTile16, 512, 4};
    case PFZ_DENSE_BF16: return {k5_gemm16_panel<bf16>, kTile16, 512, 4};
    case PFZ_DENSE_I8: return {k5_gemm8_panel<i8>, kTile16, 512, 4};
    case PFZ_DENSE_B1: return {k5_hamming_panel, kTile, 256, 8};
    default: return {k5_gemm_panel_pipe, kTile, 256, 8};
    }
}

extern "C" {

void pfz_dense_free(pfz_dense *m)
{
    if (!m) return;
    if (m->ctx) (void)hipSetDevice(m->ctx->device);
    if (m->x) pool_free(m->x);
    if (m->inv) pool_free(m->inv);
    delete m;
}

int pfz_dense_upload(pfz_ctx *ctx, const float *vec, int64_t n, int64_t dim, int32_t normalize, pfz_dense **out)
{
    return dense_create(ctx, "pfz_dense_upload", vec, n, dim, normalize, PFZ_DENSE_F32, PFZ_DENSE_SRC_SAME, out);
}

int pfz_dense_upload16(pfz_ctx *ctx, const void *vec, int64_t n, int64_t dim, int32_t normalize, int32_t dtype, int32_t source,
                       pfz_dense **out)
{
    PFZ_REQUIRE(dtype == PFZ_DENSE_F16 || dtype == PFZ_DENSE_BF16, "pfz_dense_upload16: dtype %d is neither PFZ_DENSE_F16 nor PFZ_DENSE_BF16",
                dtype);
    return dense_create(ctx, "pfz_dense_upload16", vec, n, dim, normalize, dtype, source, out);
}

int pfz_dense_upload8(pfz_ctx *ctx, const void *vec, int64_t n, int64_t dim, int32_t normalize, int32_t source, pfz_dense **out)
{
    return dense_create(ctx, "pfz_dense_upload8", vec, n, dim, normalize, PFZ_DENSE_I8, source, out);
}

int pfz_dense_upload1(pfz_ctx *ctx, const void *vec, int64_t n, int64_t dim_bits, int32_t normalize, int32_t source, pfz_dense **out)
{
    return dense_create(ctx, "pfz_dense_upload1", vec, n, dim_bits, normalize, PFZ_DENSE_B1, source, out);
}

int pfz_dense_derive16(pfz_ctx *ctx, const pfz_dense *exact, int32_t dtype, pfz_dense **out)
{
    PFZ_REQUIRE(ctx && exact && out, "pfz_dense_derive16: NULL argument");
    PFZ_REQUIRE(dtype == PFZ_DENSE_F16 || dtype == PFZ_DENSE_BF16, "pfz_dense_derive16: dtype %d is neither PFZ_DENSE_F16 nor PFZ_DENSE_BF16",
                dtype);
    PFZ_REQUIRE(exact->dtype == PFZ_DENSE_F32 && exact->normalize,
                "pfz_dense_derive16: the vectors are %s, uploaded with normalize = %d; the search copy is derived from fp32 vectors "
                "uploaded with normalize = 1 (pfz_dense_upload)", dense_dtype_name(exact->dtype), exact->normalize);
    PFZ_HIP(hipSetDevice(ctx->device));
    Owner<pfz_dense, pfz_dense_free> m(new pfz_dense());
    const int64_t n = exact->n, chunk = kChunkBytes / f16::kBytes;
    m->ctx = ctx;
    m->n = n;
    m->dim = exact->dim;
    m->dtype = dtype;
    m->normalize = 1;
    const int64_t ld = m->ld = (exact->dim + chunk - 1) / chunk * chunk;
    PFZ_TRY(pool_alloc(ctx, &m->x, (size_t)(n > 0 ? n : 1) * (size_t)ld * (size_t)f16::kBytes));
    PFZ_TRY(pool_alloc(ctx, &m->inv, (size_t)(n > 0 ? n : 1) * sizeof(float)));
    if (n > 0) {
        const int64_t blocks = std::min<int64_t>((n * ld + 255) / 256, 65536);
        hipLaunchKernelGGL(dtype == PFZ_DENSE_F16 ? k5_round16<f16> : k5_round16<bf16>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream,
                           (const float *)exact->x, n, exact->dim, exact->ld, ld, (const float *)exact->inv, (uint16_t *)m->x);
        PFZ_HIP(hipGetLastError());
        hipLaunchKernelGGL(dtype == PFZ_DENSE_F16 ? k5_inv_norms<f16> : k5_inv_norms<bf16>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0,
                           ctx->stream, (const void *)m->x, n, ld, m->inv, 1, 0);
        PFZ_HIP(hipGetLastError());
    }
    *out = m.release();
    return PFZ_OK;
}

int pfz_dense_dtype(const pfz_dense *m, int32_t *dtype)
{
    PFZ_REQUIRE(m && dtype, "pfz_dense_dtype: NULL argument");
    *dtype = m->dtype;
    return PFZ_OK;
}

int pfz_dense_shape(const pfz_dense *m, int64_t *n, int64_t *dim)
{
    PFZ_REQUIRE(m, "pfz_dense_shape: NULL matrix");
    if (n) *n = m->n;
    if (dim) *dim = m->dim;
    return PFZ_OK;
}

int pfz_dense_topn(pfz_ctx *ctx, const pfz_dense *from, const pfz_dense *to, int32_t ntop, float lower_bound,
                   int32_t exclude_diag, int64_t diag_offset, pfz_topn *out)
{
    PFZ_REQUIRE(ctx && from && to && out, "pfz_dense_topn: NULL argument");
    PFZ_REQUIRE(from->dtype != PFZ_DENSE_B1 || to->dtype != PFZ_DENSE_B1 || from->dim == to->dim,
                "pfz_dense_topn: from-vectors have %lld bits, to-vectors %lld (rows packed on the host count 8 bits per byte: float "
                "vectors whose width is not a multiple of 8 cannot be paired with them -- pack both sides the same way)",
                (long long)from->dim, (long long)to->dim);
    PFZ_REQUIRE(from->dim == to->dim, "pfz_dense_topn: from-vectors have %lld columns, to-vectors %lld", (long long)from->dim,
                (long long)to->dim);
    PFZ_REQUIRE(from->dtype == to->dtype, "pfz_dense_topn: from-vectors are %s, to-vectors %s: upload both with one compute type",
                dense_dtype_name(from->dtype), dense_dtype_name(to->dtype));
    PFZ_REQUIRE(ntop >= 1, "pfz_dense_topn: ntop must be >= 1");
    PFZ_REQUIRE(lower_bound == lower_bound, "pfz_dense_topn: lower_bound is NaN");
    constexpr int32_t kDeepPass = 1024;      // keys one pass keeps (k5_row_topn<1152>)
    PFZ_REQUIRE(out->n_rows >= from->n && out->ntop == ntop, "pfz_dense_topn: result buffer is %lldx%d, need %lldx%d",
                (long long)out->n_rows, out->ntop, (long long)from->n, ntop);
    PFZ_REQUIRE(from->dtype != PFZ_DENSE_B1 || from->normalize == to->normalize,
                "pfz_dense_topn: one binary operand was uploaded with normalize, the other without: the score is one or the other");
    // the padded width: a multiple of the type's k-chunk; 1-bit operands: the bit count and which score (b1_arg)
    const int64_t n_from = from->n, n_to = to->n, dim = from->dtype == PFZ_DENSE_B1 ? b1_arg(from->dim, from->normalize) : from->ld;
    if (n_from == 0) return PFZ_OK;
    PFZ_HIP(hipSetDevice(ctx->device));
    if (lower_bound < 0.f) lower_bound = 0.f;   // non-positive similarities are "no match" (_utils.py:122-123)
    const GemmPlan gp = gemm_plan(from->dtype);
    DevBuf dS[2], dM[2], dU[2];
    const int64_t ld = ((n_to + 255) / 256) * 256;                      // whole float4 x 64-lane steps
    // Two score panels of <= 4 GiB.  At 500 000 to-vectors that is 2048 rows: each B tile
    // serves 16 row tiles per panel.  (16 GiB panels are 1.5 % faster per step -- B is re-read once per panel -- but
    // their first allocation costs a second, which a one-shot host call cannot afford.)  The row top-n of panel p
    // runs on a side stream while the GEMM of panel p + 1 fills the other buffer; with block maxima it is a ~0.2 ms
    // kernel per panel and the overlap no longer matters, without them (d % 32 != 0) it is a full read of the panel.
    const int64_t panel_bytes = (int64_t)4 << 30;
    int64_t panel = ld > 0 ? panel_bytes / (ld * 4) : n_from;
    if (const char *forced = knob_str(knob::K5_PANEL_ROWS)) panel = atoll(forced);   // tests: several panels on small inputs
    panel = std::max<int64_t>(kTile, std::min<int64_t>(panel / kTile * kTile, ((n_from + kTile - 1) / kTile) * kTile));
    const int64_t n_panels = (n_from + panel - 1) / panel;
    const bool two = n_panels > 1 && !knob_set(knob::K5_NO_OVERLAP);       // env: A/B timing
    if (two) PFZ_TRY(ensure_side_stream(ctx));
    if (ld > 0) {
        PFZ_TRY(dS[0].alloc(ctx, (size_t)panel * (size_t)ld * sizeof(float)));
        if (two) PFZ_TRY(dS[1].alloc(ctx, (size_t)panel * (size_t)ld * sizeof(float)));
        // block maxima (one float per row and 64 columns), written by the second-generation GEMM
        PFZ_TRY(dM[0].alloc(ctx, (size_t)panel * (size_t)(ld / 64) * sizeof(float)));
        if (two) PFZ_TRY(dM[1].alloc(ctx, (size_t)panel * (size_t)(ld / 64) * sizeof(float)));
    }
    if (ntop > kDeepPass) {      // a deep top-n: every row's last key of the pass before
        PFZ_TRY(dU[0].alloc(ctx, (size_t)panel * sizeof(uint64_t)));
        if (two) PFZ_TRY(dU[1].alloc(ctx, (size_t)panel * sizeof(uint64_t)));
    }
    hipEvent_t *ready = ctx->side_events, *consumed = ctx->side_events + 2;
    int64_t pi = 0;
    for (int64_t a0 = 0; a0 < n_from; a0 += panel, ++pi) {
        const int64_t a1 = std::min(n_from, a0 + panel);
        const int buf = two ? (int)(pi & 1) : 0;
        float *S = (float *)dS[buf].p;
        const float *M = nullptr;          // set when the GEMM leaves block maxima
        if (two && pi >= 2) PFZ_HIP(hipStreamWaitEvent(ctx->stream, consumed[buf], 0));   // the top-n of panel pi - 2 read this buffer
        if (ld > 0) {
            ProfScope ps(ctx, "k5_gemm_panel");
            if (n_to > 0) {
                // 1-D grid of 8 x block_n tile blocks dealt round-robin to the 8 XCDs (see the kernels; ld is a whole number
                // of tiles of either edge)
                const int tiles_m = (int)((a1 - a0 + gp.tile - 1) / gp.tile), tiles_n = (int)(ld / gp.tile);
                const int blocks = ((tiles_m + 7) / 8) * ((tiles_n + gp.block_n - 1) / gp.block_n);
                const dim3 grid((unsigned)((blocks + 7) / 8 * 8 * 8 * gp.block_n));
                M = knob_set(knob::K5_NO_BLOCK_MAX) ? nullptr : (const float *)dM[buf].p;      // A/B knob, tests
                hipLaunchKernelGGL(gp.kernel, grid, dim3(gp.threads), 0, ctx->stream, (const void *)from->x, (const void *)to->x,
                                   (const float *)from->inv, (const float *)to->inv, a0, a1, n_to, dim, S, ld, tiles_m, tiles_n,
                                   (float *)M, ld / 64);
            }
        }
        hipStream_t ts = two ? ctx->stream2 : ctx->stream;
        if (two) {
            PFZ_HIP(hipEventRecord(ready[buf], ctx->stream));
            PFZ_HIP(hipStreamWaitEvent(ts, ready[buf], 0));
        }
        {
            ProfScope ps(ctx, "k5_row_topn", ts);
            if (ntop > kDeepPass) {
                // passes of 1024 over the same score panel, each continuing strictly below the last key of the one before (the
                // block maxima are of no use below a bound: the passes stream the rows)
                PFZ_HIP(hipMemsetAsync(dU[buf].p, 0xff, (size_t)(a1 - a0) * sizeof(uint64_t), ts));
                for (int32_t col0 = 0; col0 < ntop; col0 += kDeepPass)
                    hipLaunchKernelGGL((k5_row_topn<1152, true>), dim3((unsigned)((a1 - a0 + 3) / 4)), dim3(256), 0, ts, (const float *)S, ld,
                                       a0, a1, n_to, std::min(kDeepPass, ntop - col0), lower_bound, exclude_diag, diag_offset, out->idx,
                                       out->val, (const float *)nullptr, ld / 64, ntop, col0, (uint64_t *)dU[buf].p);
            }
            else if (ntop <= 128)
                hipLaunchKernelGGL(k5_row_topn<256>, dim3((unsigned)((a1 - a0 + 3) / 4)), dim3(256), 0, ts, (const float *)S, ld, a0,
                                   a1, n_to, ntop, lower_bound, exclude_diag, diag_offset, out->idx, out->val, M, ld / 64);
            else
                hipLaunchKernelGGL(k5_row_topn<1152>, dim3((unsigned)((a1 - a0 + 3) / 4)), dim3(256), 0, ts, (const float *)S, ld, a0,
                                   a1, n_to, ntop, lower_bound, exclude_diag, diag_offset, out->idx, out->val, M, ld / 64);
        }
        if (two) PFZ_HIP(hipEventRecord(consumed[buf], ts));
    }
    if (two) {   // later work on the context stream (downloads, the pool's reuse of the panels) is behind both top-n streams
        PFZ_HIP(hipStreamWaitEvent(ctx->stream, consumed[0], 0));
        if (pi >= 2) PFZ_HIP(hipStreamWaitEvent(ctx->stream, consumed[1], 0));
    }
    PFZ_HIP(hipGetLastError());
    return PFZ_OK;     // (the score panels go back to the pool: stream order keeps them alive until the kernels are done)
}

int pfz_dense_rescore_topn(pfz_ctx *ctx, const pfz_dense *from_exact, const pfz_dense *to_exact, const pfz_topn *candidates,
                           int32_t ntop, float lower_bound, pfz_topn *out)
{
    PFZ_REQUIRE(ctx && from_exact && to_exact && candidates && out, "pfz_dense_rescore_topn: NULL argument");
    PFZ_REQUIRE(from_exact->dtype == PFZ_DENSE_F32 && to_exact->dtype == PFZ_DENSE_F32,
                "pfz_dense_rescore_topn: the exact operands must be float32, got %s from-vectors and %s to-vectors",
                dense_dtype_name(from_exact->dtype), dense_dtype_name(to_exact->dtype));
    PFZ_REQUIRE(from_exact->dim == to_exact->dim, "pfz_dense_rescore_topn: from-vectors have %lld columns, to-vectors %lld",
                (long long)from_exact->dim, (long long)to_exact->dim);
    PFZ_REQUIRE(candidates != out, "pfz_dense_rescore_topn: the candidate table and the result are one buffer");
    PFZ_REQUIRE(candidates->n_rows >= from_exact->n, "pfz_dense_rescore_topn: the candidate table has %lld rows, the from-vectors %lld",
                (long long)candidates->n_rows, (long long)from_exact->n);
    const int32_t m = candidates->ntop;
    if (m > kRescoreMax) {
        set_error("pfz_dense_rescore_topn: %d candidates per row exceed the %d one pass ranks", m, kRescoreMax);
        return PFZ_ERR_UNSUPPORTED;
    }
    PFZ_REQUIRE(ntop >= 1 && ntop <= m, "pfz_dense_rescore_topn: ntop %d is outside 1 .. %d, the candidates per row", ntop, m);
    PFZ_REQUIRE(lower_bound == lower_bound, "pfz_dense_rescore_topn: lower_bound is NaN");
    PFZ_REQUIRE(out->n_rows >= from_exact->n && out->ntop == ntop, "pfz_dense_rescore_topn: result buffer is %lldx%d, need %lldx%d",
                (long long)out->n_rows, out->ntop, (long long)from_exact->n, ntop);
    const int64_t n_from = from_exact->n;
    if (n_from == 0) return PFZ_OK;
    PFZ_HIP(hipSetDevice(ctx->device));
    if (lower_bound < 0.f) lower_bound = 0.f;   // non-positive similarities are "no match" (_utils.py:122-123)
    {
        ProfScope ps(ctx, "k5_rescore_topn");
        auto *kernel = from_exact->ld <= kRescoreLds ? k5_rescore_topn<true> : k5_rescore_topn<false>;
        const dim3 grid((unsigned)std::min<int64_t>(n_from, (int64_t)1 << 20));
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, (const float *)from_exact->x, (const float *)from_exact->inv, n_from,
                           (const float *)to_exact->x, (const float *)to_exact->inv, to_exact->n, from_exact->ld,
                           (const int32_t *)candidates->idx, m, ntop, lower_bound, out->idx, out->val);
    }
    PFZ_HIP(hipGetLastError());
    return PFZ_OK;
}

int pfz_dense_rescore_topn_mixed(pfz_ctx *ctx, const pfz_dense *from_exact, const pfz_dense *to_coarse, const pfz_topn *candidates,
                                 int32_t ntop, float lower_bound, pfz_topn *out)
{
    PFZ_REQUIRE(ctx && from_exact && to_coarse && candidates && out, "pfz_dense_rescore_topn_mixed: NULL argument");
    PFZ_REQUIRE(from_exact->dtype == PFZ_DENSE_F32, "pfz_dense_rescore_topn_mixed: the from-vectors must be float32, got %s",
                dense_dtype_name(from_exact->dtype));
    const bool bits = to_coarse->dtype == PFZ_DENSE_B1;
    PFZ_REQUIRE(bits || to_coarse->dtype == PFZ_DENSE_I8,
                "pfz_dense_rescore_topn_mixed: the to-vectors must be int8 or binary, got %s (pfz_dense_rescore_topn is the entry for "
                "float32 to-vectors)", dense_dtype_name(to_coarse->dtype));
    PFZ_REQUIRE(!bits || from_exact->dim == to_coarse->dim,
                "pfz_dense_rescore_topn_mixed: from-vectors have %lld columns, to-vectors %lld bits (rows packed on the host count 8 "
                "bits per byte: float vectors whose width is not a multiple of 8 cannot be paired with them)",
                (long long)from_exact->dim, (long long)to_coarse->dim);
    PFZ_REQUIRE(from_exact->dim == to_coarse->dim, "pfz_dense_rescore_topn_mixed: from-vectors have %lld columns, to-vectors %lld",
                (long long)from_exact->dim, (long long)to_coarse->dim);
    PFZ_REQUIRE(!bits || from_exact->normalize == to_coarse->normalize,
                "pfz_dense_rescore_topn_mixed: the binary to-vectors were uploaded %s normalize, the from-vectors %s: the score is "
                "one or the other", to_coarse->normalize ? "with" : "without", from_exact->normalize ? "with" : "without");
    PFZ_REQUIRE(candidates != out, "pfz_dense_rescore_topn_mixed: the candidate table and the result are one buffer");
    PFZ_REQUIRE(candidates->n_rows >= from_exact->n,
                "pfz_dense_rescore_topn_mixed: the candidate table has %lld rows, the from-vectors %lld", (long long)candidates->n_rows,
                (long long)from_exact->n);
    const int32_t m = candidates->ntop;
    if (m > kRescoreMax) {
        set_error("pfz_dense_rescore_topn_mixed: %d candidates per row exceed the %d one pass ranks", m, kRescoreMax);
        return PFZ_ERR_UNSUPPORTED;
    }
    PFZ_REQUIRE(ntop >= 1 && ntop <= m, "pfz_dense_rescore_topn_mixed: ntop %d is outside 1 .. %d, the candidates per row", ntop, m);
    PFZ_REQUIRE(lower_bound == lower_bound, "pfz_dense_rescore_topn_mixed: lower_bound is NaN");
    PFZ_REQUIRE(out->n_rows >= from_exact->n && out->ntop == ntop, "pfz_dense_rescore_topn_mixed: result buffer is %lldx%d, need %lldx%d",
                (long long)out->n_rows, out->ntop, (long long)from_exact->n, ntop);
    const int64_t n_from = from_exact->n;
    if (n_from == 0) return PFZ_OK;
    PFZ_HIP(hipSetDevice(ctx->device));
    if (lower_bound < 0.f) lower_bound = 0.f;   // non-positive similarities are "no match" (_utils.py:122-123)
    {
        ProfScope ps(ctx, "k5_mixed_rescore");
        const bool lds = from_exact->ld <= kRescoreLds;
        auto *kernel = bits ? (lds ? k5_mixed_rescore<true, true> : k5_mixed_rescore<true, false>)
                            : (lds ? k5_mixed_rescore<false, true> : k5_mixed_rescore<false, false>);
        const int64_t pitch = bits ? to_coarse->ld / 8 : to_coarse->ld;      // bytes of a to-row
        const dim3 grid((unsigned)std::min<int64_t>(n_from, (int64_t)1 << 20));
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, (const float *)from_exact->x, (const float *)from_exact->inv, n_from,
                           from_exact->ld, (const unsigned char *)to_coarse->x, (const float *)to_coarse->inv, to_coarse->n, pitch,
                           to_coarse->dim, to_coarse->normalize, (const int32_t *)candidates->idx, m, ntop, lower_bound, out->idx,
                           out->val);
    }
    PFZ_HIP(hipGetLastError());
    return PFZ_OK;
}

static int dense_topn_host(pfz_ctx *ctx, const float *from_vec, int64_t n_from, const float *to_vec, int64_t n_to,
                           int64_t dim, int32_t ntop, float lower_bound, int32_t exclude_diag, int32_t normalize,
                           int32_t *out_idx, float *out_val)
{
    PFZ_REQUIRE(ctx && out_idx && out_val, "pfz_dense_cossim_topn_host: NULL argument");
    PFZ_REQUIRE(n_from >= 0 && n_to >= 0 && dim >= 1, "pfz_dense_cossim_topn_host: bad shape");
    if (n_from == 0) return PFZ_OK;
    PFZ_REQUIRE(from_vec && (n_to == 0 || to_vec), "pfz_dense_cossim_topn_host: NULL matrix");
    const bool same = to_vec == from_vec && n_to == n_from;
    pfz_dense *A = nullptr, *B = nullptr;
    pfz_topn *res = nullptr;
    int rc = pfz_dense_upload(ctx, from_vec, n_from, dim, normalize, &A);
    if (rc == PFZ_OK && !same) rc = pfz_dense_upload(ctx, to_vec, n_to, dim, normalize, &B);
    if (rc == PFZ_OK) rc = pfz_topn_alloc(ctx, n_from, ntop, &res);
    if (rc == PFZ_OK) rc = pfz_dense_topn(ctx, A, same ? A : B, ntop, lower_bound, exclude_diag, 0, res);
    if (rc == PFZ_OK) rc = pfz_topn_download(ctx, res, out_idx, out_val);
    pfz_topn_free(res);
    pfz_dense_free(B);
    pfz_dense_free(A);
    return rc;
}

int pfz_dense_cossim_topn_host(pfz_ctx *ctx, const float *from_vec, int64_t n_from, const float *to_vec, int64_t n_to,
                               int64_t dim, int32_t ntop, float lower_bound, int32_t exclude_diag, int32_t *out_idx,
                               float *out_val)
{
    return dense_topn_host(ctx, from_vec, n_from, to_vec, n_to, dim, ntop, lower_bound, exclude_diag, 1, out_idx, out_val);
}

int pfz_dense_dot_topn_host(pfz_ctx *ctx, const float *from_vec, int64_t n_from, const float *to_vec, int64_t n_to,
                            int64_t dim, int32_t ntop, float lower_bound, int32_t exclude_diag, int32_t *out_idx,
                            float *out_val)
{
    return dense_topn_host(ctx, from_vec, n_from, to_vec, n_to, dim, ntop, lower_bound, exclude_diag, 0, out_idx, out_val);
}

}  // extern "C"
