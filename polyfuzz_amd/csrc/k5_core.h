// What the dense kernels share: the operand handle; the fp32 tile program's main loop -- k5_gemm_panel_pipe (k5_dense.hip)
// and the threshold kernels of K14 (k14_dense_join.hip) run the same loop and differ in what they do with the accumulators --;
// the operand traits and the main loop of the 16-bit / 8-bit tile program -- k5_gemm16_panel, k5_gemm8_panel and K22's threshold
// search (k22_dense_join16.hip) --; the XOR / popcount main loop of the 1-bit tile program -- k5_hamming_panel and K23's threshold
// kernels (k23_hamming_join.hip) --; and the exact float64-summed score of one pair of fp32 rows (k5_rescore_topn, K22's rescoring).
#pragma once

#include "pfz_internal.h"

struct pfz_dense {
    pfz_ctx *ctx = nullptr;
    int64_t n = 0, dim = 0;
    // dim rounded up to a whole k-chunk of the type (128 B: 32 / 64 / 128 values), the extra columns zero; 1-bit rows: dim (bits)
    // rounded up to whole 16-byte pieces, in bits
    int64_t ld = 0;
    int32_t normalize = 1;
    int32_t dtype = PFZ_DENSE_F32;
    // device [n][ld] row-major values of `dtype`: float, float16 / bfloat16 bits, int8 (given or quantised per row), or bits in
    // np.packbits order (given or packed from the signs of float32 values)
    void *x = nullptr;
    // device [n], the factor of a row in the epilogue: 1 / ||row|| of the stored values; with normalize == 0 it is 1, or for
    // int8 rows quantised from float32 the row's scale max |x| / 127; 1-bit rows: 1 (the Hamming score has no row factor)
    float *inv = nullptr;
};

namespace pfz {

inline const char *dense_dtype_name(int32_t dtype)
{
    return dtype == PFZ_DENSE_F16 ? "float16" : dtype == PFZ_DENSE_BF16 ? "bfloat16" : dtype == PFZ_DENSE_I8 ? "int8"
           : dtype == PFZ_DENSE_B1 ? "binary" : "float32";
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTile = 128;   // workgroup tile (rows of A x rows of B)

__device__ inline float f4c(const float4 &v, int s) { return s == 0 ? v.x : s == 1 ? v.y : s == 2 ? v.z : v.w; }

// The main loop of the tile program for d % 32 == 0 (embedding widths: 128 ... 768 ... 4096), software-pipelined: the operands of
// chunk c + 2 travel from HBM / L2 into registers and those of chunk c + 1 from registers into the other LDS buffer while the
// MFMAs of chunk c run out of LDS; one barrier per chunk.  It adds the 128 x 128 tile A[row0 ..] . B[col0 ..]^T to acc: wave
// (wm, wn) holds its 64 x 64 corner as 2 x 2 accumulators of v_mfma_f32_32x32x2_f32, accumulator r of lane l = row
// (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31.  Rows beyond the matrix edge (a1, n_b) are clamped to the last row (the caller
// does not use their products), so the loop has no edge tests.  All 256 threads of the workgroup call it (it has barriers).  Its
// shape is what the counters and what-if builds of its predecessor (round 2's first pipelined kernel, removed; DESIGN.md section
// 4 keeps the numbers) asked for:
//  * LDS rows of 36 floats: operands staged with ds_write_b128, MFMA fragments read with ds_read_b128 -- lane (r, h)
//    takes the four floats k = 8t + 4h .. + 3 of row r, and MFMA step s of sub-step t multiplies the k-pairs
//    {8t + s, 8t + 4 + s} (A and B use the same assignment, so the sum is the same dot product in another order).
//    24 LDS instructions per wave and k-chunk instead of 48; both access patterns are conflict-free
//    (row pitch 36 = 4 (9 r mod 16) banks: the 16 lanes of a b128 group hit 16 distinct bank quads).
//  * the global loads of chunk c + 2 and the LDS stores of chunk c + 1 are spread over the chunk, one operand pair
//    per group of eight MFMAs (eight loads issued back to back kept the wave out of the matrix pipe for ~300 cycles
//    per chunk: 8 % of the GEMM, with L2-hot loads just the same); addresses are a wave-uniform base + a 32-bit lane
//    offset, so a load costs no vector ALU work.
__device__ __forceinline__ void k5_tile_loop(const void *__restrict__ A, const void *__restrict__ B, int64_t row0, int64_t col0,
                                             int64_t a1, int64_t n_b, int64_t d, int tid, int lane, int wm, int wn,
                                             f32x16 (&acc)[2][2])
{
    constexpr int BK = 32, LD = 36, NP = 4;
    __shared__ __attribute__((aligned(16))) float As[2][kTile * LD];
    __shared__ __attribute__((aligned(16))) float Bs[2][kTile * LD];
    const int lr = tid >> 3, lk = (tid & 7) * 4;          // staging: 8 threads per tile row, 32 rows per pass
    // buffer loads: descriptor = the tile's first operand row (wave-uniform), 32-bit lane offset, scalar k offset
    const __amdgpu_buffer_rsrc_t resA = __builtin_amdgcn_make_buffer_rsrc((void *)((const float *)A + row0 * d), 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t resB = __builtin_amdgcn_make_buffer_rsrc((void *)((const float *)B + col0 * d), 0, 0x7fffffff, 0x00020000);
    uint32_t offA[NP], offB[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {        // rows beyond the edge are clamped to the last row (their products are not stored)
        offA[p] = (uint32_t)((min(row0 + lr + p * 32, a1 - 1) - row0) * d + lk) * 4u;
        offB[p] = (uint32_t)((min(col0 + lr + p * 32, n_b - 1) - col0) * d + lk) * 4u;
    }
    u32x4 ra[NP], rb[NP];
    auto load = [&](int p, int k) {
        ra[p] = __builtin_amdgcn_raw_buffer_load_b128(resA, offA[p], k * 4, 0);
        rb[p] = __builtin_amdgcn_raw_buffer_load_b128(resB, offB[p], k * 4, 0);
    };
    auto stage = [&](int p, int buf) {
        *(u32x4 *)(As[buf] + (lr + p * 32) * LD + lk) = ra[p];
        *(u32x4 *)(Bs[buf] + (lr + p * 32) * LD + lk) = rb[p];
    };
#pragma unroll
    for (int p = 0; p < NP; ++p) load(p, 0);
#pragma unroll
    for (int p = 0; p < NP; ++p) stage(p, 0);
    const int dk = (int)d;
#pragma unroll
    for (int p = 0; p < NP; ++p) load(p, min(BK, dk - BK));
    __syncthreads();

    const int frag_off = (lane & 31) * LD + 4 * (lane >> 5);
    int cur = 0;
    for (int k0 = 0; k0 < dk; k0 += BK) {
        const int k2 = min(k0 + 2 * BK, dk - BK);      // (the last two chunks re-fetch the last one: no branches in the loop)
        const float *ap = As[cur] + wm * LD + frag_off, *bp = Bs[cur] + wn * LD + frag_off;
        auto frag = [&](int t, float4 (&a)[2], float4 (&b)[2]) {
            a[0] = *(const float4 *)(ap + 8 * t);
            a[1] = *(const float4 *)(ap + 32 * LD + 8 * t);
            b[0] = *(const float4 *)(bp + 8 * t);
            b[1] = *(const float4 *)(bp + 32 * LD + 8 * t);
        };
        auto mfma8 = [&](const float4 (&a)[2], const float4 (&b)[2], int s0) {
#pragma unroll
            for (int s = s0; s < s0 + 2; ++s)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(f4c(a[i], s), f4c(b[j], s), acc[i][j], 0, 0, 0);
        };
        // one operand pair per group of eight MFMAs: groups 0..3 store chunk c + 1 (in registers since the previous
        // chunk) to the other LDS buffer, groups 4..7 fetch chunk c + 2 into the registers just freed
        auto item = [&](int grp) {
            if (grp < 4) stage(grp, cur ^ 1);
            else load(grp - 4, k2);
        };
        float4 fa0[2], fb0[2], fa1[2], fb1[2];
        frag(0, fa0, fb0);
#pragma unroll
        for (int t = 0; t < 4; t += 2) {
            frag(t + 1, fa1, fb1);                 // fragments are read one sub-step (16 MFMAs) ahead
            __builtin_amdgcn_sched_barrier(0);
            mfma8(fa0, fb0, 0);
            item(2 * t);
            __builtin_amdgcn_sched_barrier(0);
            mfma8(fa0, fb0, 2);
            item(2 * t + 1);
            if (t + 2 < 4) frag(t + 2, fa0, fb0);
            __builtin_amdgcn_sched_barrier(0);
            mfma8(fa1, fb1, 0);
            item(2 * t + 2);
            __builtin_amdgcn_sched_barrier(0);
            mfma8(fa1, fb1, 2);
            item(2 * t + 3);
        }
        __syncthreads();
        cur ^= 1;
    }
}

// ---- 16-bit operands (float16 / bfloat16 embeddings) ----------------------------------------------------------------
// The vectors are stored as their 16 bits; what differs between the two types is how a value widens and rounds and which
// MFMA multiplies it.  The product of two such values is exact in fp32 and the MFMA sums in fp32: against the 16-bit
// vectors as given the scores are as good as the fp32 kernel's.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

// An operand trait: the stored value (store_t, kBytes) and how it widens; for the tile program (k5_tile_loop16) also the
// accumulator type and the MFMA that takes one 16-byte fragment of each operand.  f32 has the fp32 tile program of its own.
struct f32 {
    typedef float store_t;
    static constexpr int kBytes = 4;
    __device__ static inline float widen(float v) { return v; }
};
struct f16 {
    typedef uint16_t store_t;
    typedef f32x16 acc_t;
    static constexpr int kBytes = 2;
    __device__ static inline float widen(uint16_t b) { return (float)__builtin_bit_cast(_Float16, b); }
    __device__ static inline uint16_t narrow(float x) { return __builtin_bit_cast(uint16_t, (_Float16)x); }   // round to nearest even
    __device__ static inline f32x16 mfma(const u32x4 &a, const u32x4 &b, const f32x16 &c)
    {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    }
};
struct bf16 {
    typedef uint16_t store_t;
    typedef f32x16 acc_t;
    static constexpr int kBytes = 2;
    __device__ static inline float widen(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }
    __device__ static inline uint16_t narrow(float x)
    {
        const uint32_t u = __float_as_uint(x);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);      // NaN stays NaN
        return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);                       // round to nearest even
    }
    __device__ static inline f32x16 mfma(const u32x4 &a, const u32x4 &b, const f32x16 &c)
    {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
};
// int8: a fragment is 16 consecutive values of a row, one MFMA covers k = 32.  Which k of the 32 a lane's 16 values stand for
// does not matter here: A and B are read with the same assignment, so every step sums the same 32 products, and integer
// addition has no order (tests/test_dense8_gpu.py holds the dot products bit for bit).
struct i8 {
    typedef int8_t store_t;
    typedef i32x16 acc_t;
    static constexpr int kBytes = 1;
    __device__ static inline float widen(int8_t q) { return (float)q; }
    __device__ static inline i32x16 mfma(const u32x4 &a, const u32x4 &b, const i32x16 &c)
    {
        return __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_bit_cast(i32x4, a), __builtin_bit_cast(i32x4, b), c, 0, 0, 0);
    }
};

constexpr int kTile16 = 256; // workgroup tile of the 16-bit (and 8-bit) tile program
constexpr int kChunkBytes = 128;   // bytes of a row a tile program stages per step: 32 floats, 64 16-bit or 128 int8 values

// The main loop of the tile program for 16-bit and 8-bit operands: v_mfma_f32_32x32x16_f16 / _bf16 / v_mfma_i32_32x32x32_i8;
// k5_gemm16_panel / k5_gemm8_panel (k5_dense.hip) and the 16-bit threshold search of K22 (k22_dense_join16.hip) run it and
// differ in what they do with the accumulators.  Lane (r = l & 31, h = l >> 5) holds 16 consecutive bytes of row r of A and
// the same of B -- for 16-bit values A[row r][k = 8 h .. 8 h + 7]: both matrices are row-major [n][d] and the product is
// A . B^T, so every fragment is one ds_read_b128, no transposed read.  A k-chunk is 128 B of a row (64 16-bit values, 128 int8
// values): what 32 floats are, so the staging (8 lanes x 16 B per row), the LDS image (rows of 144 B: ds_write_b128 and
// ds_read_b128 conflict-free, see the fp32 program) and the software pipeline (chunk c + 2 into registers, chunk c + 1 into
// the other LDS buffer, one barrier per chunk, clamped edge rows) are those of k5_tile_loop.  What changes is the MFMA
// count -- a fragment feeds ONE instruction instead of four -- and with it the balance: at 128 x 128 tiles with 64 x 64 per
// wave, the MFMAs, the LDS (one ds_read_b128 per MFMA) and the CU's 64 B / clk of global loads each need the same 1024 cycles
// per chunk and CU, and the program ran at 0.23 of the MFMA peak (measured).  So the tile is 256 x 256:
// 8 waves of 128 x 64 (eight accumulators), 6 fragment reads per 8 MFMAs, half the LDS stores and global bytes per flop:
// 0.28 - 0.29.  147 456 B of LDS and 512 threads: ONE workgroup per CU, two waves per SIMD.
// It adds the 256 x 256 tile A[row0 ..] . B[col0 ..]^T to acc: wave (vr, vc, wn) owns rows 128 vr .., columns 128 vc + wn ..
// of the tile, 128 x 64, as acc[half][i][j] -- two 64 x 64 corners laid out as k5_tile_loop's.  d: the row pitch in values, a
// multiple of the k-chunk.  All 512 threads of the workgroup call it (it has barriers).
template <typename T>
__device__ __forceinline__ void k5_tile_loop16(const void *__restrict__ A, const void *__restrict__ B, int64_t row0, int64_t col0,
                                               int64_t a1, int64_t n_b, int64_t d, int tid, int lane, int vr, int vc, int wn,
                                               typename T::acc_t (&acc)[2][2][2])
{
    constexpr int CB = kChunkBytes, LD = 144, NP = 4;       // LD: LDS row pitch in bytes
    __shared__ __attribute__((aligned(16))) unsigned char As[2][kTile16 * LD];
    __shared__ __attribute__((aligned(16))) unsigned char Bs[2][kTile16 * LD];
    const int lr = tid >> 3, lb = (tid & 7) * 16;         // staging: 8 threads per tile row, 64 rows per pass
    const int64_t pitch = d * T::kBytes;                  // bytes per operand row
    const __amdgpu_buffer_rsrc_t resA =
        __builtin_amdgcn_make_buffer_rsrc((void *)((const unsigned char *)A + row0 * pitch), 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t resB =
        __builtin_amdgcn_make_buffer_rsrc((void *)((const unsigned char *)B + col0 * pitch), 0, 0x7fffffff, 0x00020000);
    uint32_t offA[NP], offB[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {        // rows beyond the edge are clamped to the last row (their products are not stored)
        offA[p] = (uint32_t)((min(row0 + lr + p * 64, a1 - 1) - row0) * pitch + lb);
        offB[p] = (uint32_t)((min(col0 + lr + p * 64, n_b - 1) - col0) * pitch + lb);
    }
    u32x4 ra[NP], rb[NP];
    auto load = [&](int p, int kb) {      // kb: byte offset of the chunk in a row
        ra[p] = __builtin_amdgcn_raw_buffer_load_b128(resA, offA[p], kb, 0);
        rb[p] = __builtin_amdgcn_raw_buffer_load_b128(resB, offB[p], kb, 0);
    };
    auto stage = [&](int p, int buf) {
        *(u32x4 *)(As[buf] + (lr + p * 64) * LD + lb) = ra[p];
        *(u32x4 *)(Bs[buf] + (lr + p * 64) * LD + lb) = rb[p];
    };
#pragma unroll
    for (int p = 0; p < NP; ++p) load(p, 0);
#pragma unroll
    for (int p = 0; p < NP; ++p) stage(p, 0);
    const int dk = (int)pitch;
#pragma unroll
    for (int p = 0; p < NP; ++p) load(p, min(CB, dk - CB));
    __syncthreads();

    const int frag_off = (lane & 31) * LD + 16 * (lane >> 5);
    int cur = 0;
    for (int k0 = 0; k0 < dk; k0 += CB) {
        const int k2 = min(k0 + 2 * CB, dk - CB);      // (the last two chunks re-fetch the last one: no branches in the loop)
        const unsigned char *ap = As[cur] + vr * 128 * LD + frag_off, *bp = Bs[cur] + (vc * 128 + wn) * LD + frag_off;
        auto frag = [&](int s, u32x4 (&a)[4], u32x4 (&b)[2]) {      // MFMA step s: bytes 32 s + 16 h .. + 15 of the chunk
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = *(const u32x4 *)(ap + i * 32 * LD + 32 * s);
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = *(const u32x4 *)(bp + j * 32 * LD + 32 * s);
        };
        auto mfma4 = [&](const u32x4 (&a)[4], const u32x4 (&b)[2], int h) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[h][i][j] = T::mfma(a[2 * h + i], b[j], acc[h][i][j]);
        };
        // one operand pair per four MFMAs: items 0..3 store chunk c + 1 (in registers since the previous chunk) to the other
        // LDS buffer, items 4..7 fetch chunk c + 2 into the registers just freed
        auto item = [&](int it) {
            if (it < 4) stage(it, cur ^ 1);
            else load(it - 4, k2);
        };
        u32x4 fa[2][4], fb[2][2];
        frag(0, fa[0], fb[0]);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if (s + 1 < 4) frag(s + 1, fa[(s + 1) & 1], fb[(s + 1) & 1]);      // fragments are read one step (8 MFMAs) ahead
            __builtin_amdgcn_sched_barrier(0);
            mfma4(fa[s & 1], fb[s & 1], 0);
            item(2 * s);
            __builtin_amdgcn_sched_barrier(0);
            mfma4(fa[s & 1], fb[s & 1], 1);
            item(2 * s + 1);
        }
        __syncthreads();
        cur ^= 1;
    }
}

// The main loop of the tile program for two 1-bit operands, on the vector ALU (there is no matrix instruction for XOR /
// popcount): k5_hamming_panel (k5_dense.hip) and the threshold kernels of K23 (k23_hamming_join.hip) run it and differ in what
// they do with the counts.  A workgroup of 256 threads owns a 128 x 128 tile.  Both row sets are staged in LDS as 32-bit words,
// a chunk of 128 B of every row at a time (a whole row at dim <= 1024), rows of 36 words (ds_write_b128 / ds_read_b128, see the
// fp32 program); rows beyond the edge (a1, n_b) are clamped to the last row (the caller does not use their counts).  Thread
// (tx = tid & 31, ty = tid >> 5) has the differing bits of row row0 + ty + 8 i and column col0 + tx + 32 j ADDED to h[i][j] (the
// caller clears h, as k5_tile_loop's callers clear acc: cleared in here, k5_hamming_panel took 185 registers instead of 122): per 16
// bytes of k it reads four B pieces, and for each of its 16 rows one A piece (two addresses per wave: a broadcast) that meets
// all four -- 20 LDS reads for 256 XORs and 256 v_bcnt_u32_b32, which add the bit count into the running count.  The words of a
// row are XORed in whatever order they lie in: both sides lie the same way.  pitch: bytes per operand row, whole 16-byte pieces.
// All 256 threads of the workgroup call it (it has barriers); 36 864 B of LDS.
__device__ __forceinline__ void k5_hamming_loop(const void *__restrict__ A, const void *__restrict__ B, int64_t row0, int64_t col0,
                                                int64_t a1, int64_t n_b, int64_t pitch, int tid, int tx, int ty, int (&h)[16][4])
{
    constexpr int LD = 36, NP = 4;                       // LDS row pitch in words; staging passes of 32 rows
    __shared__ __attribute__((aligned(16))) uint32_t As[kTile * LD];
    __shared__ __attribute__((aligned(16))) uint32_t Bs[kTile * LD];
    const int lr = tid >> 3, lb = (tid & 7) * 16;         // staging: 8 threads per tile row, 32 rows per pass
    const unsigned char *pa[NP], *pb[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {        // rows beyond the edge are clamped to the last row (their counts are not stored)
        pa[p] = (const unsigned char *)A + min(row0 + lr + p * 32, a1 - 1) * pitch + lb;
        pb[p] = (const unsigned char *)B + min(col0 + lr + p * 32, n_b - 1) * pitch + lb;
    }
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    for (int64_t kb = 0; kb < pitch; kb += kChunkBytes) {
        const bool in = kb + lb < pitch;                  // (a 16-byte piece is inside the row or beyond it: pitch is whole pieces)
        u32x4 ra[NP], rb[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            ra[p] = in ? *(const u32x4 *)(pa[p] + kb) : zero4;
            rb[p] = in ? *(const u32x4 *)(pb[p] + kb) : zero4;
        }
        if (kb) __syncthreads();                          // the chunk before has been counted
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            *(u32x4 *)(As + (lr + p * 32) * LD + lb / 4) = ra[p];
            *(u32x4 *)(Bs + (lr + p * 32) * LD + lb / 4) = rb[p];
        }
        __syncthreads();
        const int pieces = (int)(min((int64_t)kChunkBytes, pitch - kb) / 16);
        for (int q = 0; q < pieces; ++q) {
            u32x4 b[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = *(const u32x4 *)(Bs + (tx + 32 * j) * LD + 4 * q);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const u32x4 a = *(const u32x4 *)(As + (ty + 8 * i) * LD + 4 * q);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    h[i][j] += __builtin_popcount(a.x ^ b[j].x) + __builtin_popcount(a.y ^ b[j].y) +
                               __builtin_popcount(a.z ^ b[j].z) + __builtin_popcount(a.w ^ b[j].w);
            }
        }
    }
}

// The exact score of one pair of fp32 rows, as one wave computes it (k5_rescore_topn of k5_dense.hip, k22_rescore_kernel of
// k22_dense_join16.hip): fa fb sum_k xa[k] xb[k].  The sum is float64 -- the product of two floats is exact in it -- in ONE
// order: lane l adds its elements k = 4 l + 256 c + {0, 1, 2, 3} in ascending order (fma), then a xor butterfly over the lanes
// (commutative steps: every lane ends with the same bits), and the product with the two factors is rounded to fp32 once.  The
// products commute, so the score is symmetric in its two rows.  ld: a multiple of 32 floats (a float4 never crosses the end);
// xa may point into LDS.  All 64 lanes call it and every lane returns the same value.
__device__ __forceinline__ float k5_pair_score(const float *xa, const float *xb, int64_t ld, double fa, double fb, int lane)
{
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    double acc = 0.0;
    for (int64_t k0 = 0; k0 < ld; k0 += 1024) {      // four 1 KiB loads of each row in flight per wave
        float4 a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t k = k0 + u * 256 + lane * 4;
            const bool in = k < ld;
            b[u] = in ? *(const float4 *)(xb + k) : zero;
            a[u] = in ? *(const float4 *)(xa + k) : zero;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc = fma((double)a[u].x, (double)b[u].x, acc);
            acc = fma((double)a[u].y, (double)b[u].y, acc);
            acc = fma((double)a[u].z, (double)b[u].z, acc);
            acc = fma((double)a[u].w, (double)b[u].w, acc);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
    return (float)(fa * fb * acc);
}

}  // namespace pfz
