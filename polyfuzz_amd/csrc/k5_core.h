// What the dense kernels share: the operand handle, and the fp32 tile program's main loop -- k5_gemm_panel_pipe (k5_dense.hip)
// and the threshold kernels of K14 (k14_dense_join.hip) run the same loop and differ in what they do with the accumulators.
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

}  // namespace pfz
