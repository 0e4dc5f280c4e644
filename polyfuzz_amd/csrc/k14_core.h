// What the dense threshold kernels share -- K14 on fp32 operands (k14_dense_join.hip) and K22's search on 16-bit operands
// (k22_dense_join16.hip): the argument block, the workgroup -> tile deal, the end of a 64 x 64 wave corner (scores, hit mask, one
// atomic per half corner, append or unite), the cut of a call into launches and the float32 threshold.
#pragma once

#include "k5_core.h"
#include "k11_core.h"
#include "k12_core.h"

#include <algorithm>
#include <cmath>
#include <limits.h>

namespace pfz {

struct DenseJoinArgs {
    const void *A, *B;                 // [n_a][d], [n_b][d] values of the kernel's operand type (a self-join: the same matrix)
    const float *inv_a, *inv_b;        // 1 / ||row||
    int64_t n_a, n_b, d;               // d: the padded width, a whole number of k-chunks
    int32_t tiles_m, tiles_n;
    int32_t self;
    int32_t wg_base;                   // the number, in the call's 1-D deal, of this launch's first workgroup (k14_launch)
    float t32;
    int32_t hmax;                      // K23 (k23_core.h) only: a pair is a hit iff its Hamming distance is <= hmax; A, B: packed bits, d: bytes a row
    unsigned long long *state;         // [0] hits, [1] tiles executed, [2] 64 x 64 wave corners that held a hit (K23: the same three, a line apart, k23_core.h)
    uint64_t *keys;                    // join: [capacity] row << 32 | col, in the order the waves got there ...
    float *vals;                       // ... and the scores beside them (kSinkKeys: NULL, no score is kept; K23: the int32 distances)
    unsigned long long capacity;
    int32_t *parent;                   // components: [n_a] the forest (k12_core.h)
};

// The tile of this workgroup; false: there is none (beyond the edge, or below the diagonal of a self-join).  Blocks of BM x BN
// tiles are dealt round-robin to the 8 XCDs; a block's BM BN workgroups follow one another on its XCD, row tile fastest.  Two
// lists: the blocks column by column.  Self-join (BM == BN): the blocks (bi <= bj) of the upper triangle, numbered
// g = bj (bj + 1) / 2 + bi.
template <int BM, int BN>
__device__ inline bool k14_tile(const DenseJoinArgs &P, int *tm, int *tn)
{
    constexpr unsigned kPos = BM * BN;
    const int w = P.wg_base + (int)blockIdx.x, xcd = w & 7, idx = w >> 3;      // (wg_base is a multiple of 8: the XCD is blockIdx's)
    const int pos = (int)((unsigned)idx % kPos), g = (int)((unsigned)idx / kPos) * 8 + xcd;
    int bi, bj;
    if (P.self) {
        bj = (int)((sqrtf(8.f * (float)g + 1.f) - 1.f) * 0.5f);      // (a guess: float32 is a few blocks off at most)
        while ((int64_t)bj * (bj + 1) / 2 > g) --bj;
        while ((int64_t)(bj + 1) * (bj + 2) / 2 <= g) ++bj;
        bi = g - (int)((int64_t)bj * (bj + 1) / 2);
    }
    else {
        const int bm = (P.tiles_m + BM - 1) / BM;
        bi = g % bm;
        bj = g / bm;
    }
    *tm = bi * BM + (int)((unsigned)pos % BM);
    *tn = bj * BN + (int)((unsigned)pos / BM);
    return *tm < P.tiles_m && *tn < P.tiles_n && (!P.self || *tn >= *tm);
}

// inclusive prefix sum over the lanes of a wave
__device__ inline int wave_scan_i32(int v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// what a corner does with its hits: key and score appended (K14's join, K22's plain 16-bit join), the two positions united (K14's
// components), or the key alone appended, the score too where P.vals is not NULL (K22's search)
enum DenseSink { kSinkJoin, kSinkUnite, kSinkKeys };

// The end of one 64 x 64 wave corner.  acc: 2 x 2 accumulators of a 32 x 32 MFMA, accumulator r of lane l = row
// (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31 of its 32 x 32 (tile_epilogue of K5); rbase / cbase: the lane's first row and
// column, corner origin + 4 (l >> 5) and + (l & 31).  score = acc * inv_a[row] * inv_b[col], in that order: the float32 the panel
// would hold, bit for bit; hit iff score >= t32, never beyond n_a / n_b, in a self-join only col > row.
// The corner in two halves of 32 rows (the accumulator pairs i = 0, 1): the half's 32 scores of the lane, its hits as a mask
// (bit 16 j + r), and -- only where some lane of the wave has one -- ONE atomic for all of them (K11's KeyAppend, with a
// prefix sum in place of the ballot's popcount: a lane may hold several).  A corner without a hit touches no memory.
template <DenseSink kSink>
__device__ __forceinline__ void dense_corner_end(const f32x16 (&acc)[2][2], int64_t rbase, int64_t cbase, const DenseJoinArgs &P, int lane)
{
    const bool self = P.self != 0;
    float sb[2];
    bool col_ok[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        col_ok[j] = cbase + 32 * j < P.n_b;
        sb[j] = col_ok[j] ? P.inv_b[cbase + 32 * j] : 0.f;
    }
    bool corner_hit = false;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        float v[2][16];
        uint32_t mask = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = rbase + i * 32 + (r & 3) + 8 * (r >> 2);
            const bool ok = row < P.n_a;
            const float f = ok ? P.inv_a[row] : 0.f;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                v[j][r] = acc[i][j][r] * f * sb[j];
                const bool hit = ok && col_ok[j] && v[j][r] >= P.t32 && (!self || cbase + 32 * j > row);
                mask |= (uint32_t)hit << (16 * j + r);
            }
        }
        if (!__any(mask != 0)) continue;
        corner_hit = true;
        const int mine = __popc(mask), upto = wave_scan_i32(mine, lane), all = __shfl(upto, 63, 64);
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(P.state, (unsigned long long)all);
        if (kSink == kSinkUnite) {
            while (mask) {
                const int q = __builtin_ctz(mask), r = q & 15;
                mask &= mask - 1;
                uf_unite<UfDeviceOps>(P.parent, (int32_t)(rbase + i * 32 + (r & 3) + 8 * (r >> 2)), (int32_t)(cbase + 32 * (q >> 4)));
            }
            continue;
        }
        base = __shfl(base, 0, 64);
        unsigned long long pos = base + (unsigned long long)(upto - mine);
        // The two halves of a key start from values the compiler cannot tie to the 64-bit rows of the loop above (an empty asm):
        // otherwise it keeps all 32 row numbers of the half in registers ahead of the stores, work that every half with a hit paid
        // for its one or two hits (K14 at t = 0.8).  So a key costs one add, inside its hit's own block.
        uint32_t rlo = (uint32_t)rbase + i * 32, clo = (uint32_t)cbase;
        asm volatile("" : "+v"(rlo), "+v"(clo));
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if ((mask >> (16 * j + r)) & 1) {
                    if (pos < P.capacity) {
                        P.keys[pos] = (uint64_t)(rlo + ((r & 3) + 8 * (r >> 2))) << 32 | (uint64_t)(clo + 32 * j);
                        if (kSink == kSinkJoin || P.vals) P.vals[pos] = v[j][r];
                    }
                    ++pos;
                }
    }
    if (corner_hit && lane == 0) atomicAdd(P.state + 2, 1ull);
}

// the smallest float32 >= t (t in [0, 1])
inline float threshold32(double t)
{
    float f = (float)t;
    if ((double)f < t) f = nextafterf(f, INFINITY);
    return f;
}

// The grid of a call whose workgroup tiles have `tile` rows and columns and are dealt in blocks of bm x bn (a self-join: bm ==
// bn), and its argument block's tile counts; PFZ_ERR_UNSUPPORTED beyond 2^31 tiles
inline int dense_join_grid(const char *who, DenseJoinArgs *P, int tile, int bm_edge, int bn_edge, int64_t *grid)
{
    const int64_t tm = (P->n_a + tile - 1) / tile, tn = (P->n_b + tile - 1) / tile;
    const int64_t bm = (tm + bm_edge - 1) / bm_edge, bn = (tn + bn_edge - 1) / bn_edge;
    const int64_t tiles = P->self ? tm * (tm + 1) / 2 : tm * tn, blocks = P->self ? bm * (bm + 1) / 2 : bm * bn;
    *grid = (blocks + 7) / 8 * 8 * bm_edge * bn_edge;
    if (tiles > ((int64_t)1 << 31) || *grid > (int64_t)INT_MAX) {
        set_error("%s: %lld x %lld rows are %lld tiles of %d x %d, more than the 2^31 one call launches", who, (long long)P->n_a,
                  (long long)P->n_b, (long long)tiles, tile, tile);
        return PFZ_ERR_UNSUPPORTED;
    }
    P->tiles_m = (int32_t)tm;
    P->tiles_n = (int32_t)tn;
    return PFZ_OK;
}

// One launch takes fewer than 2^32 threads (hipErrorInvalidConfiguration beyond): 2^24 workgroups of 256, which K14's self-join of
// 740 000 rows exceeds, or 2^23 of 512.  So the call's deal of `grid` workgroups of `threads` is cut into launches of whole 8-block
// rounds (`round` = 8 bm bn workgroups) that stay below that; they follow one another on the context's stream and share the
// argument block but for wg_base.
inline int k14_launch(pfz_ctx *ctx, void (*kernel)(DenseJoinArgs), DenseJoinArgs P, int64_t grid, int threads, int round)
{
    const int64_t launch_max = ((((int64_t)1 << 32) / threads - 1) / round) * round;
    for (int64_t base = 0; base < grid; base += launch_max) {
        P.wg_base = (int32_t)base;
        hipLaunchKernelGGL(kernel, dim3((unsigned)std::min(launch_max, grid - base)), dim3(threads), 0, ctx->stream, P);
        PFZ_HIP(hipGetLastError());
    }
    return PFZ_OK;
}

}  // namespace pfz
