// K23's share of the Hamming tile program: the end of a 128 x 128 tile of bit counts (k5_hamming_loop of k5_core.h) under a
// distance cutoff, the layout of the call's device counters, and the cutoff that stands for a similarity.  The argument block, the tile deal, the sinks and the cut into
// launches are K14's (k14_core.h); DenseJoinArgs carries the integer cutoff in `hmax` and the row pitch in bytes in `d`.
#pragma once

#include "k14_core.h"

namespace pfz {

// K23's device words: K14's three -- hits, tiles executed, waves that held a hit -- and the components' root count, each on a
// 256-byte line of its own.  Side by side in one line, as K14 keeps them, the tile counter's and the hit-wave counter's atomics
// queue behind the reservations at one address's rate, and K23's tiles are short enough to show it: 100 000 x 100 000 codes of 64
// bits with a hit in a quarter of the waves took 21.0 ms, with the lines apart 8.8 ms.
constexpr int kK23Line = 32;      // in 64-bit words
enum { kK23Hits = 0, kK23Tiles = kK23Line, kK23HitWaves = 2 * kK23Line, kK23Roots = 3 * kK23Line, kK23Words = 4 * kK23Line };

// The end of one tile.  h: the 16 x 4 counts of thread (tx, ty), h[i][j] = row row0 + ty + 8 i, column col0 + tx + 32 j.  A pair is
// a hit iff h <= P.hmax, never beyond n_a / n_b (those rows are clamped copies of the last one), in a self-join only col > row.
// The lane's hits are a 64-bit mask, bit 4 i + j.  A wave covers 32 rows x 128 columns; one without a hit touches no memory.
// Otherwise ONE atomic reserves room for all the wave's hits (a prefix sum over the lanes' popcounts, as dense_corner_end), and
//   join:        each hit goes out as key = row << 32 | col with h as the 32-bit payload beside it -- while there is room: hits
//                beyond the capacity are counted, never written;
//   components:  each hit unites its two positions in K12's forest and nothing is stored.
// Everything inside the tile is 32-bit: rlim / clim are the rows and columns of the tile inside the matrices, diag = col0 - row0
// (a self-join launches only tiles with col0 >= row0, and positions are below 2^31).
template <DenseSink kSink>
__device__ __forceinline__ void k23_tile_end(const int (&h)[16][4], int64_t row0, int64_t col0, int tx, int ty, const DenseJoinArgs &P, int lane)
{
    static_assert(kSink == kSinkJoin || kSink == kSinkUnite, "K23 appends key and distance, or unites");
    const int rlim = (int)min((int64_t)kTile, P.n_a - row0), clim = (int)min((int64_t)kTile, P.n_b - col0);
    const bool self = P.self != 0;
    const int diag = self ? (int)(col0 - row0) : kTile;      // (two lists: tx + 32 j + 128 > ty + 8 i always)
    const int hmax = P.hmax;
    uint64_t mask = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool hit = h[i][j] <= hmax && ty + 8 * i < rlim && tx + 32 * j < clim && tx + 32 * j + diag > ty + 8 * i;
            mask |= (uint64_t)hit << (4 * i + j);
        }
    if (!__any(mask != 0)) return;
    const int mine = __popcll(mask), upto = wave_scan_i32(mine, lane), all = __shfl(upto, 63, 64);
    unsigned long long base = 0;
    if (lane == 0) {
        base = atomicAdd(P.state + kK23Hits, (unsigned long long)all);
        atomicAdd(P.state + kK23HitWaves, 1ull);
    }
    if (kSink == kSinkUnite) {
        const int32_t r = (int32_t)row0 + ty, c = (int32_t)col0 + tx;
        while (mask) {
            const int q = __builtin_ctzll(mask);
            mask &= mask - 1;
            uf_unite<UfDeviceOps>(P.parent, r + 8 * (q >> 2), c + 32 * (q & 3));
        }
        return;
    }
    base = __shfl(base, 0, 64);
    unsigned long long pos = base + (unsigned long long)(upto - mine);
    uint32_t rlo = (uint32_t)row0 + ty, clo = (uint32_t)col0 + tx;
    asm volatile("" : "+v"(rlo), "+v"(clo));      // (as dense_corner_end: a key costs one add inside its hit's own block)
    int32_t *dist = (int32_t *)P.vals;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (!((mask >> (4 * i)) & 15)) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((mask >> (4 * i + j)) & 1) {
                if (pos < P.capacity) {
                    P.keys[pos] = (uint64_t)(rlo + 8 * i) << 32 | (uint64_t)(clo + 32 * j);
                    dist[pos] = h[i][j];
                }
                ++pos;
            }
    }
}

// The score Embeddings.match reports for two binary codes of dim_bits bits that differ in h: float(dim - 2 h) / float(dim), one
// correctly rounded fp32 division (k5_hamming_panel's, bit for bit).  dim_bits < 2^24: both operands are exact.
inline float hamming_score32(int64_t dim_bits, int64_t h) { return (float)(dim_bits - 2 * h) / (float)dim_bits; }

// The largest h in [0, dim_bits] whose score, compared as K14 compares (float64, equal is kept), is >= t; -1: none.  The score
// falls (weakly) as h grows, so the rule itself is evaluated along a bisection -- no closed form: floor((1 - t) / 2 * d) is wrong
// in both directions (d = 40: t = 0.8 -> 4, not 3; t = 0.7 -> 5, not 6).
inline int64_t hamming_cutoff(int64_t dim_bits, double t)
{
    if (!((double)hamming_score32(dim_bits, 0) >= t)) return -1;
    int64_t lo = 0, hi = dim_bits;      // lo passes; the answer is in [lo, hi]
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if ((double)hamming_score32(dim_bits, mid) >= t) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// The two runs behind pfz_hamming_join / pfz_hamming_components (k23_hamming_join.hip), arguments checked by the caller: K24's
// entries hand a call over to them when its block index does not pay (k24_hamming_index.hip).  out_counters: NULL, or int64[2].
int hamming_join_run(pfz_ctx *ctx, const pfz_dense *F, const pfz_dense *T, bool self, int64_t hmax, int64_t capacity, int64_t *out_row_ptr,
                     int32_t *out_idx, int32_t *out_dist, int64_t *out_total, int64_t *out_counters);
int hamming_comp_run(pfz_ctx *ctx, const pfz_dense *V, int64_t hmax, int32_t *out_label, int64_t *out_pairs, int64_t *out_components,
                     int64_t *out_counters);

}  // namespace pfz
