// K15's two pieces of arithmetic that host and device must agree on, in plain C++ so that a host program can be held to them
// (tests/k15_core_host.cpp): the integer cutoff of the threshold join, and the upper bound that lets a from-row skip a whole
// to-block.  See k15_sparse_join.hip for the kernel and k3_cossim_topn.hip for K3's fixed-point arithmetic.
//
// The cutoff.  K3's score of a pair is (float)sum * inv_scale, sum the int32 accumulator and inv_scale = 2^-k; a pair is a hit iff
// (double)((float)sum * inv_scale) >= min_similarity and sum >= 1 (a pair that shares no n-gram is "no match", also at 0).  The
// score is non-decreasing in sum -- int -> float rounds monotonically, and the product with a power of two is exact or rounds
// monotonically --, so there is ONE smallest passing sum, smin, and the kernel compares integers only.  smin is found by
// evaluating that very expression in a binary search, not by ceil(t * S): the float32 rounding of large sums moves the border
// (K11 and K13 derive their cutoffs by evaluation for the same reason).
//
// The block bound.  Let P be the n-grams of from-row i whose (k, b) list is non-empty, as_k = a_ik * S the row's scaled values.
// For every to-row j of block b
//     sum(i, j) = SUM_P trunc(fp32(as_k * b_jk)) <= SUM_P as_k * b_jk * (1 + 2^-24) <= sqrt(SUM_P as_k^2) * ||b_j|| * (1 + 2^-24)
// (Cauchy-Schwarz), and ||b_j|| <= the index's max_norm.  So with mass = SUM_P as_k^2, summed in float32,
//     k15_block_bound(mass, max_norm) = sqrtf(mass) * max_norm * 1.0001f
// is at least every sum of the block: 1.0001, the factor k3_fixed_point already puts on the norm bound, covers the fp32 product
// rounding (2^-24), the fp32 sum of at most 64 squares in any order (<= 64 * 2^-24 relative on the mass, half of it on the root),
// the root's and the two products' own roundings and the rounding of max_norm -- 3e-6 of the 1e-4 in all.  The block is skipped
// iff the bound is below (float)smin.  ONLY for rows of at most 64 n-grams (one value per lane, one wave reduction per block);
// longer rows go unpruned.  A tighter bound from per-list maximum weights needs a change to the index and is not made here.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define K15_HD __host__ __device__ inline
#else
#define K15_HD inline
#endif

namespace pfz {

// the hit rule on one sum
K15_HD bool k15_passes(int32_t sum, float inv_scale, double min_similarity)
{
    return sum >= 1 && (double)((float)sum * inv_scale) >= min_similarity;
}

// the smallest int32 sum that passes; 0: no sum below 2^31 does (there is nothing to launch)
inline int32_t k15_cutoff(float inv_scale, double min_similarity)
{
    if (!k15_passes(INT32_MAX, inv_scale, min_similarity)) return 0;
    int32_t lo = 1, hi = INT32_MAX;          // invariant: hi passes, everything below lo fails
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (k15_passes(mid, inv_scale, min_similarity)) hi = mid;
        else lo = mid + 1;
    }
    return hi;
}

K15_HD float k15_block_bound(float mass, float max_norm) { return sqrtf(mass) * max_norm * 1.0001f; }

// no sum of the block can reach smin
K15_HD bool k15_block_skippable(float mass, float max_norm, int32_t smin)
{
#ifdef PFZ_K15_NO_BOUND      // what-if builds only (tools/build_variant.sh): the bound's worth in time; results are the same
    (void)mass;
    (void)max_norm;
    (void)smin;
    return false;
#else
    return k15_block_bound(mass, max_norm) < (float)smin;
#endif
}

}  // namespace pfz
