// K18's per-pair logic on top of K7's (k7_core.h: the exact score fz_score and its float32 upper bound fz_upper_bound -- used
// unchanged): what a fixed floor lets a lane decide, and the packed hit.  Plain C++, shared by the HIP kernels (k18_fuzz_join.hip,
// k7_general.hip) and a host program (tests/k18_core_host.cpp).
//
// Pair (a, b) is a hit iff score(a, b) >= cutoff, float64 against float64 on rapidfuzz's 0..100 scale (rapidfuzz's score_cutoff:
// equal is a hit).  fz_score is exact whenever it is >= the floor it is given, and never above the true score below it, so with the
// cutoff as that floor the test on its result IS the test on the true score (tests/test_fuzz_join_cpu.py holds it to the oracle).
// A pair is left unscored only where its upper bound, with K7's slack for the bound's float32 rounding, is below the cutoff
// rounded to float32 -- K7's own prune rule with the row's running best replaced by a constant.
//
// The packed hit, one 64-bit key that sorts by (row, to-index): row << 32 | to-index.  A float64 score does not fit beside them: it
// is stored at the hit's position in an array of its own, and the position travels with the key through the sort as its 32-bit
// payload.  Limits this implies (pfz_fuzz_join refuses beyond them): fewer than 2^31 strings per list (K7's own limit is lower) and
// a capacity of at most 2^32 - 1 hits.
#pragma once

#include <stdint.h>

#ifndef K18_HD
#if defined(__HIPCC__)
#define K18_HD __host__ __device__ inline
#else
#define K18_HD inline
#endif
#endif

namespace pfz {

constexpr float kFuzzJoinSlack = 0.05f;                    // k7_device.h: kBoundSlack (k18_fuzz_join.hip asserts they are one)
constexpr int64_t kFuzzJoinMaxCapacity = 0xffffffffll;     // the payload is the hit's position in 32 bits

K18_HD uint64_t fuzz_key_pack(int32_t row, int32_t col) { return (uint64_t)(uint32_t)row << 32 | (uint64_t)(uint32_t)col; }
K18_HD int32_t fuzz_key_row(uint64_t key) { return (int32_t)(key >> 32); }
K18_HD int32_t fuzz_key_col(uint64_t key) { return (int32_t)(uint32_t)key; }

// the hit rule: float64 against float64, equal kept
K18_HD bool fuzz_join_hit(double score, double cutoff) { return score >= cutoff; }

// the prune rule: true = the pair must be scored (its bound does not rule a hit out)
K18_HD bool fuzz_join_go(float upper_bound, double cutoff) { return !(upper_bound + kFuzzJoinSlack < (float)cutoff); }

}  // namespace pfz
