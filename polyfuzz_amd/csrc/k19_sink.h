// K19: the third sink of the kernels over K7's plan (k7_join_walk.h: k7_join_kernel; k7_general.hip: k7_general_join_kernel) --
// the ntop best choices of every from-row instead of every pair above a cutoff.  The sink itself is only the address of the
// lists: the list of a unit lives in the wave that walks it (topn_wave.h: TopnList, entry p in lane p), and the kernels handle
// it behind `if constexpr (FuzzSinkTrait<SINK>::topn)`.
//
// The list buffer of a call: [row - from_begin][n_lists][ntop] of TopnKey, filled with 0xff before the kernels ("no entry"), so a
// slot no wave writes -- a part a class does not have, the general lists of a row the general kernel never sees -- is empty.
// n_lists = the largest `parts` of the call's fast launches + kTopnGeneralLists; one topn_merge per call picks the row's.
#pragma once

#include "k18_sink.h"
#include "topn_wave.h"

namespace pfz {

constexpr int kTopnGeneralLists = 4;      // the waves of k7_general_join_kernel's workgroup: each leaves a list of its own

struct FuzzTopn {
    TopnKey *lists;
    int32_t ntop, n_lists;
    int64_t from_begin;
    int32_t general0;            // the general kernel's first slot of a row in this launch (k7_join_walk.h: fuzz_join_launch)
    __device__ TopnKey *slot(int row, int k) const { return lists + (((int64_t)row - from_begin) * n_lists + k) * ntop; }
};

template <>
struct FuzzSinkTrait<FuzzTopn> {
    static constexpr bool topn = true;
};

}  // namespace pfz
