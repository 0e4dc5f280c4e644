// K18: what the threshold kernels over K7's plan (k7_join_walk.h: k7_join_kernel; k7_general.hip: k7_general_join_kernel) do
// with a hit, and the fields of a call beside K7's argument block.  The sinks are edit_walk.h's KeyAppend / ForestHook with a
// float64 score: called by a whole wave, the hits of one call behind ONE atomic.
#pragma once

#include "k12_core.h"
#include "k18_core.h"

namespace pfz {

// what the kernels ask of a sink type at compile time: topn -- the sink is a wave's sorted list and the floor rises with it
// (k19_sink.h: FuzzTopn); the sinks below are called with every scored pair against a floor that never moves
template <typename SINK>
struct FuzzSinkTrait {
    static constexpr bool topn = false;
};

struct FuzzJoinArgs {
    double cutoff;               // 0..100; a pair is a hit iff score >= cutoff
    int32_t self;                // self-join: row i scores the choices j > i (K7's "up to" skip code -2 - i)
};

// the join's sink: key, score and payload (the position itself) at the hit's position, while there is room
struct FuzzAppend {
    unsigned long long *total;   // every hit
    uint64_t *keys;              // [capacity] row << 32 | to-index, in the order the waves got there
    double *score;               // [capacity]
    uint32_t *val;               // [capacity] the position: the sort's payload, through which the scores are gathered
    unsigned long long capacity;
    __device__ void operator()(bool hit, int row, int col, double s) const
    {
        const unsigned long long m = __ballot(hit);
        if (m == 0) return;
        const int lane = threadIdx.x & 63;
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(total, (unsigned long long)__popcll(m));
        base = __shfl(base, 0, 64);
        const unsigned long long pos = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
        if (hit && pos < capacity) {
            keys[pos] = fuzz_key_pack(row, col);
            score[pos] = s;
            val[pos] = (uint32_t)pos;
        }
    }
};

// the components' sink: the hits counted as the join counts them, each hit lane hooks its pair into K12's forest
struct FuzzUnite {
    unsigned long long *total;
    int32_t *parent;             // [n]
    __device__ void operator()(bool hit, int row, int col, double) const
    {
        const unsigned long long m = __ballot(hit);
        if (m == 0) return;
        if ((threadIdx.x & 63) == 0) atomicAdd(total, (unsigned long long)__popcll(m));
        if (hit) uf_unite<UfDeviceOps>(parent, row, col);
    }
};

}  // namespace pfz
