// What K20 (k20_jaro_join.hip: a fixed threshold) and K21 (k21_jaro_topn.hip: a floor that rises) do alike, each thing once --
// device code on k8_core.h's bit logic and bounds:
//   the pair      what a lane does with its pair inside a group of a register kernel, against a float32 threshold: sweep 1 with
//                 the abandon rule, the bound, sweep 2, the bound again, the float64 score (jaro_pair_above);
//   the work      the four counters the kernels report and their flush (JaroWork);
//   the args      the fields both argument blocks begin with (JaroWalkArgs), and what the general kernels build from them: the
//                 workgroup's match table, the wave's flag words and pair_score.h's view of the two lists (jaro_general_begin).
// The kernels themselves stay apart: K20 has the window, the ownership rule and the sink, K21 the outward walk, the floor word and
// the list.  K8's register kernel (k8_jaro.hip) keeps its own two sweeps, see its header.
#pragma once

#include "edit_walk.h"
#include "k8_core.h"
#include "pair_score.h"

namespace pfz {

struct JaroWalkArgs : EditView {
    const int32_t *rows;       // from-rows of this launch
    int32_t n_rows;
    int32_t n_to;
    int32_t g_begin, g_end;    // the to-groups of this launch
    int32_t winkler;
    const void *t_chars;       // the raw to-list, which the general kernel reads (pair_score.h)
    int32_t t_width;
    const int64_t *t_off;
    unsigned long long *counters;   // optional [4], JaroWork's in order
};

// a lane's work counts: pairs whose sweep was asked for (K20: inside the length window; K21: of a group that was walked), pairs
// alive after sweep 1, pairs scored in float64, sweep-1 to-characters of live lanes
struct JaroWork {
    unsigned long long pairs = 0, alive = 0, scored = 0, steps = 0;
};

// once, when the wave has served its last row (four atomics per wave: per row they would queue up on four words)
__device__ inline void jaro_work_flush(unsigned long long *counters, const JaroWork &w)
{
    if (!counters) return;
    wave_count(counters + 0, w.pairs);
    wave_count(counters + 1, w.alive);
    wave_count(counters + 2, w.scored);
    wave_count(counters + 3, w.steps);
}

// One pair of a register kernel against the float32 threshold t32: the lane's to-string is its column of the plan's packed group g
// (wave-uniform), the from-string the match table pm in LDS.  Returns the float64 score, 0.0 for a lane that is dead -- on entry (padding,
// not owned, left out, outside the window) or by one of k8_core.h's rules, each of which dismisses a pair only where its score is
// below t32 -- and leaves in `alive` whether the score counts.  The whole wave calls it, and every lane that enters returns: every
// exit is wave-uniform, the callers need all 64 lanes behind it (the sink; topn_insert).
// WORD: uint32_t (from-strings of <= 32 characters) or uint64_t (<= 64); NB: to-strings of up to NB words' characters (K8's flag
// registers, walked stretch by stretch with compile-time indices).
// (`alive` and the step count are copied into locals, worked on there and written back at the end: worked on through the
// references inside the loops, or with a step count of the pair's own added at the end, the 64-bit-word instances take 2 - 3 more
// registers and K20's lose a wave per SIMD, docs/JARO_SWEEP_MEASURED.md)
template <typename WORD, int IDB, int NB>
__device__ __forceinline__ double jaro_pair_above(const EditView &V, const WORD *pm, int g, int la, int lb, float inv_la, float t32, int winkler,
                                                  bool &alive_io, JaroWork &work)
{
    constexpr int PER = 32 / IDB;  // symbols per dword
    constexpr int SPW = (int)sizeof(WORD) * 8 / PER;      // dwords per stretch
    bool alive = alive_io;
    unsigned long long n_steps = work.steps;
    const float inv_lb = __builtin_amdgcn_rcpf((float)lb);
    const int need = jaro_m_need(la, lb, inv_la, inv_lb, t32, winkler);
    const int steps = __builtin_amdgcn_readfirstlane(V.g_steps[g]);       // (g is wave-uniform: say so, or the loops get a per-lane trip count)
    const uint32_t *gp = V.b_packed + V.g_off[g] + (threadIdx.x & 63);
    JaroFlags<WORD> s;
    WORD fb[NB];
    jaro_begin(s, jaro_range(la, lb));
    // sweep 1, the abandon rule once per packed dword: a lane whose matches so far plus the to-characters still to come (or la)
    // are below its pair's m_need is dead
    bool go = true;                               // wave-uniform: a live lane has to-characters left
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        s.fb = 0;
        for (int t = k * SPW; go && t < min(steps, (k + 1) * SPW); ++t) {
            const uint32_t pk = gp[(int64_t)t * 64];
#pragma unroll
            for (int q = 0; q < PER; ++q)
                jaro_match<WORD>(s, pm[__builtin_amdgcn_ubfe(pk, q * IDB, IDB)], t * PER + q, (t - k * SPW) * PER + q);
            const int done = (t + 1) * PER;       // to-characters behind this lane (its own: min(done, lb))
            if (alive && done < lb && jaro_dead(la, __popcll((uint64_t)s.fa), lb - done, need)) {
                alive = false;
                n_steps += done;
            }
            go = __any(alive && done < lb);
        }
        fb[k] = s.fb;
    }
    n_steps += alive ? lb : 0;
    const int m = __popcll((uint64_t)s.fa);
    const int prefix = jaro_prefix(s.pre);
    // the bound from m alone, with the pair's own prefix (m = 0: asked before any 0 * inf reaches a comparison)
    alive = alive && jaro_reaches(m, inv_la, inv_lb, 1.0f, prefix, winkler, t32);
    work.alive += alive;
    int half_t = 0;
    // (one flagged pair cannot be out of order; the sweep runs for the wave if a single live lane wants it)
    if (__any(alive && m >= 2)) {
        go = true;                                // wave-uniform: a live lane has a flagged from-position left
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            s.fb = fb[k];
            for (int t = k * SPW; go && t < min(steps, (k + 1) * SPW); ++t) {
                const uint32_t pk = gp[(int64_t)t * 64];
#pragma unroll
                for (int q = 0; q < PER; ++q)
                    half_t += jaro_transpose<WORD>(s, pm[__builtin_amdgcn_ubfe(pk, q * IDB, IDB)], (t - k * SPW) * PER + q);
                go = __any(alive && s.fa != 0);
            }
        }
    }
    // the bound again, with t (m = 0: asked before the division's result is)
    const float last = (float)(m - half_t / 2) * __builtin_amdgcn_rcpf((float)m);
    alive = alive && jaro_reaches(m, inv_la, inv_lb, last, prefix, winkler, t32);
    work.scored += alive;
    work.steps = n_steps;
    alive_io = alive;
    return alive ? jaro_score(m, half_t, la, lb, prefix, winkler) : 0.0;
}

// What a general kernel (any lengths, any alphabet; flags and match table in global memory) has of its own: the workgroup's match
// table (WA words per symbol; zero on entry, zero again after every row), the wave's flag words (WA for the from-side, WS for a
// to-string: fa[w * 64] is this lane's word w) and pair_score.h's view of the two lists
struct JaroGeneral {
    uint64_t *pm, *fa, *fb;
    PairView P;
};

__device__ __forceinline__ JaroGeneral jaro_general_begin(const JaroWalkArgs &A, int32_t WA, int32_t WS, uint64_t *pm_all, uint64_t *fa_all,
                                                          uint64_t *fb_all)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    JaroGeneral G;
    G.pm = pm_all + (int64_t)blockIdx.x * A.n_sym1 * WA;
    G.fa = fa_all + ((int64_t)blockIdx.x * 4 + wave) * WA * 64 + lane;
    G.fb = fb_all + ((int64_t)blockIdx.x * 4 + wave) * WS * 64 + lane;
    static_cast<FromView &>(G.P) = A;
    G.P.b_chars = A.t_chars;
    G.P.b_width = A.t_width;
    G.P.b_off = A.t_off;
    G.P.n_to = A.n_to;
    G.P.scorer = A.winkler ? PAIR_JARO_WINKLER : PAIR_JARO;
    return G;
}

}  // namespace pfz
