// K7 / K18: what the register / LDS kernels over K7's plan share -- the arg-max kernel (k7_fuzz.hip: k7_fuzz_kernel) and the
// threshold join and the top-n form (k7_join_walk.h: k7_join_kernel).  The device-side settings k7_core.h is compiled under, the few lane helpers
// both kernels use, and the host-side preparation of a call (forms, plan, from-token ids, the FuzzArgs fill, the word-class split).
#pragma once
#include "pfz_internal.h"

#include <vector>

#undef PFZ_HD
#define PFZ_HD __device__ inline
#define PFZ_LDS_U16 __attribute__((address_space(3))) uint16_t
#define PFZ_LDS_U8 __attribute__((address_space(3))) uint8_t
#ifdef PFZ_K7_PROFILE
#define FZ_TICK(T, k)                                                 \
    do {                                                              \
        const long long now_ = clock64();                             \
        (T).tk[k] += (unsigned int)(now_ - (T).t0);                   \
        (T).t0 = now_;                                                \
    } while (0)
#endif
// (the builtin takes the condition as it is: __ballot() compares an integer copy of it with 0 -- a select and a compare more)
#define FZ_BALLOT(x) __builtin_amdgcn_ballot_w64(x)
#define FZ_ANY(x) (FZ_BALLOT(x) != 0ull)
#include "k7_core.h"
#include "k7_args.h"
#include "k7_plan.h"

namespace pfz {

// One from-string per WAVE (a one-wave workgroup): what a from-string costs on top of its pairs -- the bounding sweeps, a
// batch of seeds, a last partial batch -- is paid per wave that works on it, and four waves sharing one from-string paid
// it four times over (the 100 000-name self-match: 0.79 -> 0.49 s).  More waves per workgroup = fewer from-strings in flight.
constexpr int kK7Waves = 1, kK7Threads = 64 * kK7Waves;
#ifndef PFZ_K7_OCC
#define PFZ_K7_OCC 4          // one-word rows: waves per SIMD the compiler budgets registers for (tuning builds: 3 = no spills)
#endif
constexpr float kBoundSlack = 0.05f;

// how many of the lanes below this one are set in a wave mask (v_mbcnt: two instructions)
__device__ inline int lanes_below(unsigned long long mask)
{
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// v where any of m's four components equals id (a wave-uniform value, in a scalar register), else 0
__device__ inline int select_if_any_eq(const int4 &m, int id, int v)
{
    uint64_t e0, e1, e2, e3;
    int r;
    asm("v_cmp_eq_u32_e64 %0, %1, %2" : "=s"(e0) : "s"(id), "v"(m.x));
    asm("v_cmp_eq_u32_e64 %0, %1, %2" : "=s"(e1) : "s"(id), "v"(m.y));
    asm("v_cmp_eq_u32_e64 %0, %1, %2" : "=s"(e2) : "s"(id), "v"(m.z));
    asm("v_cmp_eq_u32_e64 %0, %1, %2" : "=s"(e3) : "s"(id), "v"(m.w));
    const uint64_t any = (e0 | e1) | (e2 | e3);
    asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(r) : "v"(v), "s"(any));
    return r;
}

__device__ inline bool mode_uses_tokens(int mode) { return mode != kPartialRatio && mode != kPartialTokenSortRatio; }

// 64-bit word-steps a scored pair costs at most (work accounting for the roofline; an estimate from the lengths: one
// pass over the to-form per LCS, |from| x |to| for a window sweep)
__device__ inline int work_estimate(const Fz3<int> &la, const int4 &m, int mode, int W)
{
    const int pass = m.x + m.y + m.z;
    if (mode == kTokenSetRatio || mode == kTokenRatio) return pass * W;
    return (pass + fz_min(la[0], m.x) * fz_max(la[0], m.x) / 4) * W;
}

// ---- host side ------------------------------------------------------------------------------------------------------------

// What a call over rows [begin, end) of `from` against `to` prepares before it launches anything (k7_fuzz.hip: fuzz_prepare):
// the token forms of both lists and the to-side plan (built on first use, cached on the handles), the from-list's token ids in
// the plan's table, the argument block's from- and to-side fields, and the from-rows by word class -- rows[c] / slot[c] (the
// row's position in [begin, end)) for c = 0, 1, 2: one, two, four 64-bit words per form (<= 64, 128, 256 characters), each class
// longest string first; c = 3: the general kernel's (beyond 256 characters, 32 distinct tokens or the 60 KiB match table, or all
// of them under PFZ_K7_FORCE_GENERAL).
struct FuzzPrep {
    const pfz_fuzz_plan *plan = nullptr;
    DevBuf d_aid;                              // the from-list's token ids (two lists; a self-call reads the plan's own)
    FuzzArgs A{};
    std::vector<int32_t> rows[4], slot[4];
};
constexpr int kFuzzWords[3] = {1, 2, 4};
int fuzz_prepare(pfz_ctx *ctx, const pfz_strings *from, const pfz_strings *to, int32_t scorer, int64_t begin, int64_t end, FuzzPrep *P);
// persistent one-wave workgroups a launch may have (units are handed out), and into how many units a from-row of class c is
// split when the class has n_rows of them: few rows are split so that every workgroup has work, PFZ_K7_PARTS overrides
int64_t fuzz_max_grid(const pfz_ctx *ctx);
int32_t fuzz_parts(const pfz_ctx *ctx, const pfz_fuzz_plan *plan, int64_t n_rows);
// the match table of word class c in bytes: the first part of the dynamic LDS of both kernels (their scratch columns follow it)
inline size_t fuzz_table_bytes(const FuzzArgs &A, int c) { return (size_t)A.n_sym1 * 3 * (size_t)kFuzzWords[c] * sizeof(uint64_t); }

}  // namespace pfz
