// Host build of polyfuzz_amd/csrc/k10_core.h for tests/test_blocked_cpu.py: the LCS of one pair on one 32-bit word, one 64-bit word
// or several 64-bit words, and the ratio formula -- the functions K10's kernels call, compiled for the CPU.
#include "../polyfuzz_amd/csrc/k10_core.h"

#include <vector>

namespace {

// the from-positions [64 w, 64 w + 64) that hold code point c
uint64_t match_word(const int32_t *a, int la, int32_t c, int w)
{
    uint64_t m = 0;
    for (int i = 64 * w; i < la && i < 64 * w + 64; ++i) m |= (uint64_t)(a[i] == c) << (i - 64 * w);
    return m;
}

}  // namespace

extern "C" {

// mode 0: one 32-bit word (la <= 32), 1: one 64-bit word (la <= 64), 2: (la + 63) / 64 words.  Returns the LCS length, -1: la does
// not fit the mode.
int k10_host_lcs(const int32_t *a, int la, const int32_t *b, int lb, int mode)
{
    if ((mode == 0 && la > 32) || (mode == 1 && la > 64)) return -1;
    if (mode == 0) {
        uint32_t v = ~0u;
        for (int t = 0; t < lb; ++t) pfz::lcs_step_reg<uint32_t>(v, (uint32_t)match_word(a, la, b[t], 0));
        return __builtin_popcount(~v);
    }
    if (mode == 1) {
        uint64_t v = ~0ull;
        for (int t = 0; t < lb; ++t) pfz::lcs_step_reg<uint64_t>(v, match_word(a, la, b[t], 0));
        return __builtin_popcountll(~v);
    }
    const int W = la > 0 ? (la + 63) / 64 : 1;
    std::vector<uint64_t> v((std::size_t)W, ~0ull);
    for (int t = 0; t < lb; ++t) {
        uint64_t carry = 0;
        for (int w = 0; w < W; ++w) pfz::lcs_step_word(v[(std::size_t)w], match_word(a, la, b[t], w), carry);
    }
    int lcs = 0;
    for (int w = 0; w < W; ++w) lcs += __builtin_popcountll(~v[(std::size_t)w]);
    return lcs;
}

double k10_host_ratio(int lcs, long long maximum) { return pfz::ratio_of(lcs, (int64_t)maximum); }

}  // extern "C"
