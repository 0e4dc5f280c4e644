// polyfuzz_amd/csrc/k8_core.h -- the bit logic the K8 lanes run -- compiled for the host: every pair of two symbol
// lists (strings of up to 32 / 64 symbols; symbol 0 = a from-character the to-list never uses) scored as the register
// kernel scores it.  tests/test_jaro_cpu.py compares with the definition (tests/jaro_oracle.py).
#include <stddef.h>
#include <vector>

#include "../polyfuzz_amd/csrc/k8_core.h"

using namespace pfz;

template <typename WORD>
static int pairs(int64_t n_a, const int32_t *a_sym, const int64_t *a_off, int64_t n_b, const int32_t *b_sym, const int64_t *b_off,
                 int32_t n_sym1, int32_t winkler, double *out, float *out_bound)
{
    constexpr int WB = (int)sizeof(WORD) * 8;
    std::vector<WORD> pm((size_t)n_sym1);
    for (int64_t i = 0; i < n_a; ++i) {
        const int la = (int)(a_off[i + 1] - a_off[i]);
        if (la > WB) return 1;
        pm.assign((size_t)n_sym1, 0);
        for (int p = 0; p < la; ++p)
            if (a_sym[a_off[i] + p]) pm[(size_t)a_sym[a_off[i] + p]] |= (WORD)1 << p;
        for (int64_t k = 0; k < n_b; ++k) {
            const int lb = (int)(b_off[k + 1] - b_off[k]);
            if (lb > WB) return 1;
            const int32_t *b = b_sym + b_off[k];
            JaroFlags<WORD> s;
            jaro_begin(s, jaro_range(la, lb));
            // (the kernel walks whole packed dwords: up to three padding symbols, whose table entry is empty, behind the end)
            const int steps = (lb + 3) / 4 * 4;
            for (int j = 0; j < steps; ++j) jaro_match<WORD>(s, j < lb ? pm[(size_t)b[j]] : 0, j, j);
            const int m = __builtin_popcountll(s.fa);
            int half_t = 0;
            for (int j = 0; j < steps; ++j) half_t += jaro_transpose<WORD>(s, j < lb ? pm[(size_t)b[j]] : 0, j);
            out[i * n_b + k] = jaro_score(m, half_t, la, lb, jaro_prefix(s.pre), winkler);
            // the two bounds the kernel skips with: from m alone (before sweep 2), and with t
            out_bound[(i * n_b + k) * 2] = jaro_bound(m, 1.0f / (float)la, 1.0f / (float)lb, 1.0f, jaro_prefix(s.pre), winkler);
            out_bound[(i * n_b + k) * 2 + 1] =
                jaro_bound(m, 1.0f / (float)la, 1.0f / (float)lb, (float)(m - half_t / 2) / (float)m, jaro_prefix(s.pre), winkler);
        }
    }
    return 0;
}

// word_bits: 32 or 64, the register kernel's two classes
extern "C" int k8_host_pairs(int32_t word_bits, int64_t n_a, const int32_t *a_sym, const int64_t *a_off, int64_t n_b, const int32_t *b_sym,
                             const int64_t *b_off, int32_t n_sym1, int32_t winkler, double *out, float *out_bound)
{
    return word_bits == 32 ? pairs<uint32_t>(n_a, a_sym, a_off, n_b, b_sym, b_off, n_sym1, winkler, out, out_bound)
                           : pairs<uint64_t>(n_a, a_sym, a_off, n_b, b_sym, b_off, n_sym1, winkler, out, out_bound);
}
