// polyfuzz_amd/csrc/k9_core.h -- the bit logic the K9 lanes run -- compiled for the host: every pair of two symbol lists (symbol 0 =
// a from-character the to-list never uses) as the register kernels walk it (one 32- or 64-bit word, padding steps behind the
// to-string's end included), as the multi-word recurrence goes word by word (any number of 64-bit words), and as the general
// kernels walk their column in global memory (lev_column_begin / lev_column_step at a lane stride).  tests/test_levenshtein_cpu.py compares
// with the textbook table (tests/lev_oracle.py).
#include <stddef.h>
#include <vector>

#include "../polyfuzz_amd/csrc/k9_core.h"

using namespace pfz;

template <typename WORD, bool OSA>
static int single(int64_t n_a, const int32_t *a_sym, const int64_t *a_off, int64_t n_b, const int32_t *b_sym, const int64_t *b_off,
                  int32_t n_sym1, int32_t *out)
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
            const int32_t *b = b_sym + b_off[k];
            LevState<WORD> s;
            lev_begin(s, la);
            // (the kernel walks the packed dwords of its group's longest string: padding symbols, whose table entry is empty)
            const int steps = (lb + 3) / 4 * 4 + 8;
            for (int j = 0; j < steps; ++j) lev_step<WORD, OSA>(s, j < lb ? pm[(size_t)b[j]] : (WORD)0, j < lb);
            out[i * n_b + k] = lev_distance(s.dist, la, lb);
        }
    }
    return 0;
}

template <bool OSA>
static int multi(int64_t n_a, const int32_t *a_sym, const int64_t *a_off, int64_t n_b, const int32_t *b_sym, const int64_t *b_off,
                 int32_t n_sym1, int32_t *out)
{
    for (int64_t i = 0; i < n_a; ++i) {
        const int la = (int)(a_off[i + 1] - a_off[i]);
        const int W = la > 0 ? (la + 63) / 64 : 1;
        std::vector<uint64_t> pm((size_t)n_sym1 * (size_t)W, 0), vp((size_t)W), vn((size_t)W), d0((size_t)W);
        for (int p = 0; p < la; ++p)
            if (a_sym[a_off[i] + p]) pm[(size_t)a_sym[a_off[i] + p] * (size_t)W + (size_t)(p / 64)] |= 1ull << (p % 64);
        for (int64_t k = 0; k < n_b; ++k) {
            const int lb = (int)(b_off[k + 1] - b_off[k]);
            const int32_t *b = b_sym + b_off[k];
            for (int w = 0; w < W; ++w) {
                vp[(size_t)w] = low_ones<uint64_t>(la - 64 * w);
                vn[(size_t)w] = d0[(size_t)w] = 0;
            }
            int dist = la;
            const uint64_t last = la > 0 ? 1ull << ((la - 1) % 64) : 0;
            for (int j = 0; j < lb; ++j) {
                const uint64_t *eq = &pm[(size_t)b[j] * (size_t)W], *eq_prev = &pm[(size_t)(j > 0 ? b[j - 1] : 0) * (size_t)W];
                LevCarry c = lev_carry_begin();
                uint64_t hp = 0, hn = 0;
                for (int w = 0; w < W; ++w)
                    lev_step_word<OSA>(vp[(size_t)w], vn[(size_t)w], d0[(size_t)w], eq[w], eq_prev[w], c, &hp, &hn);
                dist += (int)((hp & last) != 0) - (int)((hn & last) != 0);
            }
            out[i * n_b + k] = lev_distance(dist, la, lb);
        }
    }
    return 0;
}

// The general kernels' column as they keep it (lev_column_begin / lev_column_step): `stride` lanes interleave their words -- lane k
// of a group of to-strings has word w at [w * stride + k] -- and the match table has WA words per symbol, of which a from-string
// of la characters uses the first W = ceil(la / 64).  The words beyond W are poisoned first and must come back untouched.
template <bool OSA>
static int column(int64_t n_a, const int32_t *a_sym, const int64_t *a_off, int64_t n_b, const int32_t *b_sym, const int64_t *b_off,
                  int32_t n_sym1, int32_t stride, int32_t WA, int32_t *out)
{
    const uint64_t poison = 0xa5a5a5a5a5a5a5a5ull;
    std::vector<uint64_t> pm((size_t)n_sym1 * (size_t)WA), vp((size_t)WA * (size_t)stride), vn(vp.size()), d0(vp.size());
    for (int64_t i = 0; i < n_a; ++i) {
        const int la = (int)(a_off[i + 1] - a_off[i]);
        const int W = la > 0 ? (la + 63) / 64 : 1;
        if (W > WA) return 1;
        pm.assign(pm.size(), 0);
        for (int p = 0; p < la; ++p)
            if (a_sym[a_off[i] + p]) pm[(size_t)a_sym[a_off[i] + p] * (size_t)WA + (size_t)(p / 64)] |= 1ull << (p % 64);
        vp.assign(vp.size(), poison);
        vn.assign(vn.size(), poison);
        d0.assign(d0.size(), poison);
        const uint64_t last = la > 0 ? 1ull << ((la - 1) % 64) : 0ull;
        for (int64_t k = 0; k < n_b; ++k) {
            const int lane = (int)(k % stride), lb = (int)(b_off[k + 1] - b_off[k]);
            const int32_t *b = b_sym + b_off[k];
            lev_column_begin(&vp[(size_t)lane], &vn[(size_t)lane], &d0[(size_t)lane], W, la, stride);
            int dist = la;
            for (int j = 0; j < lb; ++j)
                dist += lev_column_step<OSA>(&vp[(size_t)lane], &vn[(size_t)lane], &d0[(size_t)lane], &pm[(size_t)b[j] * (size_t)WA],
                                             &pm[(size_t)(j > 0 ? b[j - 1] : 0) * (size_t)WA], W, last, stride);
            out[i * n_b + k] = lev_distance(dist, la, lb);
        }
        for (size_t at = (size_t)W * (size_t)stride; at < vp.size(); ++at)
            if (vp[at] != poison || vn[at] != poison || d0[at] != poison) return 3;
    }
    return 0;
}

extern "C" int k9_host_column(int32_t osa, int32_t stride, int32_t WA, int64_t n_a, const int32_t *a_sym, const int64_t *a_off, int64_t n_b,
                              const int32_t *b_sym, const int64_t *b_off, int32_t n_sym1, int32_t *out)
{
    return osa ? column<true>(n_a, a_sym, a_off, n_b, b_sym, b_off, n_sym1, stride, WA, out)
               : column<false>(n_a, a_sym, a_off, n_b, b_sym, b_off, n_sym1, stride, WA, out);
}

// word_bits: 32 or 64, the register kernel's two classes; 0: the multi-word form
extern "C" int k9_host_pairs(int32_t word_bits, int32_t osa, int64_t n_a, const int32_t *a_sym, const int64_t *a_off, int64_t n_b,
                             const int32_t *b_sym, const int64_t *b_off, int32_t n_sym1, int32_t *out)
{
#define K9_ARGS n_a, a_sym, a_off, n_b, b_sym, b_off, n_sym1, out
    if (word_bits == 32) return osa ? single<uint32_t, true>(K9_ARGS) : single<uint32_t, false>(K9_ARGS);
    if (word_bits == 64) return osa ? single<uint64_t, true>(K9_ARGS) : single<uint64_t, false>(K9_ARGS);
    if (word_bits == 0) return osa ? multi<true>(K9_ARGS) : multi<false>(K9_ARGS);
    return 2;
#undef K9_ARGS
}

extern "C" void k9_host_similarity(int64_t n, const int32_t *d, const int32_t *la, const int32_t *lb, double *sim, double *bound)
{
    for (int64_t i = 0; i < n; ++i) {
        sim[i] = lev_similarity(d[i], la[i], lb[i]);
        bound[i] = lev_length_bound(la[i], lb[i]);
    }
}
