// polyfuzz_amd/csrc/k13_core.h -- what K13's lanes decide from the threshold: the integer cutoff lmin, the length window and the
// rule that abandons a walk -- and K10's LCS recurrence (k10_core.h) as K13 drives it, compiled for the host and checked against
// the definition.  tests/test_indel_join_cpu.py calls these and asserts on the reports.
//   k13_host_lmin_check    [0] (t, S) combinations checked, [1] some lcs in 0 .. S/2 with (indel_similarity(lcs, S) >= t) !=
//                          (lcs >= lmin), or lmin outside 0 .. S/2 + 1, [2] the similarity not strictly rising in lcs at some S
//   k13_host_window_check  [0] (t, la, lb) checked, [1] indel_in_window disagrees with the formula on min(la, lb), [2] for some la
//                          the lb inside are not one interval, [3] a non-empty interval that does not contain la, [4] (t, la)
//                          whose interval is not everything (the window does cut)
//   k13_host_walk          every pair of strings over {a, b} of up to max_len characters, the from-string padded in FRONT with
//                          'c' to pad_to characters (0: as it is), walked in 32-bit words, 64-bit words (word_bits) or the
//                          multi-word form (0): [0] pairs, [1] the LCS differs from the textbook table, [2] some prefix j with
//                          l_j + (lb - j) < lcs (abandon would kill a hit at SOME threshold), [3] l_j fell or rose by more than 1
//   k13_host_order         all (lcs1, S1), (lcs2, S2) with S <= max_s, lcs <= S / 2: [0] pairs of pairs, [1] indel_similarity and
//                          ratio_of compare differently (<, ==, >)
// With -DK13_HOST_MAIN: a stand-alone program (for a sanitizer run) that runs every check and exits 1 on a violation.
#include <stddef.h>
#include <algorithm>
#include <string>
#include <vector>

#include "../polyfuzz_amd/csrc/k13_core.h"

using namespace pfz;

static int table(const std::string &a, const std::string &b)
{
    std::vector<std::vector<int>> L(a.size() + 1, std::vector<int>(b.size() + 1, 0));
    for (size_t i = 1; i <= a.size(); ++i)
        for (size_t j = 1; j <= b.size(); ++j)
            L[i][j] = a[i - 1] == b[j - 1] ? L[i - 1][j - 1] + 1 : std::max(L[i - 1][j], L[i][j - 1]);
    return L[a.size()][b.size()];
}

// l_j for j = 0 .. lb as the register kernels have it
template <typename WORD> static void walk_single(const std::string &a, const std::string &b, std::vector<int> &l)
{
    WORD pm[256] = {};
    for (size_t p = 0; p < a.size(); ++p) pm[(unsigned char)a[p]] |= (WORD)1 << p;
    WORD v = (WORD)~(WORD)0;
    l.assign(1, indel_lcs_of(v, (int)a.size()));
    for (size_t j = 0; j < b.size(); ++j) {
        lcs_step_reg<WORD>(v, pm[(unsigned char)b[j]]);
        l.push_back(indel_lcs_of(v, (int)a.size()));
    }
}

// ... and as the general kernel has it: W 64-bit words, the carry chained
static void walk_multi(const std::string &a, const std::string &b, std::vector<int> &l)
{
    const int la = (int)a.size(), W = la > 0 ? (la + 63) / 64 : 1;
    std::vector<uint64_t> pm((size_t)256 * (size_t)W, 0), v((size_t)W, ~0ull);
    for (int p = 0; p < la; ++p) pm[(size_t)(unsigned char)a[(size_t)p] * (size_t)W + (size_t)(p / 64)] |= 1ull << (p % 64);
    auto count = [&]() {
        int n = 0;
        for (int w = 0; w < W; ++w) n += indel_lcs_of(v[(size_t)w], la - 64 * w);
        return n;
    };
    l.assign(1, count());
    for (size_t j = 0; j < b.size(); ++j) {
        const uint64_t *eq = &pm[(size_t)(unsigned char)b[j] * (size_t)W];
        uint64_t carry = 0;
        for (int w = 0; w < W; ++w) lcs_step_word(v[(size_t)w], eq[w], carry);
        l.push_back(count());
    }
}

static std::vector<std::string> all_strings(int max_len)
{
    std::vector<std::string> out;
    for (int n = 0; n <= max_len; ++n)
        for (int bits = 0; bits < (1 << n); ++bits) {
            std::string s((size_t)n, 'a');
            for (int p = 0; p < n; ++p)
                if (bits >> p & 1) s[(size_t)p] = 'b';
            out.push_back(s);
        }
    return out;
}

// lcs_out: NULL or int32[n * n], the strings in the order of all_strings (by length, then the binary number with 'b' = 1)
extern "C" int k13_host_walk(int32_t word_bits, int32_t max_len, int32_t pad_to, int64_t *report, int32_t *lcs_out)
{
    if (word_bits != 0 && word_bits != 32 && word_bits != 64) return 2;
    if (word_bits != 0 && std::max(pad_to, max_len) > word_bits) return 2;
    const std::vector<std::string> s = all_strings(max_len);
    std::vector<int> l;
    for (size_t i = 0; i < s.size(); ++i) {
        const std::string a = (size_t)pad_to > s[i].size() ? std::string((size_t)pad_to - s[i].size(), 'c') + s[i] : s[i];
        for (size_t k = 0; k < s.size(); ++k) {
            const std::string &b = s[k];
            if (word_bits == 32) walk_single<uint32_t>(a, b, l);
            else if (word_bits == 64) walk_single<uint64_t>(a, b, l);
            else walk_multi(a, b, l);
            const int lb = (int)b.size(), lcs = l[(size_t)lb];
            report[0] += 1;
            report[1] += lcs != table(s[i], b);
            bool below = false, jump = l[0] != 0;
            for (int j = 0; j <= lb; ++j) {
                below |= l[(size_t)j] + (lb - j) < lcs;
                jump |= j > 0 && (l[(size_t)j] < l[(size_t)j - 1] || l[(size_t)j] > l[(size_t)j - 1] + 1);
            }
            report[2] += below;
            report[3] += jump;
            if (lcs_out) lcs_out[i * s.size() + k] = lcs;
        }
    }
    return 0;
}

extern "C" int k13_host_lmin_check(int64_t n_t, const double *ts, int32_t max_s, int64_t *report)
{
    for (int S = 0; S <= max_s; ++S) {
        bool rising = true;
        for (int x = 1; x <= S / 2; ++x) rising &= indel_similarity(x, S) > indel_similarity(x - 1, S);
        report[2] += !rising;
        for (int64_t k = 0; k < n_t; ++k) {
            const double t = ts[k];
            const int lm = indel_lmin(t, S);
            bool wrong = lm < 0 || lm > S / 2 + 1;
            for (int x = 0; x <= S / 2; ++x) wrong |= (indel_similarity(x, S) >= t) != (x >= lm);
            report[0] += 1;
            report[1] += wrong;
        }
    }
    return 0;
}

extern "C" int k13_host_window_check(int64_t n_t, const double *ts, int32_t max_len, int64_t *report)
{
    std::vector<int> lmin((size_t)2 * (size_t)max_len + 1);
    for (int64_t k = 0; k < n_t; ++k) {
        const double t = ts[k];
        for (int S = 0; S <= 2 * max_len; ++S) lmin[(size_t)S] = indel_lmin(t, S);
        for (int la = 0; la <= max_len; ++la) {
            int first = -1, last = -1, inside = 0;
            for (int lb = 0; lb <= max_len; ++lb) {
                const bool in = indel_in_window(lmin[(size_t)(la + lb)], la, lb);
                report[0] += 1;
                report[1] += in != (indel_similarity(std::min(la, lb), la, lb) >= t);
                if (in) {
                    if (first < 0) first = lb;
                    last = lb;
                    ++inside;
                }
            }
            report[2] += inside > 0 && inside != last - first + 1;
            report[3] += inside > 0 && !(first <= la && la <= last);
            report[4] += inside != max_len + 1;
        }
    }
    return 0;
}

extern "C" int k13_host_order(int32_t max_s, int64_t *report)
{
    struct P { int lcs, S; double sim, ratio; };
    std::vector<P> p;
    for (int S = 0; S <= max_s; ++S)
        for (int x = 0; x <= S / 2; ++x) p.push_back(P{x, S, indel_similarity(x, S), ratio_of(x, S)});
    for (const P &u : p)
        for (const P &w : p) {
            report[0] += 1;
            report[1] += (u.sim < w.sim) != (u.ratio < w.ratio) || (u.sim == w.sim) != (u.ratio == w.ratio);
        }
    return 0;
}

extern "C" int32_t k13_host_lmin(double t, int32_t S) { return indel_lmin(t, S); }
extern "C" double k13_host_similarity(int32_t lcs, int32_t la, int32_t lb) { return indel_similarity(lcs, la, lb); }
extern "C" double k13_host_ratio(int32_t lcs, int32_t la, int32_t lb) { return ratio_of(lcs, (int64_t)la + lb); }
extern "C" int32_t k13_host_abandon(int32_t l_j, int32_t j, int32_t lb, int32_t lmin) { return indel_abandon(l_j, j, lb, lmin); }

extern "C" void k13_host_unpack(int32_t row, int32_t to, int32_t lcs, int32_t *out)
{
    const uint64_t key = join_pack(row, to, lcs);
    out[0] = join_key_row(key);
    out[1] = join_key_to(key);
    out[2] = join_key_dist(key);
}

#ifdef K13_HOST_MAIN
#include <cmath>
#include <stdio.h>

int main()
{
    std::vector<double> ts;
    for (double t : {0.0, 0.25, 1.0 / 3.0, 0.5, 2.0 / 3.0, 0.8, 0.9, 1.0})
        for (double v : {std::nextafter(t, -1.0), t, std::nextafter(t, 2.0)})
            if (v >= 0.0 && v <= 1.0) ts.push_back(v);
    int bad = 0;
    int64_t a[3] = {}, b[5] = {}, c[2] = {};
    k13_host_lmin_check((int64_t)ts.size(), ts.data(), 600, a);
    k13_host_window_check((int64_t)ts.size(), ts.data(), 300, b);
    k13_host_order(100, c);
    printf("lmin: %lld checked, %lld wrong, %lld not rising; window: %lld checked, %lld wrong, %lld split, %lld off la; order: %lld of %lld\n",
           (long long)a[0], (long long)a[1], (long long)a[2], (long long)b[0], (long long)b[1], (long long)b[2], (long long)b[3],
           (long long)c[1], (long long)c[0]);
    bad |= a[1] || a[2] || b[1] || b[2] || b[3] || c[1];
    const int forms[][2] = {{32, 0}, {64, 0}, {0, 0}, {64, 64}, {0, 64}, {0, 65}, {0, 130}};
    for (const auto &f : forms) {
        int64_t rep[4] = {};
        k13_host_walk(f[0], 6, f[1], rep, nullptr);
        printf("word %2d pad %3d: pairs %lld lcs %lld below %lld jump %lld\n", f[0], f[1], (long long)rep[0], (long long)rep[1],
               (long long)rep[2], (long long)rep[3]);
        bad |= rep[1] || rep[2] || rep[3];
    }
    return bad;
}
#endif
