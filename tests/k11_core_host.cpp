// polyfuzz_amd/csrc/k11_core.h -- what K11's lanes decide from the threshold: the per-pair cutoff kmax, the length window and the
// rule that abandons a walk -- compiled for the host and checked against the definition, exhaustively: every pair of strings over
// {a, b} of up to `max_len` characters, walked as the register kernels do (one 32- or 64-bit word) or as the general kernel does
// (64-bit words, lev_step_word), and seeded long pairs whose from-strings cross the word borders.  For every pair and threshold:
//   [0] pairs checked
//   [1] kmax disagrees with the formula: some d in 0 .. M with (lev_similarity(d) >= t) != (d <= kmax)
//   [2] the walk's bound exceeds the final distance: some j with dist_j - (lb - j) > d
//   [3] a hit lost: lev_similarity(d) >= t, and the window or the abandon rule would have left the pair out
//   [4] the bit logic's distance differs from the textbook table (computed here)
//   [5] (pair, threshold) combinations the abandon rule fired on (it must be at work, or [3] shows nothing)
//   [6] a horizontal delta of the bottom cell outside -1 .. +1
// tests/test_join_cpu.py asserts [1] [2] [3] [4] [6] == 0 and compares the distances with tests/lev_oracle.py.
// With -DK11_HOST_MAIN: a stand-alone program (for a sanitizer run) that runs every form and exits 1 on a violation.
#include <stddef.h>
#include <algorithm>
#include <string>
#include <vector>

#include "../polyfuzz_amd/csrc/k11_core.h"
#include "rows_fill_host.h"

using namespace pfz;

static int table(const std::string &a, const std::string &b, bool osa)
{
    const int la = (int)a.size(), lb = (int)b.size();
    std::vector<std::vector<int>> D((size_t)la + 1, std::vector<int>((size_t)lb + 1));
    for (int i = 0; i <= la; ++i) D[(size_t)i][0] = i;
    for (int j = 0; j <= lb; ++j) D[0][(size_t)j] = j;
    for (int i = 1; i <= la; ++i)
        for (int j = 1; j <= lb; ++j) {
            int v = std::min({D[(size_t)i - 1][(size_t)j] + 1, D[(size_t)i][(size_t)j - 1] + 1,
                              D[(size_t)i - 1][(size_t)j - 1] + (a[(size_t)i - 1] != b[(size_t)j - 1])});
            if (osa && i >= 2 && j >= 2 && a[(size_t)i - 1] == b[(size_t)j - 2] && a[(size_t)i - 2] == b[(size_t)j - 1])
                v = std::min(v, D[(size_t)i - 2][(size_t)j - 2] + 1);
            D[(size_t)i][(size_t)j] = v;
        }
    return D[(size_t)la][(size_t)lb];
}

// dist_j for j = 0 .. lb: the bottom cell of the column after j to-characters, as the kernels track it
template <typename WORD, bool OSA> static void walk_single(const std::string &a, const std::string &b, std::vector<int> &dist)
{
    WORD pm[256] = {};
    for (size_t p = 0; p < a.size(); ++p) pm[(unsigned char)a[p]] |= (WORD)1 << p;
    LevState<WORD> s;
    lev_begin(s, (int)a.size());
    dist.assign(1, s.dist);
    for (size_t j = 0; j < b.size(); ++j) {
        lev_step<WORD, OSA>(s, pm[(unsigned char)b[j]], true);
        dist.push_back(s.dist);
    }
}

template <bool OSA> static void walk_multi(const std::string &a, const std::string &b, std::vector<int> &dist)
{
    const int la = (int)a.size(), W = la > 0 ? (la + 63) / 64 : 1;
    std::vector<uint64_t> pm((size_t)256 * (size_t)W, 0), vp((size_t)W), vn((size_t)W, 0), d0((size_t)W, 0);
    for (int p = 0; p < la; ++p) pm[(size_t)(unsigned char)a[(size_t)p] * (size_t)W + (size_t)(p / 64)] |= 1ull << (p % 64);
    for (int w = 0; w < W; ++w) vp[(size_t)w] = low_ones<uint64_t>(la - 64 * w);
    const uint64_t last = la > 0 ? 1ull << ((la - 1) % 64) : 0;
    int d = la;
    dist.assign(1, d);
    const std::vector<uint64_t> none((size_t)W, 0);
    for (size_t j = 0; j < b.size(); ++j) {
        const uint64_t *eq = &pm[(size_t)(unsigned char)b[j] * (size_t)W];
        const uint64_t *eq_prev = j > 0 ? &pm[(size_t)(unsigned char)b[j - 1] * (size_t)W] : none.data();
        LevCarry c = lev_carry_begin();
        uint64_t hp = 0, hn = 0;
        for (int w = 0; w < W; ++w) lev_step_word<OSA>(vp[(size_t)w], vn[(size_t)w], d0[(size_t)w], eq[w], eq_prev[w], c, &hp, &hn);
        d += (int)((hp & last) != 0) - (int)((hn & last) != 0);
        dist.push_back(d);
    }
}

static void check_pair(const std::string &a, const std::string &b, bool osa, const std::vector<int> &dist, int64_t n_t, const double *ts,
                       int64_t *report, int32_t *d_out)
{
    const int la = (int)a.size(), lb = (int)b.size(), m = std::max(la, lb);
    const int d = lev_distance(dist[(size_t)lb], la, lb);
    if (d_out) *d_out = d;
    report[0] += 1;
    report[4] += d != table(a, b, osa);
    bool above = false, wide = false;
    for (int j = 0; j <= lb; ++j) {
        above |= dist[(size_t)j] - (lb - j) > d;
        wide |= j > 0 && la > 0 && std::abs(dist[(size_t)j] - dist[(size_t)j - 1]) > 1;
    }
    report[2] += above;
    report[6] += wide;
    for (int64_t k = 0; k < n_t; ++k) {
        const double t = ts[k];
        const int km = join_kmax(t, la, lb);
        bool wrong = km < -1 || km > m;
        for (int x = 0; x <= m; ++x) wrong |= (lev_similarity(x, la, lb) >= t) != (x <= km);
        report[1] += wrong;
        bool left_out = !join_in_window(km, la, lb);
        bool fired = false;
        for (int j = 0; j <= lb; ++j) fired |= join_abandon(dist[(size_t)j], j, lb, km);
        report[5] += fired && !left_out;
        if (lev_similarity(d, la, lb) >= t) report[3] += left_out || fired;
    }
}

template <bool OSA> static void walk(int word_bits, const std::string &a, const std::string &b, std::vector<int> &dist)
{
    if (word_bits == 32) walk_single<uint32_t, OSA>(a, b, dist);
    else if (word_bits == 64) walk_single<uint64_t, OSA>(a, b, dist);
    else walk_multi<OSA>(a, b, dist);
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

// word_bits: 32 or 64, the register kernel's two classes; 0: the multi-word form.  d_out: NULL or int32[n * n] distances, the
// strings in the order of all_strings (by length, then the binary number with 'b' = 1, first character lowest)
extern "C" int k11_host_exhaustive(int32_t word_bits, int32_t osa, int32_t max_len, int64_t n_t, const double *ts, int64_t *report,
                                   int32_t *d_out)
{
    if (word_bits != 0 && word_bits != 32 && word_bits != 64) return 2;
    const std::vector<std::string> s = all_strings(max_len);
    std::vector<int> dist;
    for (size_t i = 0; i < s.size(); ++i)
        for (size_t k = 0; k < s.size(); ++k) {
            if (osa) walk<true>(word_bits, s[i], s[k], dist);
            else walk<false>(word_bits, s[i], s[k], dist);
            check_pair(s[i], s[k], osa != 0, dist, n_t, ts, report, d_out ? d_out + i * s.size() + k : nullptr);
        }
    return 0;
}

// seeded pairs over {a, b} with from-strings at the word borders (near-duplicates among them, so that there are hits)
extern "C" int k11_host_long(int32_t word_bits, int32_t osa, int64_t n_pairs, int64_t n_t, const double *ts, int64_t *report)
{
    static const int borders[] = {31, 32, 33, 63, 64, 65, 127, 128, 129, 130};
    uint64_t x = 0x9e3779b97f4a7c15ull;
    auto next = [&x]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    std::vector<int> dist;
    for (int64_t n = 0; n < n_pairs; ++n) {
        const int la = borders[next() % 10];
        if (word_bits != 0 && la > word_bits) continue;
        std::string a((size_t)la, 'a'), b;
        for (char &c : a) c = next() & 1 ? 'b' : 'a';
        if (n % 2) {                     // an edited copy: a few substitutions, deletions, insertions, swaps
            b = a;
            for (int e = (int)(next() % 12); e > 0 && !b.empty(); --e) {
                const size_t p = next() % b.size();
                switch (next() % 4) {
                case 0: b[p] = b[p] == 'a' ? 'b' : 'a'; break;
                case 1: b.erase(p, 1); break;
                case 2: b.insert(p, 1, next() & 1 ? 'b' : 'a'); break;
                default: if (p + 1 < b.size()) std::swap(b[p], b[p + 1]);
                }
            }
        }
        else {
            b.assign((size_t)(next() % 141), 'a');
            for (char &c : b) c = next() & 1 ? 'b' : 'a';
        }
        if (osa) walk<true>(word_bits, a, b, dist);
        else walk<false>(word_bits, a, b, dist);
        check_pair(a, b, osa != 0, dist, n_t, ts, report, nullptr);
    }
    return 0;
}

extern "C" int32_t k11_host_kmax(double t, int32_t la, int32_t lb) { return join_kmax(t, la, lb); }

extern "C" void k11_host_unpack(int32_t row, int32_t to, int32_t d, int32_t *out)
{
    const uint64_t key = join_pack(row, to, d);
    out[0] = join_key_row(key);
    out[1] = join_key_to(key);
    out[2] = join_key_dist(key);
}

// the row pointers of the unpacking (rows_fill_host.h), in both pointer widths; *cases: the sequences tried
extern "C" int k11_host_rows_fill(int64_t *cases)
{
    long long n = 0;
    const int bad = rows_fill_check<int64_t>(&n) + rows_fill_check<int32_t>(&n);
    *cases = n;
    return bad;
}

#ifdef K11_HOST_MAIN
#include <cmath>
#include <stdio.h>

int main()
{
    std::vector<double> ts;
    for (double t : {0.0, 0.25, 1.0 / 3.0, 0.5, 2.0 / 3.0, 0.8, 1.0})
        for (double v : {std::nextafter(t, -1.0), t, std::nextafter(t, 2.0)})
            if (v >= 0.0 && v <= 1.0) ts.push_back(v);
    int bad = 0;
    for (int word_bits : {32, 64, 0})
        for (int osa = 0; osa < 2; ++osa) {
            int64_t rep[7] = {};
            k11_host_exhaustive(word_bits, osa, 6, (int64_t)ts.size(), ts.data(), rep, nullptr);
            k11_host_long(word_bits, osa, 600, (int64_t)ts.size(), ts.data(), rep);
            printf("word %2d osa %d: pairs %lld kmax %lld bound %lld lost %lld table %lld fired %lld delta %lld\n", word_bits, osa,
                   (long long)rep[0], (long long)rep[1], (long long)rep[2], (long long)rep[3], (long long)rep[4], (long long)rep[5],
                   (long long)rep[6]);
            bad |= rep[1] || rep[2] || rep[3] || rep[4] || rep[6] || rep[5] == 0;
        }
    int64_t cases = 0;
    bad |= k11_host_rows_fill(&cases) != 0;
    printf("rows_fill: %lld sequences\n", (long long)cases);
    return bad;
}
#endif
