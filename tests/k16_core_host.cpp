// Host build of polyfuzz_amd/csrc/k16_core.h, run stand-alone by tests/test_pairs_join_cpu.py: K16's keys, the sentinel's place in
// the sorted order, the rule that picks every distinct pair once and the row pointers, held to a model made of std::set on seeded
// random tables -- two lists and self-join, with junk cells, own indices, duplicates, empty rows in front, in the middle and at the
// end, and tables without a single pair; then the row-pointer fill they share with the other joins, exhaustively on small inputs
// (rows_fill_host.h).  Prints "k16_core_host ok <tables> <pairs> <row sequences>" and returns 0, or says what differs.
#include "../polyfuzz_amd/csrc/k16_core.h"
#include "rows_fill_host.h"

#include <algorithm>
#include <cstdio>
#include <random>
#include <set>
#include <utility>
#include <vector>

namespace {

int fail(const char *what, int seed, long long a, long long b)
{
    std::printf("k16_core_host: %s (table %d): %lld != %lld\n", what, seed, a, b);
    return 1;
}

// one table: n rows of m cells into a to-list of n_to (self: n_to == n); fill: the share of cells that hold an index
int one_table(int seed, int n, int m, int n_to, bool self, double fill, long long *pairs_out)
{
    std::mt19937 rng((unsigned)seed);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    const int32_t junk[4] = {-1, -7, n_to, INT32_MAX};
    std::vector<int32_t> cand((size_t)n * m);
    for (int i = 0; i < n; ++i) {
        const bool empty_row = u(rng) < 0.2 || (seed % 3 == 0 && (i < 2 || i >= n - 2));
        for (int k = 0; k < m; ++k) {
            int32_t v = junk[rng() % 4];
            if (!empty_row && u(rng) < fill) v = (int32_t)(rng() % (unsigned)n_to);
            if (!empty_row && k > 0 && u(rng) < 0.1) v = cand[(size_t)i * m + k - 1];      // a cell listed twice
            if (self && !empty_row && u(rng) < 0.05) v = i;                                   // the row's own index
            cand[(size_t)i * m + k] = v;
        }
    }
    // the model: rules of include/polyfuzz_hip.h on sets
    std::set<std::pair<int64_t, int64_t>> want;
    int64_t want_cells = 0;
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < m; ++k) {
            const int64_t j = cand[(size_t)i * m + k];
            if (j < 0 || j >= n_to || (self && j == i)) continue;
            ++want_cells;
            want.insert(self ? std::make_pair(std::min<int64_t>(i, j), std::max<int64_t>(i, j)) : std::make_pair((int64_t)i, j));
        }
    // the kernel's way
    const int64_t cells = (int64_t)n * m;
    std::vector<uint64_t> keys((size_t)cells);
    for (int64_t c = 0; c < cells; ++c) keys[(size_t)c] = pfz::pair_key(c / m, cand[(size_t)c], n_to, self);
    std::sort(keys.begin(), keys.end());
    std::vector<int32_t> seg((size_t)n + 1, -12345);
    std::vector<int> written((size_t)n + 1, 0);
    for (int64_t p = 0; p < cells; ++p) {
        std::vector<int32_t> before = seg;
        pfz::pair_rows_fill(keys.data(), p, cells, n, seg.data());
        for (int r = 0; r <= n; ++r) written[(size_t)r] += seg[(size_t)r] != before[(size_t)r];
    }
    for (int r = 0; r <= n; ++r)
        if (written[(size_t)r] != 1) return fail("a row pointer is not written exactly once", seed, r, written[(size_t)r]);
    if (seg[0] != 0) return fail("seg[0]", seed, seg[0], 0);
    if (seg[(size_t)n] != want_cells) return fail("cells that are a pair", seed, seg[(size_t)n], want_cells);
    for (int64_t p = seg[(size_t)n]; p < cells; ++p)
        if (keys[(size_t)p] != pfz::kPairKeyNone) return fail("a real key behind the sentinel", seed, p, (long long)keys[(size_t)p]);
    std::vector<std::pair<int64_t, int64_t>> got;
    for (int r = 0; r < n; ++r) {
        if (seg[(size_t)r] > seg[(size_t)r + 1]) return fail("row pointers descend", seed, seg[(size_t)r], seg[(size_t)r + 1]);
        for (int64_t p = seg[(size_t)r]; p < seg[(size_t)r + 1]; ++p) {
            if (pfz::pair_key_row(keys[(size_t)p], n) != r) return fail("a key in another row's range", seed, p, r);
            if (pfz::pair_key_first(keys.data(), p)) got.emplace_back(r, pfz::pair_key_to(keys[(size_t)p]));
        }
    }
    if (got.size() != want.size()) return fail("distinct pairs", seed, (long long)got.size(), (long long)want.size());
    if (!std::equal(got.begin(), got.end(), want.begin())) return fail("the pairs or their order", seed, 0, 1);
    *pairs_out += (long long)got.size();
    return 0;
}

}  // namespace

int main()
{
    // the packing itself: the sentinel sorts behind the largest real key, the self-join folds the two directions into one key
    const int64_t big = INT32_MAX;
    if (!(pfz::pair_key(big - 1, (int32_t)(big - 1), big, false) < pfz::kPairKeyNone)) return fail("largest key vs sentinel", -1, 0, 1);
    if (pfz::pair_key(5, 3, 10, true) != pfz::pair_key(3, 5, 10, true) || pfz::pair_key(5, 3, 10, true) != ((3ull << 32) | 5ull))
        return fail("self-join key", -1, 0, 1);
    if (pfz::pair_key(5, 3, 10, false) != ((5ull << 32) | 3ull)) return fail("two-list key", -1, 0, 1);
    if (pfz::pair_key(5, 5, 10, true) != pfz::kPairKeyNone || pfz::pair_key(5, 5, 10, false) == pfz::kPairKeyNone)
        return fail("own index", -1, 0, 1);
    if (pfz::pair_key(0, 10, 10, false) != pfz::kPairKeyNone || pfz::pair_key(0, -1, 10, false) != pfz::kPairKeyNone)
        return fail("outside the to-list", -1, 0, 1);
    long long pairs = 0;
    int tables = 0;
    for (int seed = 0; seed < 240; ++seed) {
        const bool self = seed % 2 == 0;
        const int n = 1 + seed % 37, m = 1 + (seed / 3) % 9;
        const int n_to = self ? n : 1 + (seed * 7) % 23;
        const double fill = seed % 5 == 4 ? 0.0 : 0.15 * (1 + seed % 5);      // (every fifth table has no pair at all)
        if (one_table(seed, n, m, n_to, self, fill, &pairs)) return 1;
        ++tables;
    }
    long long sequences = 0;
    if (const int bad = rows_fill_check<int32_t>(&sequences) + rows_fill_check<int64_t>(&sequences))
        return fail("row pointers of the small sequences against the counting loop", -1, bad, 0);
    std::printf("k16_core_host ok %d %lld %lld\n", tables, pairs, sequences);
    return 0;
}
