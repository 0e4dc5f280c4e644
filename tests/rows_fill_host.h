// The shared row-pointer fill (polyfuzz_amd/csrc/k11_core.h rows_fill) held to a counting loop on the host, for the two host
// programs that include it (k11_core_host.cpp, k16_core_host.cpp): every ascending sequence of `total` = 1 .. 5 rows over n_rows =
// 0 .. 4 rows -- rows without a hit in front, in the middle and at the end among them, and the row "n_rows" of K16's keys that are
// no pair -- with the pointers in PTR's width.  Returns the number of (sequence, pointer) mismatches and adds the sequences to *cases.
#pragma once

#include "../polyfuzz_amd/csrc/k11_core.h"

#include <stddef.h>
#include <vector>

template <typename PTR> inline int rows_fill_check(long long *cases)
{
    int bad = 0;
    for (int n_rows = 0; n_rows <= 4; ++n_rows)
        for (int total = 1; total <= 5; ++total) {
            int rows[5] = {0, 0, 0, 0, 0};                // the first `total`: ascending, each in 0 .. n_rows
            for (;;) {
                std::vector<PTR> got((size_t)n_rows + 1, (PTR)-77);
                std::vector<int> written((size_t)n_rows + 1, 0);
                for (int p = 0; p < total; ++p) {
                    const std::vector<PTR> before = got;
                    pfz::rows_fill<PTR>(p > 0 ? rows[p - 1] : -1, rows[p], p, total, n_rows, got.data());
                    for (int r = 0; r <= n_rows; ++r) written[(size_t)r] += got[(size_t)r] != before[(size_t)r];
                }
                for (int r = 0; r <= n_rows; ++r) {
                    long long want = 0;                    // the reference: the hits in the rows before r, counted
                    for (int p = 0; p < total; ++p) want += rows[p] < r;
                    bad += (long long)got[(size_t)r] != want || written[(size_t)r] != 1;
                }
                ++*cases;
                int k = total - 1;                         // the next ascending sequence
                while (k >= 0 && rows[k] == n_rows) --k;
                if (k < 0) break;
                const int v = rows[k] + 1;
                for (int q = k; q < total; ++q) rows[q] = v;
            }
        }
    return bad;
}
