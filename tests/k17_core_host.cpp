// polyfuzz_amd/csrc/k17_core.h compiled for the host (tests/test_blocked_threshold_cpu.py): the item arithmetic of K17 over row
// pointers read from standard input -- "S n" and n + 1 row pointers -- printed for a numpy restatement to compare:
//   kPairSlice
//   the number of items, the bound pair_item_bound gives for them
//   one line "row p0 p1" per item, rows ascending, a row's slices in order
#include <cstdio>
#include <vector>

#include "../polyfuzz_amd/csrc/k17_core.h"

int main()
{
    long long S, n;
    if (scanf("%lld %lld", &S, &n) != 2 || n < 0) return 2;
    std::vector<long long> ptr((size_t)n + 1);
    for (auto &p : ptr)
        if (scanf("%lld", &p) != 1) return 2;
    long long items = 0;
    for (long long r = 0; r < n; ++r) items += pfz::pair_item_count(ptr[r + 1] - ptr[r], (int32_t)S);
    printf("%d\n%lld %lld\n", (int)pfz::kPairSlice, items, (long long)pfz::pair_item_bound(n, ptr[n] - ptr[0], (int32_t)S));
    for (long long r = 0; r < n; ++r) {
        const int32_t c = pfz::pair_item_count(ptr[r + 1] - ptr[r], (int32_t)S);
        for (int32_t k = 0; k < c; ++k) {
            const pfz::PairItem it = pfz::pair_item_slice((int32_t)r, ptr[r], ptr[r + 1], k, (int32_t)S);
            printf("%d %d %d\n", it.row, it.p0, it.p1);
        }
    }
    return 0;
}
