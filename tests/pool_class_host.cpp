// polyfuzz_amd/csrc/pool_class.h on the host: the allocator's size classes over a sweep of request sizes -- every class a multiple
// of 8 bytes (pfz_pool_fill writes whole 64-bit words over the whole class), at least the request, at most 25 % above it from 512
// bytes on, non-decreasing in the request, and a class of its own members -- and the three fill words.  Prints
// "pool_class_host ok <sizes checked> <distinct classes>".
#include <stdio.h>
#include <stdlib.h>

#include <set>

#include "../polyfuzz_amd/csrc/pool_class.h"

#define REQUIRE(c)                                                                        \
    do {                                                                                  \
        if (!(c)) {                                                                       \
            fprintf(stderr, "pool_class_host: %s failed at line %d\n", #c, __LINE__);     \
            exit(1);                                                                      \
        }                                                                                 \
    } while (0)

static size_t g_checked = 0;
static std::set<size_t> g_classes;

static void check(size_t bytes)
{
    const size_t c = pfz::size_class(bytes);
    REQUIRE(c % 8 == 0);
    REQUIRE(c >= bytes && c >= 512);
    if (bytes >= 512) REQUIRE(c - bytes <= bytes / 4);      // at most 25 % lost
    REQUIRE(pfz::size_class(c) == c);                         // a class is its own class
    if (bytes > 0) REQUIRE(pfz::size_class(bytes - 1) <= c);  // non-decreasing
    g_classes.insert(c);
    ++g_checked;
}

int main()
{
    for (size_t b = 0; b <= (size_t)1 << 16; ++b) check(b);                       // every size up to 64 KiB
    for (int s = 9; s < 46; ++s) {                                                // around every class border up to 32 TiB
        const size_t p2 = (size_t)1 << s;
        for (int j = 0; j < 4; ++j) {
            const size_t edge = p2 + (p2 / 4) * j;
            for (long d = -9; d <= 9; ++d) check(edge + d);
        }
    }
    unsigned long long x = 88172645463325252ull;                                  // xorshift: sizes all over 44 bits
    for (int k = 0; k < 200000; ++k) {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        check((size_t)(x >> (20 + k % 40)));
    }
    REQUIRE(pfz::size_class(0) == 512 && pfz::size_class(512) == 512 && pfz::size_class(513) == 640);
    REQUIRE(pfz::size_class(1025) == 1280 && pfz::size_class(2048) == 2048 && pfz::size_class(1793) == 2048);
    REQUIRE(pfz::pool_fill_word(1) == 0x0000000000000000ull && pfz::pool_fill_word(2) == 0x0000000000000001ull);
    REQUIRE(pfz::pool_fill_word(3) == 0x0000000100000001ull);
    REQUIRE(pfz::pool_fill_mode_ok(0) && pfz::pool_fill_mode_ok(3) && !pfz::pool_fill_mode_ok(4) && !pfz::pool_fill_mode_ok(-1));
    printf("pool_class_host ok %zu %zu\n", g_checked, g_classes.size());
    return 0;
}
