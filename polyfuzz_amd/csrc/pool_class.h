// The caching allocator's size classes and fill patterns (pfz_api.hip: pool_alloc_raw, pfz_pool_fill).  Plain integer C++,
// compiled into the library and into a host program that sweeps it on the CPU (tests/pool_class_host.cpp).
//
// A request is rounded up to 512 bytes, or to the next of p2, 1.25, 1.5, 1.75, 2 x p2 (p2 the power of two at or below it): at
// most 25 % is lost, and every class is a multiple of 8 bytes -- which the fill of pfz_pool_fill relies on: it writes whole
// 64-bit words over the whole class.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace pfz {

inline size_t size_class(size_t bytes)
{
    if (bytes < 512) return 512;
    size_t p2 = 512;
    while (p2 * 2 <= bytes) p2 *= 2;       // p2 <= bytes < 2*p2
    for (int j = 0; j <= 4; ++j) {
        const size_t c = p2 + (p2 / 4) * j;  // p2, 1.25, 1.5, 1.75, 2 x p2
        if (c >= bytes) return c;
    }
    return p2 * 2;
}

// pfz_pool_fill's modes (include/polyfuzz_hip.h) and the 64-bit little-endian word each writes
constexpr int32_t kPoolFillOff = 0, kPoolFillZero = 1, kPoolFillOne64 = 2, kPoolFillOne32 = 3;

inline bool pool_fill_mode_ok(int32_t mode) { return mode >= kPoolFillOff && mode <= kPoolFillOne32; }

inline uint64_t pool_fill_word(int32_t mode)
{
    return mode == kPoolFillOne64 ? 0x0000000000000001ull : mode == kPoolFillOne32 ? 0x0000000100000001ull : 0ull;
}

}  // namespace pfz
