// K25's rule (k25_simhash.hip): the character-n-gram SimHash fingerprint of a string.
//
//   symbols     the string's code points as uint32; with `clean` (1-byte code units only) the sequence TFIDF's analyzer keeps:
//               lower-cased, only [a-z0-9 ], runs of ' ' collapsed, no ' ' at either end (the step functions below -- K1's rule, k_extract of
//               k1_vectorize.hip, restated on code points instead of alphabet ranks).
//   windows     for every n in lo .. hi every run of n consecutive symbols; with remove_space the windows that hold a ' ' are dropped.
//               Every occurrence counts.
//   hash        g = mix(G); g = mix(g ^ c) for the window's symbols in order.  Word 0 of the window's hash is g, word q >= 1 is
//               mix(g + q G): 64 W bits for a fingerprint of W words.  mix is the finaliser of splitmix64.
//   votes       V[64 q + b] = sum over the windows of +1 where bit b (least significant = 0) of word q is set, else -1; the
//               fingerprint's bit 64 q + b is V > 0 (a tie gives 0).  With `ones` windows that set the bit out of `windows`, V =
//               2 ones - windows: the kernel counts the ones.
//   layout      np.packbits order: bit k of a fingerprint is bit 7 - k % 8 of byte k / 8, so byte j of word q's eight is the
//               bit-reversed byte j of the 64-bit mask whose bit b is fingerprint bit 64 q + b.
//   no window   an all-zero fingerprint; such a string is nobody's partner (it gets no row in the operand handle).
//
// Plain integer C++, compiled for the device and for a host program that holds it to a Python restatement (tests/k25_core_host.cpp).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define K25_HD __host__ __device__ inline
#else
#define K25_HD inline
#endif

namespace pfz {

constexpr uint64_t kK25Golden = 0x9E3779B97F4A7C15ull;
constexpr int32_t kK25MinBits = 64, kK25MaxBits = 1024;      // whole 64-bit words
constexpr int32_t kK25MaxGram = 8;                           // 1 <= lo <= hi <= 8
constexpr uint32_t kK25Space = 0x20u;
constexpr uint32_t kK25None = 0xFFFFFFFFu;                   // no code point: "nothing here" in a symbol line, ends every window

K25_HD bool k25_bits_ok(int64_t bits) { return bits >= kK25MinBits && bits <= kK25MaxBits && bits % 64 == 0; }
K25_HD bool k25_grams_ok(int64_t lo, int64_t hi) { return 1 <= lo && lo <= hi && hi <= kK25MaxGram; }

K25_HD uint64_t k25_mix(uint64_t z)
{
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// the hash of a window: k25_window_begin(), then k25_window_feed() with each symbol in order
K25_HD uint64_t k25_window_begin() { return k25_mix(kK25Golden); }
K25_HD uint64_t k25_window_feed(uint64_t g, uint32_t symbol) { return k25_mix(g ^ (uint64_t)symbol); }
// word q of the hash whose word 0 is g
K25_HD uint64_t k25_word(uint64_t g, int32_t q) { return q == 0 ? g : k25_mix(g + (uint64_t)q * kK25Golden); }

// a symbol that no window may hold
K25_HD bool k25_breaks(uint32_t symbol, bool remove_space) { return symbol == kK25None || (remove_space && symbol == kK25Space); }

// the bit of a vote: `ones` of `windows` windows set it
K25_HD bool k25_vote_bit(int32_t ones, int32_t windows) { return 2 * (int64_t)ones > (int64_t)windows; }

// byte j (0 .. 7) of the eight a fingerprint word occupies; bit b of `mask` is the word's bit b
K25_HD uint8_t k25_packed_byte(uint64_t mask, int32_t j)
{
    uint32_t v = (uint32_t)(mask >> (8 * j)) & 0xffu, r = 0;
    for (int32_t t = 0; t < 8; ++t) r |= ((v >> t) & 1u) << (7 - t);
    return (uint8_t)r;
}

// ---- the cleaning rule on 1-byte code units ------------------------------------------------------------------------------------
// what one code unit is: kK25None = dropped, ' ' = a space, else the kept symbol (the lower-cased letter or the digit)
K25_HD uint32_t k25_clean_class(uint32_t c)
{
    if (c >= 'A' && c <= 'Z') c += 32;
    if (c == kK25Space) return kK25Space;
    return (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9') ? c : kK25None;
}

// ---- one step of the wave's walk over a string --------------------------------------------------------------------------------
// A step takes kK25CleanStep code units when it cleans, 64 when it does not, and leaves at most 64 symbols: a ' ' is put in front of a
// kept character when a space lies between it and the kept character before, and every such ' ' but one stands for a space unit of
// the step itself -- the one is the space pending from the steps before (`pend`), which is why a cleaning step takes 63 units.  The
// symbols go to a line of kK25Line words: line[kK25Carry + k] is symbol k of the step, the kK25Carry words in front hold the symbols
// before the step (the last kK25MaxGram - 1 are all a window can reach back to; line[0] is never read).
// Everything below is a pure function of the step's two masks (bit l: unit l is kept / is a space), the two flags and a lane number;
// the kernel gets the masks from ballots and calls the functions per lane, the host program loops over the lanes.
constexpr int32_t kK25CleanStep = 63, kK25RawStep = 64;
constexpr int32_t kK25Carry = 8;
constexpr int32_t kK25Line = kK25Carry + 64;

struct K25Flags {
    bool pend = false;      // a space since the last kept character
    bool any = false;       // a kept character so far
};

K25_HD int32_t k25_popc(uint64_t m) { return (int32_t)__builtin_popcountll(m); }
K25_HD int32_t k25_top(uint64_t m) { return 63 - (int32_t)__builtin_clzll(m); }      // m != 0
K25_HD uint64_t k25_below(int32_t lane) { return (1ull << lane) - 1ull; }

// unit `lane` is kept: does a ' ' go in front of it?
K25_HD bool k25_space_before(uint64_t keepm, uint64_t spm, K25Flags f, int32_t lane)
{
    const uint64_t kb = keepm & k25_below(lane);                                    // kept units before this one
    if (kb == 0ull) return f.any && (f.pend || (spm & k25_below(lane)) != 0ull);    // the step's first kept unit (never the string's first)
    const int32_t q = k25_top(kb);                                                  // the nearest kept unit before
    return (spm & k25_below(lane) & ~((2ull << q) - 1ull)) != 0ull;                 // a space in (q, lane)
}
// ... and its place among the step's symbols; esm: the lanes whose unit gets a ' ' in front (the ' ' itself goes to place - 1)
K25_HD int32_t k25_place(uint64_t keepm, uint64_t esm, int32_t lane)
{
    return k25_popc(keepm & k25_below(lane)) + k25_popc(esm & (k25_below(lane) | (1ull << lane)));
}
K25_HD int32_t k25_step_symbols(uint64_t keepm, uint64_t esm) { return k25_popc(keepm) + k25_popc(esm); }
// the flags behind the step
K25_HD K25Flags k25_step_flags(uint64_t keepm, uint64_t spm, K25Flags f)
{
    K25Flags g;
    if (keepm) {
        const int32_t last = k25_top(keepm);
        g.pend = last < 63 && (spm >> (last + 1)) != 0ull;
        g.any = true;
    } else {
        g.any = f.any;
        g.pend = f.any && (f.pend || spm != 0ull);
    }
    return g;
}

// The windows that end at one symbol; `at` points at it in the line (at[-j]: the symbol j places back, j < kK25MaxGram).
// the symbols ending here without a break, at most hi: a window of n symbols ends here iff n <= this
template <class Ptr> K25_HD int32_t k25_run_back(Ptr at, int32_t hi, bool remove_space)
{
    int32_t run = 0;
    bool open = true;
    for (int32_t j = 0; j < hi; ++j) {
        open = open && !k25_breaks(at[-j], remove_space);
        run += open ? 1 : 0;
    }
    return run;
}
// word 0 of the hash of the window of n symbols that ends here
template <class Ptr> K25_HD uint64_t k25_hash_back(Ptr at, int32_t n)
{
    uint64_t g = k25_window_begin();
    for (int32_t t = n - 1; t >= 0; --t) g = k25_window_feed(g, at[-t]);
    return g;
}
// what word 1 + k (k < kK25Carry - 1) of the line holds behind a step of n_step symbols: the last 7 of (carry, step)
K25_HD int32_t k25_carry_from(int32_t n_step, int32_t k) { return 1 + n_step + k; }

}  // namespace pfz
