// polyfuzz_amd/csrc/k25_core.h compiled for the host (tests/test_simhash_cpu.py): the SimHash rule of K25 over commands read from
// standard input until its end, one answer line per command, for a Python restatement to compare:
//   C                              -> "mix(G) hash(abc) min_bits max_bits max_gram", the first two in hex
//   S lo hi clean rs bits n        followed by n code units in hex -> "fingerprint windows symbols": the packed bytes in hex, the number
//                                  of windows, and the symbols the analyzer kept as hex numbers joined by ',' ("-" for none) -- by the
//                                  kernel's own walk: steps of 63 / 64 units through the step functions the kernel calls
#include <cstdio>
#include <vector>

#include "../polyfuzz_amd/csrc/k25_core.h"

int main()
{
    char cmd;
    while (scanf(" %c", &cmd) == 1) {
        if (cmd == 'C') {
            uint64_t g = pfz::k25_window_begin();
            for (uint32_t c : {97u, 98u, 99u}) g = pfz::k25_window_feed(g, c);
            printf("%016llx %016llx %d %d %d\n", (unsigned long long)pfz::k25_window_begin(), (unsigned long long)g, pfz::kK25MinBits,
                   pfz::kK25MaxBits, pfz::kK25MaxGram);
        }
        else if (cmd == 'S') {
            int lo, hi, clean, rs, bits;
            long long n;
            if (scanf("%d %d %d %d %d %lld", &lo, &hi, &clean, &rs, &bits, &n) != 6) return 2;
            if (!pfz::k25_bits_ok(bits) || !pfz::k25_grams_ok(lo, hi) || n < 0) return 2;
            std::vector<uint32_t> units((size_t)n);      // exactly the string: the sanitizer sees a read behind it
            for (auto &u : units)
                if (scanf("%x", &u) != 1) return 2;
            const int words = bits / 64;
            std::vector<int32_t> ones((size_t)bits, 0);
            std::vector<uint32_t> symbols;
            int32_t windows = 0;
            // the kernel's walk, lane by lane: a line of exactly kK25Line words (the sanitizer sees a symbol too many), the step's masks,
            // the placement, the windows that end at every symbol, the carry
            std::vector<uint32_t> line((size_t)pfz::kK25Line, 0xDEADBEEFu);
            for (int l = 0; l < pfz::kK25Carry; ++l) line[(size_t)l] = pfz::kK25None;
            pfz::K25Flags flags;
            const long long step = clean ? pfz::kK25CleanStep : pfz::kK25RawStep;
            for (long long c0 = 0; c0 < n; c0 += step) {
                int n_step;
                if (clean) {
                    uint32_t cls[64];
                    uint64_t keepm = 0, spm = 0, esm = 0;
                    for (int l = 0; l < 64; ++l) {
                        cls[l] = l < step && c0 + l < n ? pfz::k25_clean_class(units[(size_t)(c0 + l)]) : pfz::kK25None;
                        if (cls[l] == pfz::kK25Space) spm |= 1ull << l;
                        else if (cls[l] != pfz::kK25None) keepm |= 1ull << l;
                    }
                    for (int l = 0; l < 64; ++l)
                        if ((keepm >> l & 1) && pfz::k25_space_before(keepm, spm, flags, l)) esm |= 1ull << l;
                    for (int l = 0; l < 64; ++l) {
                        if (!(keepm >> l & 1)) continue;
                        const int pos = pfz::k25_place(keepm, esm, l);
                        if (esm >> l & 1) line.at((size_t)(pfz::kK25Carry + pos - 1)) = pfz::kK25Space;
                        line.at((size_t)(pfz::kK25Carry + pos)) = cls[l];
                    }
                    n_step = pfz::k25_step_symbols(keepm, esm);
                    flags = pfz::k25_step_flags(keepm, spm, flags);
                }
                else {
                    n_step = (int)(n - c0 < step ? n - c0 : step);
                    for (int l = 0; l < n_step; ++l) line[(size_t)(pfz::kK25Carry + l)] = units[(size_t)(c0 + l)];
                }
                if (n_step > 64) return 3;
                for (int l = 0; l < n_step; ++l) {
                    const uint32_t *at = line.data() + pfz::kK25Carry + l;
                    if (*at == 0xDEADBEEFu) return 3;      // a symbol nobody wrote
                    symbols.push_back(*at);
                    const int run = pfz::k25_run_back(at, hi, rs != 0);
                    for (int nn = lo; nn <= hi && nn <= run; ++nn) {
                        const uint64_t g = pfz::k25_hash_back(at, nn);
                        ++windows;
                        for (int q = 0; q < words; ++q) {
                            const uint64_t word = pfz::k25_word(g, q);
                            for (int b = 0; b < 64; ++b) ones[(size_t)(64 * q + b)] += (int32_t)(word >> b & 1);
                        }
                    }
                }
                uint32_t keep[pfz::kK25Carry - 1];
                for (int k = 0; k < pfz::kK25Carry - 1; ++k) keep[k] = line.at((size_t)pfz::k25_carry_from(n_step, k));
                for (int k = 0; k < pfz::kK25Carry - 1; ++k) line[(size_t)(1 + k)] = keep[k];
                for (int l = pfz::kK25Carry; l < pfz::kK25Line; ++l) line[(size_t)l] = 0xDEADBEEFu;
            }
            for (int q = 0; q < words; ++q) {
                uint64_t mask = 0;
                for (int b = 0; b < 64; ++b) mask |= (uint64_t)(pfz::k25_vote_bit(ones[(size_t)(64 * q + b)], windows) ? 1 : 0) << b;
                for (int j = 0; j < 8; ++j) printf("%02x", pfz::k25_packed_byte(mask, j));
            }
            printf(" %d ", windows);
            if (symbols.empty()) printf("-");
            for (size_t t = 0; t < symbols.size(); ++t) printf("%s%x", t ? "," : "", symbols[t]);
            printf("\n");
        }
        else return 2;
    }
    return 0;
}
