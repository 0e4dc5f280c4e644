// polyfuzz_amd/csrc/k18_core.h on the CPU: the packed hit, the hit rule and the prune rule of the threshold join over K7's scorers,
// for tests/test_fuzz_join_cpu.py (a shared library, called through ctypes).  With -DK18_HOST_MAIN the same file is a program of
// its own that walks the borders once and returns 0 -- what a sanitizer build (-fsanitize=address,undefined) runs.
#include "../polyfuzz_amd/csrc/k18_core.h"

#include <cmath>
#include <cstdio>

using namespace pfz;

extern "C" {

uint64_t k18_host_pack(int32_t row, int32_t col) { return fuzz_key_pack(row, col); }
int32_t k18_host_row(uint64_t key) { return fuzz_key_row(key); }
int32_t k18_host_col(uint64_t key) { return fuzz_key_col(key); }
int k18_host_hit(double score, double cutoff) { return fuzz_join_hit(score, cutoff) ? 1 : 0; }
int k18_host_go(float upper_bound, double cutoff) { return fuzz_join_go(upper_bound, cutoff) ? 1 : 0; }
float k18_host_slack(void) { return kFuzzJoinSlack; }
int64_t k18_host_max_capacity(void) { return kFuzzJoinMaxCapacity; }

}  // extern "C"

#ifdef K18_HOST_MAIN
int main()
{
    int bad = 0;
    const int32_t edge[] = {0, 1, (1 << 26) - 1, 0x7fffffff};
    for (int32_t r : edge)
        for (int32_t c : edge) {
            const uint64_t k = fuzz_key_pack(r, c);
            bad += fuzz_key_row(k) != r || fuzz_key_col(k) != c;
        }
    // keys sort by (row, col)
    bad += !(fuzz_key_pack(0, (1 << 26) - 1) < fuzz_key_pack(1, 0));
    const double s = 85.5;
    const double cut[] = {0.0, std::nextafter(s, -INFINITY), s, std::nextafter(s, INFINITY), 100.0};
    const int want_hit[] = {1, 1, 1, 0, 0};
    for (int k = 0; k < 5; ++k) {
        bad += (fuzz_join_hit(s, cut[k]) ? 1 : 0) != want_hit[k];
        bad += want_hit[k] && !fuzz_join_go((float)s, cut[k]);      // a hit is never pruned by a bound that holds
    }
    bad += fuzz_join_go((float)(s - 1.0), s);                        // a bound a whole point below the cutoff prunes
    std::printf("k18_core_host: %d violations\n", bad);
    return bad != 0;
}
#endif
