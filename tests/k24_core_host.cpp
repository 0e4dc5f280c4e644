// polyfuzz_amd/csrc/k24_core.h compiled for the host (tests/test_hamming_index_cpu.py): the block-index rule of K24 over commands read
// from standard input until its end, one answer line (or block of lines) per command, for a numpy restatement to compare:
//   B d hmax              -> "indexable m narrowest widest lo_0 .. lo_m"  (not indexable: "0")
//   K d hmax n bytes      followed by n rows of `bytes` two-digit hex numbers -> n lines of m block keys
//   F m b                 followed by two rows of m keys -> "1" if the pair is reported in block b under the first-block rule, else "0"
//   R n_to m b key i self followed by m n_to ascending sort keys -> "p0 p1", the probe's run
//   C                     -> "max_blocks max_rows ratio slice"
#include <cstdio>
#include <vector>

#include "../polyfuzz_amd/csrc/k24_core.h"

int main()
{
    char cmd;
    while (scanf(" %c", &cmd) == 1) {
        if (cmd == 'C') {
            printf("%d %lld %lld %d\n", (int)pfz::kK24MaxBlocks, (long long)pfz::kK24MaxRows, (long long)pfz::kK24AutoRatio, (int)pfz::kPairSlice);
        }
        else if (cmd == 'B') {
            long long d, hmax;
            if (scanf("%lld %lld", &d, &hmax) != 2) return 2;
            if (!pfz::k24_indexable(d, hmax)) {
                printf("0\n");
                continue;
            }
            const long long m = hmax + 1;
            printf("1 %lld %d %d", m, pfz::k24_block_min(d, m), pfz::k24_block_max(d, m));
            for (long long b = 0; b <= m; ++b) printf(" %d", pfz::k24_block_lo(d, m, b));
            printf("\n");
        }
        else if (cmd == 'K') {
            long long d, hmax, n, bytes;
            if (scanf("%lld %lld %lld %lld", &d, &hmax, &n, &bytes) != 4 || !pfz::k24_indexable(d, hmax) || 8 * bytes < d) return 2;
            const long long m = hmax + 1;
            std::vector<uint8_t> row((size_t)bytes);      // exactly the row: the sanitizer sees a read behind it
            for (long long r = 0; r < n; ++r) {
                for (auto &x : row) {
                    unsigned v;
                    if (scanf("%2x", &v) != 1) return 2;
                    x = (uint8_t)v;
                }
                for (long long b = 0; b < m; ++b)
                    printf("%u%c", pfz::k24_block_key(row.data(), pfz::k24_block_lo(d, m, b), pfz::k24_block_lo(d, m, b + 1)), b + 1 < m ? ' ' : '\n');
            }
        }
        else if (cmd == 'F') {
            long long m, b;
            if (scanf("%lld %lld", &m, &b) != 2 || b >= m) return 2;
            std::vector<uint32_t> ka((size_t)m), kb((size_t)m);
            for (auto &x : ka)
                if (scanf("%u", &x) != 1) return 2;
            for (auto &x : kb)
                if (scanf("%u", &x) != 1) return 2;
            printf("%d\n", pfz::k24_first_block(ka.data(), kb.data(), (int32_t)b) ? 1 : 0);
        }
        else if (cmd == 'R') {
            long long n_to, m, b, key, i, self;
            if (scanf("%lld %lld %lld %lld %lld %lld", &n_to, &m, &b, &key, &i, &self) != 6) return 2;
            std::vector<uint64_t> s((size_t)(n_to * m));
            for (auto &x : s) {
                unsigned long long v;
                if (scanf("%llu", &v) != 1) return 2;
                x = v;
            }
            int64_t p0, p1;
            pfz::k24_probe_run(s.data(), n_to, (int32_t)b, (uint32_t)key, (int32_t)i, self != 0, &p0, &p1);
            printf("%lld %lld\n", (long long)p0, (long long)p1);
        }
        else return 2;
    }
    return 0;
}
