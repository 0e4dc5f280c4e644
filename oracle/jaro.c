/*
 * oracle/jaro.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * The definition K8 is held to, in plain C: jellyfish's jaro_similarity /
 * jaro_winkler_similarity with their default arguments on Unicode code points,
 * restated from the docstring and body of tests/jaro_oracle.py (from-major, one
 * flag per character, float64 in the definition's order of operations):
 *     r = max(max(|a|, |b|) / 2 - 1, 0)
 *     every a[i], in order, takes the first unflagged j in [i - r, i + r] with b[j] == a[i];   m = pairs taken
 *     t = (k-th flagged character of a != k-th flagged character of b, counted over k) / 2     (integer division)
 *     w = (m / |a| + m / |b| + (m - t) / m) / 3;   0 when a string is empty or m = 0
 *     Winkler: if w > 0.7:  w = w + (l * 0.1) * (1 - w),  l = common prefix, at most 4
 * It shares nothing with polyfuzz_amd/csrc/k8_core.h (to-major, bit words, float32 bounds) -- the two are independent.
 * PARITY UNPINNED against jellyfish itself (not installable where this was written); tests/test_jaro_cpu.py holds this
 * file == tests/jaro_oracle.py and both to jellyfish wherever it is importable.
 *
 * Compiled with -ffp-contract=off: the Winkler step is a product and a sum (fused, its last bit differs).
 * Any length: the flags are allocated for the longest string of either list.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static double jaro_pair(const uint32_t *a, int64_t la, const uint32_t *b, int64_t lb, int winkler, uint8_t *flag_a, uint8_t *flag_b)
{
    if (la == 0 || lb == 0) return 0.0;                 /* also when both are empty */
    int64_t r = (la > lb ? la : lb) / 2 - 1;
    if (r < 0) r = 0;
    memset(flag_a, 0, (size_t)la);
    memset(flag_b, 0, (size_t)lb);
    int64_t m = 0;
    for (int64_t i = 0; i < la; ++i) {
        const int64_t lo = i - r > 0 ? i - r : 0, hi = i + r < lb - 1 ? i + r : lb - 1;
        const uint32_t c = a[i];
        for (int64_t j = lo; j <= hi; ++j) {
            if (b[j] == c && !flag_b[j]) {
                flag_a[i] = flag_b[j] = 1;
                ++m;
                break;
            }
        }
    }
    if (m == 0) return 0.0;
    int64_t differ = 0, j = 0;
    for (int64_t i = 0; i < la; ++i) {
        if (!flag_a[i]) continue;
        while (!flag_b[j]) ++j;                         /* (as many flags on either side) */
        differ += a[i] != b[j];
        ++j;
    }
    const int64_t t = differ / 2;
    const double dm = (double)m;
    double w = (dm / (double)la + dm / (double)lb + (double)(m - t) / dm) / 3.0;
    if (winkler && w > 0.7) {
        int64_t l = 0;
        while (l < la && l < lb && l < 4 && a[l] == b[l]) ++l;
        w = w + ((double)l * 0.1) * (1.0 - w);
    }
    return w;
}

static int alloc_flags(const int64_t *a_off, int64_t r0, int64_t r1, const int64_t *b_off, int64_t n_b, uint8_t **fa, uint8_t **fb)
{
    int64_t max_la = 0, max_lb = 0;
    for (int64_t i = r0; i < r1; ++i)
        if (a_off[i + 1] - a_off[i] > max_la) max_la = a_off[i + 1] - a_off[i];
    for (int64_t j = 0; j < n_b; ++j)
        if (b_off[j + 1] - b_off[j] > max_lb) max_lb = b_off[j + 1] - b_off[j];
    *fa = (uint8_t *)malloc((size_t)max_la + 1);
    *fb = (uint8_t *)malloc((size_t)max_lb + 1);
    if (!*fa || !*fb) {
        free(*fa);
        free(*fb);
        return -1;
    }
    return 0;
}

/* scorer: 0 = Jaro, 1 = Jaro-Winkler.  out: [(row_end - row_begin) * n_b], every pair's score. */
int oracle_jaro_matrix(const uint32_t *a_cp, const int64_t *a_off, int64_t n_a, const uint32_t *b_cp, const int64_t *b_off, int64_t n_b,
                       int32_t scorer, int64_t row_begin, int64_t row_end, double *out)
{
    uint8_t *fa, *fb;
    if ((scorer != 0 && scorer != 1) || row_begin < 0 || row_begin > row_end || row_end > n_a) return -2;
    if (alloc_flags(a_off, row_begin, row_end, b_off, n_b, &fa, &fb)) return -1;
    for (int64_t i = row_begin; i < row_end; ++i)
        for (int64_t j = 0; j < n_b; ++j)
            out[(i - row_begin) * n_b + j] =
                jaro_pair(a_cp + a_off[i], a_off[i + 1] - a_off[i], b_cp + b_off[j], b_off[j + 1] - b_off[j], scorer, fa, fb);
    free(fa);
    free(fb);
    return 0;
}

/*
 * The first maximum of every from-row over the choices its skip code leaves in (skip may be NULL: all of them):
 * skip[i] >= 0 leaves that choice out, skip[i] <= -2 every choice up to -2 - skip[i], -1 nothing
 * (tests/jaro_oracle.py left_out).  A row with no choice: -1 / 0.0.
 */
int oracle_jaro_argmax(const uint32_t *a_cp, const int64_t *a_off, int64_t n_a, const uint32_t *b_cp, const int64_t *b_off, int64_t n_b,
                       int32_t scorer, const int32_t *skip, int64_t row_begin, int64_t row_end, int32_t *out_idx, double *out_score)
{
    uint8_t *fa, *fb;
    if ((scorer != 0 && scorer != 1) || row_begin < 0 || row_begin > row_end || row_end > n_a) return -2;
    if (alloc_flags(a_off, row_begin, row_end, b_off, n_b, &fa, &fb)) return -1;
    for (int64_t i = row_begin; i < row_end; ++i) {
        const int64_t sk = skip ? skip[i] : -1;
        int32_t best = -1;
        double best_s = 0.0;
        for (int64_t j = 0; j < n_b; ++j) {
            if (j == sk || j <= -2 - sk) continue;
            const double s = jaro_pair(a_cp + a_off[i], a_off[i + 1] - a_off[i], b_cp + b_off[j], b_off[j + 1] - b_off[j], scorer, fa, fb);
            if (best < 0 || s > best_s) {
                best = (int32_t)j;
                best_s = s;
            }
        }
        out_idx[i - row_begin] = best;
        out_score[i - row_begin] = best_s;
    }
    free(fa);
    free(fb);
    return 0;
}
