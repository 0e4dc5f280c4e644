// polyfuzz_amd/csrc/k8_core.h -- what a fixed threshold lets a K20 lane leave out -- compiled for the host:
//   k20_host_dismissals   every dismissal against jaro_score, exhaustively over lengths, matches, transpositions and prefixes;
//   k20_host_pairs        the whole decision on one pair as the register kernel takes it (sweep 1 with the abandon rule once per
//                         packed dword, the bound with the pair's prefix, sweep 2, the bound with t, the float64 score), in both word
//                         widths, a to-string in up to four stretches of the word;
//   k20_host_len_ok / k20_host_len_run   the length bound and the run the set-up launch finds with it.
// tests/test_jaro_join_cpu.py compares with the definition (tests/jaro_oracle.py).
#include <stddef.h>
#include <vector>

#include "../polyfuzz_amd/csrc/k8_core.h"

using namespace pfz;

// For every la, lb <= max_len, both scorers and every threshold: whenever the length bound, m_need, the abandon rule (at every
// split of flagged / remaining) or one of the two bounds behind the sweeps dismisses, jaro_score < t must hold for every (m, t-count,
// prefix) it dismisses; the run of jaro_len_run must be the lb that jaro_len_ok admits; at t == 0 nothing is dismissed.
// Returns the number of violations; dismissed[k]: how many (la, lb, m, t-count, prefix) threshold k dismissed by any rule.
extern "C" int64_t k20_host_dismissals(int32_t max_len, int32_t n_thr, const double *thr, int64_t *dismissed)
{
    int64_t bad = 0;
    for (int k = 0; k < n_thr; ++k) {
        const double t = thr[k];
        const float t32 = (float)t;
        dismissed[k] = 0;
        for (int winkler = 0; winkler < 2; ++winkler)
            for (int la = 0; la <= max_len; ++la) {
                int run_lo, run_hi;
                jaro_len_run(la, max_len, t32, winkler, &run_lo, &run_hi);
                for (int lb = 0; lb <= max_len; ++lb) {
                    const int mn = la < lb ? la : lb;
                    const float inv_la = 1.0f / (float)la, inv_lb = 1.0f / (float)lb;      // (inf for an empty string, as the kernel's)
                    const bool len_ok = jaro_len_ok(la, lb, t32, winkler);
                    bad += len_ok != (lb >= run_lo && lb <= run_hi);
                    const int need = jaro_m_need(la, lb, inv_la, inv_lb, t32, winkler);
                    if (t == 0.0) bad += !len_ok || need != 0;
                    int m_first_hit = mn + 1;                 // the fewest matches any hit of these lengths has
                    for (int m = 0; m <= mn; ++m)
                        for (int tc = 0; tc <= m / 2; ++tc)
                            for (int prefix = 0; prefix <= jaro_min3(4, la, lb); ++prefix) {
                                const bool hit = jaro_score(m, 2 * tc, la, lb, prefix, winkler) >= t;
                                bad += jaro_score(m, 2 * tc + 1, la, lb, prefix, winkler) != jaro_score(m, 2 * tc, la, lb, prefix, winkler);
                                if (hit && m < m_first_hit) m_first_hit = m;
                                const bool after1 = jaro_reaches(m, inv_la, inv_lb, 1.0f, prefix, winkler, t32);
                                const float last = (float)(m - tc) * (1.0f / (float)m);
                                const bool after2 = jaro_reaches(m, inv_la, inv_lb, last, prefix, winkler, t32);
                                const bool out = !len_ok || m < need || !after1 || !after2;
                                bad += out && hit;
                                bad += t == 0.0 && out;
                                dismissed[k] += out;
                            }
                    // the abandon rule: `flagged` so far, `remaining` to come -- the pair ends with m <= min(la, flagged + remaining)
                    for (int flagged = 0; flagged <= mn; ++flagged)
                        for (int remaining = 0; remaining <= lb; ++remaining) {
                            const int most = jaro_min3(la, lb, flagged + remaining);
                            if (jaro_dead(la, flagged, remaining, need)) bad += m_first_hit <= most || t == 0.0;
                        }
                }
            }
    }
    return bad;
}

// PER: to-characters per packed dword (4 or 2), the abandon rule's stride.  out_hit: 1 = hit, 0 = miss; out_score: the float64
// score of a pair that was scored (a hit always is), -1.0 of one that was dismissed; out_stage[4]: pairs that passed the length
// bound, sweep 1, the bound with the prefix, the bound with t.
template <typename WORD, int NB>
static int pairs(int per, int64_t n_a, const int32_t *a_sym, const int64_t *a_off, int64_t n_b, const int32_t *b_sym, const int64_t *b_off,
                 int32_t n_sym1, int32_t winkler, double t, uint8_t *out_hit, double *out_score, int64_t *out_stage)
{
    constexpr int WB = (int)sizeof(WORD) * 8;
    const float t32 = (float)t;
    std::vector<WORD> pm((size_t)n_sym1);
    for (int k = 0; k < 4; ++k) out_stage[k] = 0;
    for (int64_t i = 0; i < n_a; ++i) {
        const int la = (int)(a_off[i + 1] - a_off[i]);
        if (la > WB) return 1;
        pm.assign((size_t)n_sym1, 0);
        for (int p = 0; p < la; ++p)
            if (a_sym[a_off[i] + p]) pm[(size_t)a_sym[a_off[i] + p]] |= (WORD)1 << p;
        const float inv_la = 1.0f / (float)la;
        for (int64_t k = 0; k < n_b; ++k) {
            const int lb = (int)(b_off[k + 1] - b_off[k]);
            if (lb > NB * WB) return 1;
            const int32_t *b = b_sym + b_off[k];
            uint8_t *hit = out_hit + i * n_b + k;
            double *score = out_score + i * n_b + k;
            *hit = 0;
            *score = -1.0;
            bool alive = jaro_len_ok(la, lb, t32, winkler);
            if (!alive) continue;
            ++out_stage[0];
            const float inv_lb = 1.0f / (float)lb;
            const int need = jaro_m_need(la, lb, inv_la, inv_lb, t32, winkler);
            const int steps = (lb + per - 1) / per * per;      // whole packed dwords: padding symbols, whose table entry is empty
            JaroFlags<WORD> s;
            WORD fb[NB];
            jaro_begin(s, jaro_range(la, lb));
            for (int kb = 0; kb < NB; ++kb) {
                s.fb = 0;
                for (int j = kb * WB; alive && j < (steps < (kb + 1) * WB ? steps : (kb + 1) * WB); ++j) {
                    jaro_match<WORD>(s, j < lb ? pm[(size_t)b[j]] : 0, j, j - kb * WB);
                    const int done = j + 1;
                    if (done % per == 0 && done < lb && jaro_dead(la, __builtin_popcountll(s.fa), lb - done, need)) alive = false;
                }
                fb[kb] = s.fb;
            }
            if (!alive) continue;
            ++out_stage[1];
            const int m = __builtin_popcountll(s.fa);
            const int prefix = jaro_prefix(s.pre);
            if (!jaro_reaches(m, inv_la, inv_lb, 1.0f, prefix, winkler, t32)) continue;
            ++out_stage[2];
            int half_t = 0;
            if (m >= 2)
                for (int kb = 0; kb < NB; ++kb) {
                    s.fb = fb[kb];
                    for (int j = kb * WB; j < (steps < (kb + 1) * WB ? steps : (kb + 1) * WB); ++j)
                        half_t += jaro_transpose<WORD>(s, j < lb ? pm[(size_t)b[j]] : 0, j - kb * WB);
                }
            const float last = (float)(m - half_t / 2) * (1.0f / (float)m);
            if (!jaro_reaches(m, inv_la, inv_lb, last, prefix, winkler, t32)) continue;
            ++out_stage[3];
            *score = jaro_score(m, half_t, la, lb, prefix, winkler);
            *hit = *score >= t;
        }
    }
    return 0;
}

// word_bits: 32 (from <= 32 x to <= 32) or 64 (from <= 64 x to <= 256), the register kernels' two classes
extern "C" int k20_host_pairs(int32_t word_bits, int32_t per, int64_t n_a, const int32_t *a_sym, const int64_t *a_off, int64_t n_b,
                              const int32_t *b_sym, const int64_t *b_off, int32_t n_sym1, int32_t winkler, double t, uint8_t *out_hit,
                              double *out_score, int64_t *out_stage)
{
    return word_bits == 32 ? pairs<uint32_t, 1>(per, n_a, a_sym, a_off, n_b, b_sym, b_off, n_sym1, winkler, t, out_hit, out_score, out_stage)
                           : pairs<uint64_t, 4>(per, n_a, a_sym, a_off, n_b, b_sym, b_off, n_sym1, winkler, t, out_hit, out_score, out_stage);
}

extern "C" int k20_host_len_ok(int32_t la, int32_t lb, double t, int32_t winkler) { return jaro_len_ok(la, lb, (float)t, winkler); }

extern "C" void k20_host_len_run(int32_t la, int32_t lb_max, double t, int32_t winkler, int32_t *lo, int32_t *hi)
{
    jaro_len_run(la, lb_max, (float)t, winkler, lo, hi);
}
