// The launches of an all-pairs Jaro call over K4's to-side plan, planned once for K8 (k8_jaro.hip: a best per row) and K21
// (k21_jaro_topn.hip: a list per wave): which from-rows the register kernels serve and against which groups, into how many parts
// a row's groups are split, and where a launch leaves what it found for its rows; and what every Jaro entry -- K20's
// (k20_jaro_join.hip) too -- checks before it plans.  Host code only.
#pragma once

#include "edit_walk.h"

#include <algorithm>
#include <vector>

namespace pfz {

// one register launch: rows [row0, row0 + n_rows) of rows_reg against the groups [g_begin, g_end) in 32-bit (wide: 64-bit) words;
// part p of a row leaves its result in slot slot0 + p of the row.  parts == 0: the launch is not made
struct JaroRegLaunch {
    size_t row0, n_rows;
    int32_t g_begin, g_end;
    bool wide;
    int32_t parts, slot0;
};

struct JaroPlan {
    int32_t n_groups, g32, g256;         // the groups are sorted by length: the first g32 / g256 hold to-strings of <= 32 / <= 256 characters only
    std::vector<int32_t> rows_reg;       // the register kernels' rows: the n32 of <= 32 characters first, then those of 33 .. 64
    size_t n32;
    std::vector<int32_t> rows_long;      // the general kernel's alone; `longest` of them
    int64_t longest;
    int64_t max_grid;
    JaroRegLaunch reg[3];                // <= 32 x groups <= 32;  <= 32 x groups 33 .. 256;  33 .. 64 x groups <= 256
    int32_t parts_long;                  // the parts of a row of rows_long (the general kernel over every group)
    int32_t n_slots;                     // K8's records per row: the register launches' parts, then one for the general kernel
    bool general_behind_reg() const { return !rows_reg.empty() && g256 < n_groups; }      // rows_reg against the groups beyond 256
};

// what every Jaro entry refuses before it plans: positions (padded to groups of 64) and lengths are 32-bit
inline int jaro_check_limits(const char *entry, const pfz_strings *F, const pfz_strings *T)
{
    if (T->n >= INT_MAX - 64 || F->n >= INT_MAX || T->max_len >= INT_MAX / 2 || F->max_len >= INT_MAX / 2) {
        set_error("%s: list or string too long", entry);
        return PFZ_ERR_UNSUPPORTED;
    }
    return PFZ_OK;
}

inline int jaro_check_scorer(const char *entry, int32_t scorer)
{
    PFZ_REQUIRE(scorer == 0 || scorer == 1, "%s: scorer %d is neither 0 (Jaro) nor 1 (Jaro-Winkler)", entry, scorer);
    return PFZ_OK;
}

// the groups are sorted by length: the first whole_groups_up_to(T, pl, len) of them hold to-strings of <= len characters only
inline int32_t whole_groups_up_to(const pfz_strings *T, const pfz_indel_plan *pl, int64_t len)
{
    int64_t n = 0;
    for (int64_t j = 0; j < T->n; ++j) n += T->h_off[(size_t)j + 1] - T->h_off[(size_t)j] <= len;
    return n == T->n ? (int32_t)pl->n_groups : (int32_t)(n / 64);
}

// The register kernel's share, while the match table fits 60 KiB of LDS: from-strings of <= 32 characters against the groups whose
// to-strings all have <= 32 in 32-bit words; those from-strings against the groups of up to 256, and the from-strings of 33 .. 64
// characters against all groups of up to 256, in 64-bit words (four for a to-string's flags).  Few from-strings: the to-groups of
// each are split over `parts` workgroups (K4's rule: >= 4 rounds of work units on the chip, each part at least one group per wave).
inline JaroPlan jaro_plan(const pfz_ctx *ctx, const pfz_strings *F, const pfz_strings *T, const pfz_indel_plan *pl, int64_t begin, int64_t end)
{
    JaroPlan P;
    const bool lds_fits = lds_table_fits(pl);
    P.n_groups = (int32_t)pl->n_groups;
    P.g32 = lds_fits ? whole_groups_up_to(T, pl, 32) : 0;
    P.g256 = lds_fits ? whole_groups_up_to(T, pl, 256) : 0;
    std::vector<int32_t> rows_64;
    P.longest = 1;
    for (int64_t i = begin; i < end; ++i) {
        const int64_t la = F->h_off[(size_t)i + 1] - F->h_off[(size_t)i];
        if (la <= 32 && P.g256 > 0) P.rows_reg.push_back((int32_t)i);
        else if (la <= 64 && P.g256 > 0) rows_64.push_back((int32_t)i);
        else {
            P.rows_long.push_back((int32_t)i);
            P.longest = std::max(P.longest, la);
        }
    }
    P.n32 = P.rows_reg.size();
    P.rows_reg.insert(P.rows_reg.end(), rows_64.begin(), rows_64.end());

    P.max_grid = (int64_t)ctx->prop.multiProcessorCount * 8;
    const JaroRegLaunch reg[3] = {{0, P.n32, 0, P.g32, false, 1, 0}, {0, P.n32, P.g32, P.g256, true, 1, 0},
                                  {P.n32, P.rows_reg.size() - P.n32, 0, P.g256, true, 1, 0}};
    for (int k = 0; k < 3; ++k) {
        JaroRegLaunch &L = P.reg[k] = reg[k];
        if (L.n_rows == 0 || L.g_begin >= L.g_end) {
            L.parts = 0;
            continue;
        }
        const int64_t want = (4 * P.max_grid + (int64_t)L.n_rows - 1) / (int64_t)L.n_rows, cap = std::max<int32_t>(1, (L.g_end - L.g_begin) / 4);
        L.parts = (int32_t)std::max<int64_t>(1, std::min(want, cap));
    }
    P.reg[1].slot0 = P.reg[0].parts;
    // the other from-strings have the general kernel alone: their to-groups are split by the same rule
    P.parts_long = 1;
    if (!P.rows_long.empty()) {
        const int64_t n = (int64_t)P.rows_long.size(), want = (4 * P.max_grid + n - 1) / n, cap = std::max<int32_t>(1, P.n_groups / 4);
        P.parts_long = (int32_t)std::max<int64_t>(1, std::min(want, cap));
    }
    P.n_slots = std::max(std::max(P.reg[0].parts + P.reg[1].parts, P.reg[2].parts) + 1, P.parts_long);
    return P;
}

}  // namespace pfz
