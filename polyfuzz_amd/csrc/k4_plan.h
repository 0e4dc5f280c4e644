// K4's to-side plan -- the to-list's alphabet, its strings sorted by length into groups of 64, their symbols packed per
// group -- as the kernels that walk it see it: K4 (k4_indel.hip, which builds it), K8 (k8_jaro.hip), K9 (k9_levenshtein.hip), K11
// (k11_join.hip) and K12 (k12_components.hip) through edit_walk.h's EditView; K10 (k10_pairs.hip) reads its symbol table alone.
#pragma once

#include "pfz_internal.h"

struct pfz_indel_plan {
    pfz_ctx *ctx = nullptr;
    int32_t n_sym = 0, idb = 8;          // alphabet size, bits per packed symbol
    uint32_t lut_len = 0;
    uint16_t *lut = nullptr;             // device [lut_len]
    uint32_t *packed = nullptr;          // device
    int64_t *g_off = nullptr;
    int32_t *g_steps = nullptr, *b_len = nullptr, *b_orig = nullptr;
    int64_t n_groups = 0;
    int64_t char_steps = 0;              // sum over to-strings of their (padded) steps * 64 / per: the bench's work count
    ~pfz_indel_plan()
    {
        for (void *p : {(void *)lut, (void *)packed, (void *)g_off, (void *)g_steps, (void *)b_len, (void *)b_orig})
            if (p) pfz::pool_free(p);
    }
};

namespace pfz {

// the plan of to-list T, built on first use and cached on the handle
int indel_plan_get(pfz_ctx *ctx, const pfz_strings *T, const pfz_indel_plan **out);

// the grid of a general kernel, halved until its match tables (pm_per bytes per workgroup) stay within 2 GiB; false: a single
// table is beyond 8 GiB
inline bool general_grid_cap(int64_t *grid, size_t pm_per)
{
    while (*grid > 1 && pm_per * (size_t)*grid > ((size_t)2 << 30)) *grid /= 2;
    return pm_per * (size_t)*grid <= ((size_t)8 << 30);
}

}  // namespace pfz
