// K18 / K19 -- the ONE walk over K7's to-side plan that bounds every pair of a from-row against a floor, scores the survivors and
// hands them to a sink: k7_join_kernel and the launches of a call.  Two translation units include it: k18_fuzz_join.hip (the
// threshold join and its components: the sinks FuzzAppend / FuzzUnite of k18_sink.h, the floor a constant) and k19_fuzz_topn.hip
// (the n best choices of every row: the sink FuzzTopn of k19_sink.h, the floor rising with the wave's list).  What differs is
// the sink and sits behind `if constexpr` on FuzzSinkTrait<SINK>::topn; the instances of the two older sinks compile to what they
// were.  The arithmetic of one pair -- the exact score fz_score, its float32 upper bound fz_upper_bound -- is K7's (k7_core.h),
// unchanged; the hit rule and the prune rule are k18_core.h.
//
// A fixed threshold is the easy case for K7's machinery: the floor `cur` a pair is bounded and scored against never moves, so
// there are no seeds, no bound cache, no shared running best, no continuation units -- and no wave ever waits for another
// workgroup.  The top-n form keeps all of that: its floor moves, but only inside the wave that owns the unit.
//
// Mapping to CDNA4 -- K7's (k7_fuzz.hip), on K7's to-side plan (to-strings sorted by length in groups of 64, every summary
// stored [group][lane]): persistent one-wave workgroups draw units (from-row, part) from ONE atomic counter and leave when the
// number they draw is past the end.  The wave sets the from-string up as K7 does -- match table [symbol][form][W] in LDS, class
// histogram, token masks, signature, presence words -- and its lanes walk the unit's to-groups ONCE:
//    bound   every lane computes the upper bound of its pair from registers; the pair goes on iff
//            !(bound + slack < (float)cutoff)  (k18_core.h fuzz_join_go);
//    queue   the survivors are ballot-compacted into a ring of 128 entries in LDS and scored 64 at a time, one pair per lane;
//            a coarse entry (its to-string has more than four tokens and the signatures meet) is bounded again with the exact
//            token intersection when it is popped, as in K7;
//    score   fz_score<W, false>(F, T, mode, cutoff): the full score in the lane, window sweeps included (every lane has a scratch
//            column of its own in LDS);
//    sink    score >= cutoff is a hit: appended behind one atomic per batch (join), or its two positions united in K12's forest
//            (components).
// Heavy rows are spread by `parts` alone (K7's rule, PFZ_K7_PARTS honoured): part p of a row walks the groups p, p + parts, ...
// Self-join: row i scores the choices j > i -- K7's "up to" skip -2 - i, generated here.  The to-groups are sorted by length, not
// by position, so a row still bounds every group (a lane whose choice is left out is not a candidate); the units keep K7's
// order, longest from-strings first.
//
// The top-n sink (K19).  The wave keeps the unit's TopnList (topn_wave.h: entry p in lane p, three registers per lane), empty when
// the unit (row, part) starts and stored to the unit's slot [row][part][ntop] of the call's list buffer when it ends.  A scored
// pair is offered to topn_insert iff score >= cutoff (the caller's score_cutoff, equal kept).  The floor of the bound and of
// fz_score is read again at the start of every bounding trip and of every batch: the score of the list's entry ntop - 1 once the
// list is full, the cutoff before -- wave-uniform, never falling.  Exact, by the two facts K18 rests on: fz_score is exact
// whenever it reaches its floor and never above the true score below it, and fuzz_join_go prunes only where the bound is
// STRICTLY below the floor -- a tie with the n-th best is still scored, and topn_insert's (score, index) compare places it; a
// score computed against an older, lower floor that no longer makes the list is dropped by that same compare.  A part's n-th
// best is never above its row's, so parts with floors of their own lose nothing.  The choices left out are K7's per-row skip
// codes (A.skip_idx / A.skip_up_to) as K7's one unsigned range test, not J.self.
//
// The set-up of a row, the record of a to-string, both bounds of a pair, to_of and the counters are K7's own: both kernels read
// them from k7_row.h, so a change of the bound is one edit (and moves every instance: tests/test_kernel_budget_cpu.py).
//
// What the fast kernel leaves out takes the general join kernel (k7_general.hip), three regions in all, each pair in exactly one:
// fast rows x ordinary to-strings (here), general rows (beyond 256 characters / 32 distinct tokens / a 60 KiB table, or all under
// PFZ_K7_FORCE_GENERAL) x all to-strings, fast rows x the to-strings with more than 32 distinct tokens.
#pragma once
#include "k7_device.h"
#include "k7_row.h"
#include "k19_sink.h"

#include <algorithm>
#include <climits>
#include <cmath>

namespace pfz {

static_assert(kFuzzJoinSlack == kBoundSlack, "k18_core.h restates K7's slack");

int fuzz_general_join_launch(pfz_ctx *ctx, FuzzArgs A, const FuzzJoinArgs &J, const FuzzAppend &sink, const pfz_strings *F,
                             const pfz_strings *T, const std::vector<int32_t> &rows);      // k7_general.hip
int fuzz_general_join_launch(pfz_ctx *ctx, FuzzArgs A, const FuzzJoinArgs &J, const FuzzUnite &sink, const pfz_strings *F,
                             const pfz_strings *T, const std::vector<int32_t> &rows);
int fuzz_general_join_launch(pfz_ctx *ctx, FuzzArgs A, const FuzzJoinArgs &J, const FuzzTopn &sink, const pfz_strings *F,
                             const pfz_strings *T, const std::vector<int32_t> &rows);

// the scratch columns: [position][lane] 16-bit symbols, one column per lane (fz_partial stages a to-form of up to kFuzzStage
// symbols there before it sweeps the windows)
constexpr size_t kJoinStageBytes = (size_t)kFuzzStage * 64 * sizeof(uint16_t);

template <int W, typename SINK, int MODE = -1>
__global__ __launch_bounds__(kK7Threads, W == 1 ? PFZ_K7_OCC : (W == 2 ? 3 : 2)) void k7_join_kernel(FuzzArgs A, FuzzJoinArgs J, SINK sink)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    // dynamic part: the from-string's match table [symbol][form][word]; the scratch columns [position][lane]
    uint64_t *pm = (uint64_t *)smem_raw;
    unsigned char *s_stage = smem_raw + (size_t)A.n_sym1 * 3 * W * sizeof(uint64_t);
    __shared__ FuzzRow<W> s_row;                  // the from-string (k7_row.h)
    __shared__ int s_queue[128];
    __shared__ int s_unit;
    const int tid = threadIdx.x, lane = tid & 63;
    const int mode = MODE >= 0 ? MODE : A.mode, parts = A.parts;      // (MODE >= 0: the scorer a compile-time constant)
    const double cutoff = J.cutoff;
    constexpr bool kTopn = FuzzSinkTrait<SINK>::topn;
    double cur = cutoff;                            // the floor a pair is bounded and scored against: the cutoff, until a full list raises it (K19)
    const int n_units = A.n_rows * parts;

    for (int p = tid; p < A.n_sym1 * 3 * W; p += kK7Threads) pm[p] = 0ull;
    __syncthreads();

    unsigned int n_bounded = 0, n_scored = 0;      // (work counters of this wave, per lane)
    unsigned long long n_steps = 0;
    for (;;) {
        if (tid == 0) s_unit = atomicAdd(A.next_unit, 1);
        __syncthreads();
        const int u = s_unit;
        if (u >= n_units) break;                   // (no unit is ever waited for: past the end, the workgroup leaves)
        const int r = u / parts, part = u - r * parts;
        const int row = A.rows[r];
        // ---- the from-string's tables, class histogram, tokens (k7_row.h)
        fuzz_row_setup<W>(A, s_row, pm, row, tid);
        FuzzFrom<W> F;
        FuzzRowSide B;
        fuzz_row_read<W>(s_row, pm, F, B);
        // the choices left out, as K7's ONE unsigned range test: a self-join leaves out 0 .. row, two lists the empty range at -1
        B.skip_lo = J.self ? 0 : -1;
        B.skip_span = J.self ? (unsigned)row : 0u;
        // the unit's list, and the floor back at the cutoff (K19); the range from K7's per-row skip codes -- "equal": skip alone;
        // "up to": 0 .. skip; none (-1): the empty range at -1
        [[maybe_unused]] TopnList list = topn_empty();
        if constexpr (kTopn) {
            const int skip = A.skip_idx ? A.skip_idx[row] : -1;
            B.skip_lo = A.skip_up_to && skip >= 0 ? 0 : skip;
            B.skip_span = (unsigned)(skip - B.skip_lo);
            cur = cutoff;
        }
        // (wave-uniform: every lane reads entry ntop - 1 from its lane)
        auto raise_floor = [&]() {
            if constexpr (kTopn) {
                double s;
                cur = topn_full(list, sink.ntop, &s) ? fmax(cutoff, s) : cutoff;
            }
        };

        // one batch: up to 64 queued pairs, one per lane -- a coarse entry's refined bound, the score, the sink
        auto score_batch = [&](int entry, bool active) {
            double sc = 0.0;
            int orig = -1;
            bool hit = false;
            raise_floor();
            if (active) {
                const int slot = entry & 0x7fffffff;
                const int4 m = A.b_meta[slot];
                const int4 m2 = A.b_meta2[slot];
                orig = m2.w;
                FuzzTo T = fuzz_to_of(A, slot, m, (PFZ_LDS_U16 *)(s_stage + lane * sizeof(uint16_t)), 64);      // (the lane's column)
                if (entry >= 0 || fuzz_join_go(fuzz_second_bound<W>(A, B, F, T, slot, m, m2, mode), cur)) {
                    sc = fz_score<W, false>(F, T, mode, cur);
                    hit = fuzz_join_hit(sc, cutoff);
                    n_scored += 1;
                    n_steps += (unsigned long long)work_estimate(F.la, m, mode, W);
                }
            }
            // (K19: a score below the floor it was computed against may be short of the true one -- it is behind entry ntop - 1
            // either way, and topn_insert's compare drops it)
            if constexpr (kTopn) topn_insert(list, sink.ntop, hit, sc, orig);
            else sink(hit, row, orig, sc);
        };

        // ---- the walk.  Two loops inside one, as in K7's second sweep: a tight one that bounds groups and pushes the survivors until
        //      64 pairs wait in the queue (nothing but the bound, a ballot and a push: no barrier, no scoring code), and around it
        //      the ONE place where pairs are scored -- that code, by far the largest part of the kernel, is inlined exactly once.
        int q_head = 0, q_tail = 0;             // wave-uniform; entries [q_head, q_tail) of a ring of 128
        auto visit = [&](const FuzzMeta &x, int g) {
            bool valid, coarse;
            const float ub = fuzz_bound_of(B, x, mode, valid, coarse);
            n_bounded += valid ? 1u : 0u;
            const bool go = valid && fuzz_join_go(ub, cur);
            const unsigned long long bal = FZ_BALLOT(go);
            if (go) s_queue[(q_tail + lanes_below(bal)) & 127] = (g * 64 + lane) | (coarse ? (int)0x80000000 : 0);
            q_tail += __popcll(bal);            // (fewer than 64 waited: at most 127 do now)
        };
        int g = part;
        // two groups per trip, each record fetched a group ahead into registers of its own (K7's first sweep: a record handed
        // from trip to trip costs seventeen register moves per group; the last trips re-read a group: harmless)
        FuzzMeta xa = fuzz_load_meta(A, min(g, A.n_groups - 1), lane, mode);
        for (;;) {
            raise_floor();          // (a bounding trip: the list changes in the batches below only)
            while (g < A.n_groups && q_tail - q_head < 64) {
                const FuzzMeta xb = fuzz_load_meta(A, min(g + parts, A.n_groups - 1), lane, mode);
                visit(xa, g);
                g += parts;
                if (!(g < A.n_groups && q_tail - q_head < 64)) {
                    xa = xb;
                    break;
                }
                xa = fuzz_load_meta(A, min(g + parts, A.n_groups - 1), lane, mode);
                visit(xb, g);
                g += parts;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            const bool last = g >= A.n_groups;
            while (q_tail - q_head >= 64 || (last && q_tail > q_head)) {
                const bool active = lane < q_tail - q_head;
                score_batch(active ? s_queue[(q_head + lane) & 127] : -1, active);
                q_head += min(64, q_tail - q_head);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            }
            if (last) break;
        }
        if constexpr (kTopn) topn_store(list, sink.ntop, sink.slot(row, part));
        fuzz_row_clear<W>(A, s_row, pm, A.a_off[row], tid);      // (a_off[row] read again: held through the unit, as K7 holds it, the walk measured slower)
    }
    fuzz_add_counters(A.counters, n_bounded, n_scored, n_steps, lane);
}

template <int W, typename SINK>
static void join_launch_w(int32_t scorer, dim3 grid, size_t lds, hipStream_t st, const FuzzArgs &A, const FuzzJoinArgs &J, const SINK &sink)
{
    // WRatio -- what RapidFuzz() runs by default -- has instances of its own, as in K7: the scorer a compile-time constant
    if (scorer == kWRatio) hipLaunchKernelGGL((k7_join_kernel<W, SINK, kWRatio>), grid, dim3(kK7Threads), lds, st, A, J, sink);
    else hipLaunchKernelGGL((k7_join_kernel<W, SINK>), grid, dim3(kK7Threads), lds, st, A, J, sink);
}

// The kernels of a call over the prepared rows, on the context's stream: the three word classes of the fast kernel, then the
// general kernel's two regions.  d_next: int32[4], zeroed -- the unit counters of the three classes.
// The top-n sink's slots of a row (k19_sink.h): the parts of the fast kernel first, then the four waves of the general kernel's
// workgroup -- a row is a fast row or a general one, so the general rows' lists sit in the slots 0 .. 3, and the lists of the fast
// rows against the to-strings with more than 32 distinct tokens in the last four, behind the parts.
template <typename SINK>
static int fuzz_join_launch(pfz_ctx *ctx, FuzzPrep &prep, const pfz_strings *F, const pfz_strings *T, int32_t scorer, const FuzzJoinArgs &J,
                            const SINK &sink, int32_t *d_next)
{
    FuzzArgs &A = prep.A;
    const pfz_fuzz_plan *pl = prep.plan;
    DevBuf d_rows[3];
    for (int c = 0; c < 3; ++c) {
        if (prep.rows[c].empty()) continue;
        PFZ_TRY(d_rows[c].upload(ctx, prep.rows[c]));
        A.rows = d_rows[c].as<int32_t>();
        A.n_rows = (int32_t)prep.rows[c].size();
        A.parts = fuzz_parts(ctx, pl, A.n_rows);
        if constexpr (FuzzSinkTrait<SINK>::topn)
            PFZ_REQUIRE(A.parts <= sink.n_lists - kTopnGeneralLists, "pfz_fuzz_topn: %d parts, %d lists per row", A.parts, sink.n_lists);
        A.next_unit = d_next + c;
        const size_t lds = fuzz_table_bytes(A, c) + kJoinStageBytes;
        const dim3 grid((unsigned)std::min<int64_t>((int64_t)A.n_rows * A.parts, fuzz_max_grid(ctx)));
        if (c == 0) join_launch_w<1>(scorer, grid, lds, ctx->stream, A, J, sink);
        else if (c == 1) join_launch_w<2>(scorer, grid, lds, ctx->stream, A, J, sink);
        else join_launch_w<4>(scorer, grid, lds, ctx->stream, A, J, sink);
        PFZ_HIP(hipGetLastError());
    }
    A.parts = 1;
    A.big_slots = nullptr;
    A.n_big = 0;
    SINK general = sink;
    if constexpr (FuzzSinkTrait<SINK>::topn) general.general0 = 0;
    PFZ_TRY(fuzz_general_join_launch(ctx, A, J, general, F, T, prep.rows[3]));
    if (!pl->big_slots.empty()) {
        std::vector<int32_t> others;
        for (int c = 0; c < 3; ++c) others.insert(others.end(), prep.rows[c].begin(), prep.rows[c].end());
        A.big_slots = pl->d_big_slots;
        A.n_big = (int32_t)pl->big_slots.size();
        if constexpr (FuzzSinkTrait<SINK>::topn) general.general0 = sink.n_lists - kTopnGeneralLists;
        PFZ_TRY(fuzz_general_join_launch(ctx, A, J, general, F, T, others));
    }
    return PFZ_OK;
}

}  // namespace pfz
