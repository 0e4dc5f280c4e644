// K7 / K18 / K19: what the two register / LDS kernels over K7's plan do alike for one from-string, held ONCE -- k7_fuzz_kernel
// (k7_fuzz.hip, the arg-max) and k7_join_kernel (k7_join_walk.h, the threshold join and the top-n) both read it from here:
//    * the from-string's LDS state (FuzzRow<W>), its set-up and the table clean-up at the end of a unit;
//    * the from-side values the bound reads (FuzzRowSide), the record a lane reads of one to-string (FuzzMeta), and the
//      float32 upper bound of a pair from registers only (fuzz_bound_of);
//    * the second, exact-intersection bound of a coarse queue entry (fuzz_second_bound);
//    * the to-string's record for the scorer (fuzz_to_of) and the work-counter reduction (fuzz_add_counters).
// A change of the bound is one edit here and moves all 24 instances of the two kernels at once: tests/test_kernel_budget_cpu.py
// holds their registers, tools/kernel_budget.py prints them.  What a kernel does with a bound -- seeds, bound cache, floor,
// queue, sink -- and which choices a row leaves out (skip_lo / skip_span) stay in the kernel.
// Everything here is force-inlined into its one caller; "wave-uniform" marks the arguments that sit in scalar registers.
#pragma once
#include "k7_device.h"

namespace pfz {

// the from-string in LDS, one instance per workgroup (64-bit members first: no padding -- 512 W + 456 bytes, and K7's static LDS
// sits on a 256-byte occupancy step)
template <int W> struct FuzzRow {
    uint64_t tmask[kFuzzMaxTokens * W], smask[kFuzzMaxTokens * W];      // FuzzFrom: the positions of token i in form 2, of the space after it
    int tid[kFuzzMaxTokens], tlen[kFuzzMaxTokens];                      // distinct tokens: id in the to-side's table, length
    int cnt[4 * kFuzzHistWords];                                        // characters per class, counted ...
    uint32_t hist[kFuzzHistWords], sig[2], pres[2];                     // ... and packed; token signature; symbol-presence words
    int la[3], ta, nspace, usum;                                        // form lengths, distinct tokens, spaces, sum of cnt (-1: a count > 255)
};
static_assert(sizeof(FuzzRow<1>) == 968 && sizeof(FuzzRow<2>) == 1480 && sizeof(FuzzRow<4>) == 2504, "FuzzRow has padding");

__device__ inline bool mode_bounds_presence(int mode) { return mode != kTokenSetRatio && mode != kTokenRatio; }      // (see fuzz_bound_of)

// The from-string's tables, class histogram, presence words, tokens, signature.  All threads of the workgroup call it; row is
// wave-uniform; pm: the match table [symbol][form][W], all zero.  The first barrier also covers what the caller stored just
// before the call; the last one leaves R readable by every thread.
template <int W> __device__ __forceinline__ void fuzz_row_setup(const FuzzArgs &A, FuzzRow<W> &R, uint64_t *pm, int row, int tid)
{
    const int64_t a0 = A.a_off[row];
    if (tid < 4 * kFuzzHistWords) R.cnt[tid] = 0;
    if (tid < 2) R.pres[tid] = 0u;
    if (tid == 0) R.nspace = 0;
    __syncthreads();
    for (int v = 0; v < 3; ++v) {
        const int m = v == 0 ? (int)(A.a_off[row + 1] - a0) : (v == 1 ? A.a_len1[row] : A.a_len2[row]);
        if (tid == 0) R.la[v] = m;
        for (int p = tid; p < m; p += kK7Threads) {
            const uint32_t c = load_unit(A.a_form[v], A.a_width, a0 + p);
            const int sy = c < A.lut_len ? (int)A.lut[c] : 0;
            if (sy) {
                atomicOr((unsigned long long *)&pm[(sy * 3 + v) * W + (p >> 6)], 1ull << (p & 63));
                if (v == 0) {
                    atomicAdd(&R.cnt[A.cls[sy]], 1);
                    if (sy == A.space_rank) atomicAdd(&R.nspace, 1);
                    if (!is_space_cp(c)) atomicOr(&R.pres[(sy & 63) >> 5], 1u << (sy & 31));      // (no whitespace symbol: see k7_pack)
                }
            }
        }
    }
    if (tid == 0) {
        const int64_t tb = tok_base(a0, row);
        const int ta = A.a_ntok[row];
        R.ta = ta;
        int start = 0;
        uint64_t sig = 0ull;
        for (int i = 0; i < ta; ++i) {
            const int len = A.a_tok_len[tb + i];
            R.tid[i] = A.a_tok_id[tb + i];
            R.tlen[i] = len;
            sig |= fz_sig_bit(R.tid[i]);
            uint64_t tm[W], sm[W];
            fz_range_mask<W>(tm, start, start + len);
            fz_range_mask<W>(sm, start + len, i + 1 < ta ? start + len + 1 : start + len);
#pragma unroll
            for (int w = 0; w < W; ++w) {
                R.tmask[i * W + w] = tm[w];
                R.smask[i * W + w] = sm[w];
            }
            start += len + 1;
        }
        R.sig[0] = (uint32_t)sig;
        R.sig[1] = (uint32_t)(sig >> 32);
    }
    __syncthreads();
    if (tid == 0) {
        const int nt_all = A.a_ntok_all[row];
        const int extra = (nt_all - 1) - R.nspace;
        if (extra > 0) R.cnt[A.space_class] += extra;
        int usum = 0, big = 0;
        for (int c = 0; c < 4 * kFuzzHistWords; ++c) {
            usum += R.cnt[c];
            big |= R.cnt[c] > 255;
        }
        for (int d = 0; d < kFuzzHistWords; ++d)
            R.hist[d] = (uint32_t)R.cnt[4 * d] | (uint32_t)R.cnt[4 * d + 1] << 8 | (uint32_t)R.cnt[4 * d + 2] << 16 | (uint32_t)R.cnt[4 * d + 3] << 24;
        R.usum = big ? -1 : usum;
    }
    __syncthreads();
}

// clear this from-string's table entries at the end of a unit (all threads; a0 = a_off[row], wave-uniform)
template <int W> __device__ __forceinline__ void fuzz_row_clear(const FuzzArgs &A, const FuzzRow<W> &R, uint64_t *pm, int64_t a0, int tid)
{
    for (int v = 0; v < 3; ++v) {
        const int m = R.la[v];
        for (int p = tid; p < m; p += kK7Threads) {
            const uint32_t c = load_unit(A.a_form[v], A.a_width, a0 + p);
            const int sy = c < A.lut_len ? (int)A.lut[c] : 0;
#pragma unroll
            for (int w = 0; w < W; ++w) pm[(sy * 3 + v) * W + w] = 0ull;
        }
    }
    __syncthreads();
}

// The from-side values the bound reads, all wave-uniform.  The kernel adds the choices its row leaves out --
// choice_left_out(w, skip, up_to) for w >= 0 as ONE unsigned range test (the first sweep runs it for every pair): the choices
// skip_lo .. skip_lo + skip_span are left out; none: the empty range at -1.
struct FuzzRowSide {
    FuzzSummary sa;
    uint32_t pres_a0, pres_a1;
    int n_pres_a;
    int skip_lo;
    unsigned skip_span;
    int la2, ta;                     // length of form 2, distinct tokens
    const int *tid, *tlen;           // the tokens' ids and lengths, in LDS
};

// after the set-up: the from-string as the scorer (F) and the bound (B, but for skip_lo / skip_span) read it
template <int W> __device__ __forceinline__ void fuzz_row_read(const FuzzRow<W> &R, const uint64_t *pm, FuzzFrom<W> &F, FuzzRowSide &B)
{
    F = {pm, {R.la[0], R.la[1], R.la[2]}, R.ta, R.tid, R.tlen, R.tmask, R.smask};
#pragma unroll
    for (int v = 0; v < 3; ++v) B.sa.len[v] = F.la[v];
    B.sa.ntok = F.ta;
#pragma unroll
    for (int d = 0; d < kFuzzHistWords; ++d) B.sa.hist[d] = R.hist[d];
    B.sa.usum = R.usum;
    B.sa.sig = (uint64_t)R.sig[0] | (uint64_t)R.sig[1] << 32;
    B.pres_a0 = R.pres[0];
    B.pres_a1 = R.pres[1];
    B.n_pres_a = __popc(B.pres_a0) + __popc(B.pres_a1);
    B.la2 = F.la[2];
    B.ta = F.ta;
    B.tid = R.tid;
    B.tlen = R.tlen;
}

// the to-string in slot `slot` for the scorer; m = b_meta[slot].  stage / stride: the lane's scratch column for fz_partial's window
// sweeps (nullptr, 0: the scorer sweeps none itself)
__device__ __forceinline__ FuzzTo fuzz_to_of(const FuzzArgs &A, int slot, const int4 &m, PFZ_LDS_U16 *stage, int stride)
{
    const int4 rec = A.b_meta3[slot];
    return {{A.b_sym + rec.x, A.b_sym + rec.x + rec.w, A.b_sym + rec.x + 2 * rec.w},      // sym
            A.b_tag + rec.y, A.b_tok_id + rec.z, A.b_tok_len + rec.z,                     // tag, tok_id, tok_len
            {m.x, m.y, m.z}, m.w, stage, stride, -1, 0};                                  // lb, tb, the column, staged: none, n_windows
}

// what a sweep reads of one to-string: five 128-bit loads, all issued one group ahead of their use
struct FuzzMeta {
    int4 m, m2, m4;
    uint4 h0, h1;
    uint2 p;
};
// (byte offsets in 32 bits: a scalar base + one vector offset per load instead of 64-bit address arithmetic per lane
// and array -- the to-side holds at most 2^26 strings, 2^30 B of its widest array)
// g, mode: wave-uniform
__device__ __forceinline__ FuzzMeta fuzz_load_meta(const FuzzArgs &A, int g, int lane, int mode)
{
    const uint32_t off = ((uint32_t)g * 64u + (uint32_t)lane) * 16u;
    FuzzMeta x;
    x.m = *(const int4 *)((const char *)A.b_meta + off);
    x.m2 = *(const int4 *)((const char *)A.b_meta2 + off);
    x.m4 = *(const int4 *)((const char *)A.b_meta4 + off);
    const uint32_t hoff = ((uint32_t)g * 128u + (uint32_t)lane) * 16u;
    x.h0 = *(const uint4 *)((const char *)A.b_hist + hoff);
    x.h1 = *(const uint4 *)((const char *)A.b_hist + hoff + 1024u);
    x.p = mode_bounds_presence(mode) ? *(const uint2 *)((const char *)A.b_pres + (off >> 1)) : make_uint2(0u, 0u);
    return x;
}

// the to-side of the bound from a to-string's records: b_meta, b_meta2 and its two of b_hist
__device__ __forceinline__ FuzzSummary fuzz_summary_of(const int4 &m, const int4 &m2, const uint4 &h0, const uint4 &h1)
{
    return {{m.x, m.y, m.z}, m.w, {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w},       // len, ntok, hist
            m2.z, (uint64_t)(uint32_t)m2.x | (uint64_t)(uint32_t)m2.y << 32};             // usum, sig
}

// float32 upper bound of the pair (from-string, to-string x) FROM REGISTERS ONLY; valid = a real candidate of this
// kernel.  When the token signatures meet, the exact intersection is taken from the first four token ids (nearly
// every to-string has no more); `coarse` = the signatures meet but the string has more tokens: the bound assumes
// the best, and the pair is looked at again -- with its record -- when it is popped from the queue.
// B, mode: wave-uniform
__device__ __forceinline__ float fuzz_bound_of(const FuzzRowSide &B, const FuzzMeta &x, int mode, bool &valid, bool &coarse)
{
    const FuzzSummary &sa = B.sa;
    const bool use_tokens = mode_uses_tokens(mode), use_pres = mode_bounds_presence(mode);
    const int4 m = x.m;
    valid = x.m2.w >= 0 && (unsigned)(x.m2.w - B.skip_lo) > B.skip_span && m.w <= kFuzzMaxTokens;
    const FuzzSummary sb = fuzz_summary_of(x.m, x.m2, x.h0, x.h1);
    const int uu = fz_common_chars(sa, sb);
    const bool maybe = use_tokens && (sa.sig & sb.sig) != 0ull;
    coarse = maybe && m.w > 4;
    // the common tokens: every lane compares its (up to four) to-token ids with the from-string's, which sit in
    // scalar registers -- one pass, no branch (disjoint signatures simply find nothing)
    // (the four compares leave lane masks in scalar registers, or-ed there; one select and one add per from-token carry
    // both sums -- common tokens << 16 | their characters, a form is shorter than 2^16: 8 vector instructions per token
    // where the compiler's own rendering of `hit ? .. : ..` took 18, and the kernel is bound by its vector issue rate)
    int nc = 0, sect_chars = 0;
    if (use_tokens) {
        int acc = 0;
        for (int i = 0; i < B.ta; ++i) {
            const int ida = __builtin_amdgcn_readfirstlane(B.tid[i]);          // (absent to-tokens are -1, unknown from-tokens <= -2)
            acc += select_if_any_eq(x.m4, ida, B.tlen[i] | 0x10000);
        }
        nc = acc >> 16;
        sect_chars = acc & 0xffff;
    }
    // symbols of the one string that the other lacks (fz_presence_miss, the from-side's bits in scalar registers)
    // (only where it pays: the scorers that sweep windows, WRatio included -- 20k x 20k titles, WRatio 8.38 -> 8.04 ms
    // with 3.8 % of the pairs scored instead of 6.0 %; token_ratio, which sweeps none, 5.33 -> 5.86 ms for 2.5 %
    // instead of 2.9 %: there the bits stay out, a wave-uniform choice)
    int miss_a = 0, miss_b = 0;
    if (use_pres) {
        const int pres_common = __popc(B.pres_a0 & x.p.x) + __popc(B.pres_a1 & x.p.y);
        miss_a = B.n_pres_a - pres_common;
        miss_b = __popc(x.p.x) + __popc(x.p.y) - pres_common;
    }
    // (WRatio reads the token-set bound in one of its two families only -- fz_upper_bound; groups are sorted by length,
    // so whole waves skip it)
    const bool wants_tset = mode == kTokenSetRatio || mode == kTokenRatio ||
                            (mode == kWRatio && 2 * max(sa.len[0], m.x) < 3 * min(sa.len[0], m.x));
    const float tset = nc != 0 && wants_tset ? fz_token_set_bound_n(B.la2, B.ta, m.z, m.w, uu, nc, sect_chars, miss_a, miss_b) : -1.0f;
    return fz_upper_bound(sa, sb, mode, uu, coarse ? -1 : (nc != 0 ? 1 : 0), coarse ? -1.0f : tset, miss_a, miss_b);
}

// The second look at a coarse entry, when it is popped from the queue: the bound again, with the exact token intersection
// from the to-string's record T.  m, m2: b_meta[slot], b_meta2[slot].  The kernel compares it with its own floor.
template <int W>
__device__ __forceinline__ float fuzz_second_bound(const FuzzArgs &A, const FuzzRowSide &B, const FuzzFrom<W> &F, const FuzzTo &T, int slot,
                                                   const int4 &m, const int4 &m2, int mode)
{
    const FuzzSummary sb = fuzz_summary_of(m, m2, A.b_hist[((slot >> 6) * 2 + 0) * 64 + (slot & 63)], A.b_hist[((slot >> 6) * 2 + 1) * 64 + (slot & 63)]);
    const int uu = fz_common_chars(B.sa, sb);
    uint32_t ca, cb;
    fz_intersect<W>(F, T, ca, cb);
    return fz_upper_bound(B.sa, sb, mode, uu, ca ? 1 : 0, ca ? fz_token_set_bound<W>(F, ca, m.z, m.w, uu) : -1.0f);
}

// the lanes' work counters -- pairs bounded, pairs scored, word-steps -- summed over the wave into counters[0..2] (wave-uniform;
// null: not asked for)
__device__ __forceinline__ void fuzz_add_counters(unsigned long long *counters, unsigned long long nb, unsigned long long nsc,
                                                  unsigned long long nst, int lane)
{
    if (!counters) return;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        nb += __shfl_xor(nb, d, 64);
        nsc += __shfl_xor(nsc, d, 64);
        nst += __shfl_xor(nst, d, 64);
    }
    if (lane == 0) {
        atomicAdd(&counters[0], nb);
        atomicAdd(&counters[1], nsc);
        atomicAdd(&counters[2], nst);
    }
}

}  // namespace pfz
