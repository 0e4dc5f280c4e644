// K25 -- character-n-gram SimHash fingerprints of a resident string list, written straight into a 1-bit operand handle
// (pfz_simhash, what SimHash.join / .components / .match run in front of K23 / K24 / K5's Hamming program).  The rule is
// k25_core.h's: TFIDF's analyzer (clean, windows of lo .. hi symbols, windows with a ' ' dropped), a 64-bit mixing hash per window
// widened to W words, a +-1 vote per bit and window, bit = vote > 0.
//
// Mapping to CDNA4: one wave per string, four waves per workgroup, no workgroup barrier.  The string is taken 64 code units at a
// time, 63 where it is cleaned (k25_core.h says why), as k_extract_wave of k1_vectorize.hip takes it: every lane classifies its
// unit, two ballots place the kept characters and the collapsed spaces (the step functions of k25_core.h, which the host program of
// the tests runs too), and the step's symbols go to a line of 8 + 64 words in LDS.  The line's first 8 words hold the symbols in
// front of the step -- the last hi - 1 are all a window can reach back to -- and are rewritten after every step, the wave carries
// `pend` / `any` in registers: no length limit, no second kernel.  Every lane then hashes the windows that END at its symbol.
// Votes: lane b owns bit b of every word, it holds one int32 count of set bits per word.  For every window of the step (a loop over
// the ballot of the lanes that have one, so a short string pays for its windows only) the hash word is read from the window's lane
// (v_readlane) and the lane adds its bit: shift, and, add.  The other exact way -- lane = window, 64 ballots + popcounts per step and
// word whatever the number of windows -- costs a full step for a name of twenty characters; docs/SIMHASH_MEASURED.md.  At the end
// one ballot per word of (2 ones > windows) IS the fingerprint word; lanes 0 .. 7 write its bit-reversed bytes (k5_pack_signs).
// WB words are voted per walk over the string: 1 for 64 bits, 2 for 128, else 4 -- 192 bits pay for 256 --, and wider fingerprints
// walk it again for the next four words:
// the counts stay in registers whatever W is.  No atomics, no scratch.
//
// Behind it: exclusive_scan_i32 over "has a window" gives every surviving string its row, and k25_compact writes the rows into a
// fresh PFZ_DENSE_B1 handle in pfz_dense_upload1's layout (pitch of whole 16-byte pieces, padding zero, factor 1).
#include "k5_core.h"
#include "k25_core.h"

namespace pfz {

struct K25Args {
    const void *chars;
    const int64_t *off;
    int64_t n;
    int32_t lo, hi, clean, remove_space, words;
    uint64_t *fp;              // [n][words]: every string's fingerprint, as the bytes of the packed layout
    int32_t *windows;          // [n]
    int32_t *flag;             // [n + 1]: 1 = the string has a window (the scan's input)
};

// bit `lane` of lane src's 64-bit value: both halves come over as scalars, the lane picks its half and its bit
__device__ __forceinline__ int32_t k25_bit_of_lane(uint64_t v, int src, int lane)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src);
    return (int32_t)(((lane < 32 ? lo : hi) >> (lane & 31)) & 1u);
}

__device__ __forceinline__ void k25_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

template <int CW, int WB>
__global__ __launch_bounds__(256) void k25_fingerprint(K25Args P)
{
    __shared__ uint32_t s_line[4][kK25Line];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * 4 + wave;
    if (i >= P.n) return;                                   // (the whole wave: nothing below waits for another wave)
    uint32_t *line = s_line[wave];
    const int64_t b = P.off[i], len = P.off[i + 1] - b;
    const int lo = P.lo, hi = P.hi;
    const bool remove_space = P.remove_space != 0;
    int32_t n_win = 0;

    for (int q0 = 0; q0 < P.words; q0 += WB) {
        int32_t ones[WB];
#pragma unroll
        for (int w = 0; w < WB; ++w) ones[w] = 0;
        n_win = 0;
        if (lane < kK25Carry) line[lane] = kK25None;        // nothing in front of the string
        K25Flags flags;
        k25_wave_sync();
        // (a cleaning step takes 63 units: with the space pending from the steps before, 64 could leave 65 symbols -- k25_core.h)
        const int step = CW == 1 && P.clean ? kK25CleanStep : kK25RawStep;
        for (int64_t c0 = 0; c0 < len; c0 += step) {
            // ---- the step's symbols -----------------------------------------------------------------------------------------
            const int64_t p = c0 + lane;
            const bool mine = lane < step && p < len;
            uint32_t c = kK25None;
            if (mine) c = CW == 1 ? (uint32_t)((const uint8_t *)P.chars)[b + p] : ((const uint32_t *)P.chars)[b + p];
            int n_step;
            if (CW == 1 && P.clean) {
                const uint32_t s = mine ? k25_clean_class(c) : kK25None;
                const bool keep = s != kK25None && s != kK25Space;
                const uint64_t keepm = __ballot(keep), spm = __ballot(s == kK25Space);
                const bool sp_before = keep && k25_space_before(keepm, spm, flags, lane);
                const uint64_t esm = __ballot(sp_before);
                const int pos = k25_place(keepm, esm, lane);
                if (sp_before) line[kK25Carry + pos - 1] = kK25Space;
                if (keep) line[kK25Carry + pos] = s;
                n_step = k25_step_symbols(keepm, esm);                 // <= 64
                flags = k25_step_flags(keepm, spm, flags);
            } else {
                if (mine) line[kK25Carry + lane] = c;
                n_step = (int)(len - c0 < step ? len - c0 : step);
            }
            k25_wave_sync();
            // ---- the windows that end at symbol `lane` of the step -------------------------------------------------------------
            const uint32_t *at = line + kK25Carry + lane;
            const int run = lane < n_step ? k25_run_back(at, hi, remove_space) : 0;
            for (int nn = lo; nn <= hi; ++nn) {
                const bool valid = run >= nn;
                const uint64_t vm = __ballot(valid);
                if (vm == 0ull) break;                      // (no longer window either)
                const uint64_t g = valid ? k25_hash_back(at, nn) : 0ull;
                uint64_t h[WB];
#pragma unroll
                for (int w = 0; w < WB; ++w) h[w] = k25_word(g, q0 + w);
                n_win += __popcll(vm);
#if defined(K25_VOTE_BY_WINDOW)
                // the other exact count, lane = window (a variant build for the measurement, tools/build_variant.sh): 64 ballots a word
                for (int bit = 0; bit < 64; ++bit) {
#pragma unroll
                    for (int w = 0; w < WB; ++w) {
                        const uint64_t set = __ballot(valid && ((h[w] >> bit) & 1ull) != 0ull);
                        if (lane == bit) ones[w] += __popcll(set);
                    }
                }
#else
                for (uint64_t m = vm; m; m &= m - 1ull) {
                    const int src = __builtin_ctzll(m);
#pragma unroll
                    for (int w = 0; w < WB; ++w) ones[w] += k25_bit_of_lane(h[w], src, lane);
                }
#endif
            }
            // ---- the symbols the next step can reach back to ---------------------------------------------------------------------
            uint32_t keep_sym = kK25None;
            if (lane < kK25Carry - 1) keep_sym = line[k25_carry_from(n_step, lane)];      // the last 7 of (carry, step): all written
            k25_wave_sync();
            if (lane < kK25Carry - 1) line[1 + lane] = keep_sym;
            k25_wave_sync();
        }
#pragma unroll
        for (int w = 0; w < WB; ++w) {
            const uint64_t mask = __ballot(k25_vote_bit(ones[w], n_win));
            if (q0 + w < P.words && lane < 8) ((uint8_t *)(P.fp + i * P.words + q0 + w))[lane] = k25_packed_byte(mask, lane);
        }
    }
    if (lane == 0) {
        P.windows[i] = n_win;
        P.flag[i] = n_win > 0 ? 1 : 0;
    }
}

// thread (string, 8-byte word of the row's pitch): the rows of the strings with a window, in order, into the operand handle
__global__ __launch_bounds__(256) void k25_compact(const uint64_t *__restrict__ fp, const int32_t *__restrict__ windows,
                                                    const int32_t *__restrict__ row_of, int64_t n, int32_t words, int32_t pitch_words,
                                                    uint64_t *__restrict__ x, float *__restrict__ inv, int32_t *__restrict__ out_row)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = t / pitch_words;
    const int k = (int)(t - i * pitch_words);
    if (i >= n) return;
    const bool has = windows[i] > 0;
    const int32_t r = row_of[i];
    if (has) x[(int64_t)r * pitch_words + k] = k < words ? fp[i * words + k] : 0ull;
    if (k == 0) {
        out_row[i] = has ? r : -1;
        if (has) inv[r] = 1.f;
    }
}

template <int CW>
static void k25_launch(pfz_ctx *ctx, const K25Args &P)
{
    const dim3 grid((unsigned)((P.n + 3) / 4));
    if (P.words == 1) hipLaunchKernelGGL((k25_fingerprint<CW, 1>), grid, dim3(256), 0, ctx->stream, P);
    else if (P.words == 2) hipLaunchKernelGGL((k25_fingerprint<CW, 2>), grid, dim3(256), 0, ctx->stream, P);
    else hipLaunchKernelGGL((k25_fingerprint<CW, 4>), grid, dim3(256), 0, ctx->stream, P);
}

}  // namespace pfz

using namespace pfz;

extern "C" {

int pfz_simhash(pfz_ctx *ctx, const pfz_strings *strings, const pfz_tfidf_params *params, int32_t bits, pfz_dense **out_codes,
                int32_t *out_row, int32_t *out_windows, uint8_t *out_bytes)
{
    PFZ_REQUIRE(ctx && strings && params && out_codes, "pfz_simhash: NULL argument");
    PFZ_REQUIRE(strings->n == 0 || out_row, "pfz_simhash: NULL out_row");
    PFZ_REQUIRE(k25_bits_ok(bits), "pfz_simhash: %d bits; a fingerprint has a multiple of 64 bits in [%d, %d]", bits, kK25MinBits, kK25MaxBits);
    PFZ_REQUIRE(k25_grams_ok(params->ngram_lo, params->ngram_hi), "pfz_simhash: n_gram_range (%d, %d) does not satisfy 1 <= lo <= hi <= %d",
                params->ngram_lo, params->ngram_hi, kK25MaxGram);
    PFZ_REQUIRE(strings->char_width == 1 || strings->char_width == 4, "pfz_simhash: code units of %d bytes", strings->char_width);
    PFZ_REQUIRE(!(params->clean && strings->char_width != 1),
                "pfz_simhash: clean = 1 on 4-byte code units; strings with code points > 0xFF are cleaned on the host (pass clean = 0)");
    const int64_t n = strings->n;
    if (n >= ((int64_t)1 << 31)) {
        set_error("pfz_simhash: %lld strings exceed the 32-bit rows", (long long)n);
        return PFZ_ERR_UNSUPPORTED;
    }
    PFZ_HIP(hipSetDevice(ctx->device));
    const int32_t words = bits / 64;
    Owner<pfz_dense, pfz_dense_free> m(new pfz_dense());
    m->ctx = ctx;
    m->dim = bits;
    m->ld = ((int64_t)bits + 127) / 128 * 128;
    m->normalize = 1;
    m->dtype = PFZ_DENSE_B1;
    const int32_t pitch_words = (int32_t)(m->ld / 64);
    int32_t total = 0;
    DevBuf fp, windows, row_of, d_row;
    if (n > 0) {
        PFZ_TRY(fp.alloc(ctx, (size_t)n * words * sizeof(uint64_t)));
        PFZ_TRY(windows.alloc(ctx, (size_t)n * sizeof(int32_t)));
        PFZ_TRY(row_of.alloc(ctx, (size_t)(n + 1) * sizeof(int32_t)));
        PFZ_TRY(d_row.alloc(ctx, (size_t)n * sizeof(int32_t)));
        K25Args P;
        P.chars = strings->chars;
        P.off = strings->offsets;
        P.n = n;
        P.lo = params->ngram_lo;
        P.hi = params->ngram_hi;
        P.clean = params->clean ? 1 : 0;
        P.remove_space = params->remove_space_ngrams ? 1 : 0;
        P.words = words;
        P.fp = fp.as<uint64_t>();
        P.windows = windows.as<int32_t>();
        P.flag = row_of.as<int32_t>();
        {
            ProfScope ps(ctx, "k25_fingerprint");
            if (strings->char_width == 1) k25_launch<1>(ctx, P);
            else k25_launch<4>(ctx, P);
            PFZ_HIP(hipGetLastError());
        }
        PFZ_TRY(exclusive_scan_i32(ctx, row_of.as<int32_t>(), n));
        PFZ_TRY(copy_d2h(ctx, &total, row_of.as<int32_t>() + n, sizeof(total)));      // (waits: the handle's size)
    }
    m->n = total;
    PFZ_TRY(pool_alloc(ctx, &m->x, (size_t)(total > 0 ? total : 1) * (size_t)pitch_words * sizeof(uint64_t)));
    PFZ_TRY(pool_alloc(ctx, &m->inv, (size_t)(total > 0 ? total : 1) * sizeof(float)));
    if (n > 0) {
        {
            ProfScope ps(ctx, "k25_compact");
            const int64_t threads = n * pitch_words;
            hipLaunchKernelGGL(k25_compact, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx->stream, fp.as<uint64_t>(),
                               windows.as<int32_t>(), row_of.as<int32_t>(), n, words, pitch_words, (uint64_t *)m->x, m->inv, d_row.as<int32_t>());
            PFZ_HIP(hipGetLastError());
        }
        PFZ_TRY(copy_d2h(ctx, out_row, d_row.p, (size_t)n * sizeof(int32_t)));
        if (out_windows) PFZ_TRY(copy_d2h(ctx, out_windows, windows.p, (size_t)n * sizeof(int32_t)));
        if (out_bytes) PFZ_TRY(copy_d2h(ctx, out_bytes, fp.p, (size_t)n * words * sizeof(uint64_t)));
    }
    *out_codes = m.release();
    return PFZ_OK;
}

}  // extern "C"
