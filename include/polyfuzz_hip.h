/*
 * polyfuzz_hip.h -- C ABI of libpolyfuzz_hip.so, the MI355X (gfx950) engine
 * behind PolyFuzz's TFIDF / EditDistance matchers.
 *
 * The reference (MaartenGr/PolyFuzz v0.4.3) is pure Python and has no FFI of
 * its own; the entry points below are what a binding for its hot path would
 * bind.  Each one cites the reference interface it replaces (file:line under
 * the reference tree).  Conventions:
 *   - plain pointers and sizes only; no torch / numpy types;
 *   - every function returns 0 on success or a negative pfz_status; the
 *     message of the last failure on the calling thread is pfz_last_error();
 *   - host ("_host" / upload / download) entry points take caller-owned host
 *     buffers; every other buffer is device memory owned by an opaque handle;
 *   - all device work of a context is issued on that context's own HIP stream;
 *     calls return after enqueueing unless documented otherwise
 *     (downloads and pfz_ctx_sync block);
 *   - "no match" is idx = -1, score = 0.
 * There is NO CPU fallback anywhere behind this ABI: without a gfx950 device
 * pfz_ctx_create fails with PFZ_ERR_NO_DEVICE.
 */
#ifndef POLYFUZZ_HIP_H
#define POLYFUZZ_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PFZ_VERSION 100 /* 0.1.0 */

typedef enum pfz_status {
    PFZ_OK = 0,
    PFZ_ERR_INVALID = -1,     /* bad argument */
    PFZ_ERR_NO_DEVICE = -2,   /* no usable HIP device */
    PFZ_ERR_HIP = -3,         /* a HIP runtime call failed (see pfz_last_error) */
    PFZ_ERR_UNSUPPORTED = -4, /* valid request outside what the kernels cover */
    PFZ_ERR_NOMEM = -5,
    PFZ_ERR_RCCL = -6
} pfz_status;

typedef struct pfz_ctx pfz_ctx;       /* one device + one stream + scratch */
typedef struct pfz_csr pfz_csr;       /* device-resident CSR matrix (fp32 values, sorted indices) */
typedef struct pfz_index pfz_index;   /* device-resident inverted index of a to-side CSR */
typedef struct pfz_topn pfz_topn;     /* device-resident (idx int32, score fp32)[n_rows][ntop] */
typedef struct pfz_strings pfz_strings; /* device-resident packed string list */
typedef struct pfz_tfidf pfz_tfidf;   /* fitted vectoriser: vocabulary + idf */
typedef struct pfz_comm pfz_comm;     /* RCCL communicator bound to a context (one process per GPU) */
typedef struct pfz_pairs pfz_pairs;   /* device-resident pair list of a threshold join: sorted keys row << 32 | col + fp32 scores */

/* ---- library / context -------------------------------------------------- */
int pfz_version(void);
const char *pfz_last_error(void);
/* number of HIP devices, 0 if none (never an error) */
int pfz_device_count(void);
int pfz_ctx_create(int device, pfz_ctx **out);
void pfz_ctx_destroy(pfz_ctx *ctx);
int pfz_ctx_sync(pfz_ctx *ctx);
/* device properties of the context: name (<=255 chars), CU count, HBM bytes */
int pfz_ctx_info(pfz_ctx *ctx, char *name256, int32_t *n_cu, int64_t *hbm_bytes);
/* the context's caching allocator: bytes in blocks that handles and running calls hold, bytes it keeps for re-use */
int pfz_pool_stats(pfz_ctx *ctx, int64_t *live_bytes, int64_t *cached_bytes);
/* Diagnostic, in the spirit of pfz_prof_enable: what the allocator's blocks hold when they are handed out.  The contents of a block
 * are UNSPECIFIED -- a fresh block is whatever the runtime gives (very often zero), a cached one holds what its last user left -- and
 * every entry point must compute the same result whatever they are.  Mode 0 (the default) leaves the allocator as it is: it does
 * not clear, and the only cost is one branch per allocation.  Modes 1 to 3 fill every block handed out from then on, fresh or
 * cached, over its whole size class with one 64-bit little-endian word, and wait for the context's stream before returning (so work
 * on the side streams sees the fill as well; slow, for tests):
 *   1  ZERO   0x0000000000000000
 *   2  ONE64  0x0000000000000001  every 8-, 16-, 32- or 64-bit integer view reads 0 or 1: an index, length, count or offset that
 *                                 nobody wrote stays in range everywhere
 *   3  ONE32  0x0000000100000001  every 32-bit word reads 1 (ONE64 leaves the odd ones at 0); a 64-bit view reads 2^32 + 1, so run
 *                                 it only where ONE64 has shown no dependence
 * A result that differs between two modes depends on memory nobody wrote.  BLIND SPOT: as floats all three patterns are zero or
 * denormals of about 0 (1.4e-45, 4.9e-324), so a float accumulator that is not cleared is NOT detected; NaN and large patterns are
 * left out on purpose -- a missed initialisation must show as a wrong answer, never as a wild address.  The context's scratch buffer
 * and the pinned staging buffers are no pool blocks and are not filled.  Any other mode: PFZ_ERR_INVALID. */
int pfz_pool_fill(pfz_ctx *ctx, int32_t mode);

/* HIP-event timers on the context's stream (used by bench.py for the live
 * per-kernel timing the roofline is computed from).  slot in [0, 64). */
int pfz_event_record(pfz_ctx *ctx, int32_t slot);
/* blocks until both events completed */
int pfz_event_elapsed_ms(pfz_ctx *ctx, int32_t slot_begin, int32_t slot_end, float *ms);
/* `bytes` of the context's PINNED staging buffer for the caller to fill (*host; NULL when the request is too large for it): what is
 * handed to pfz_strings_upload from there is read by the DMA where it lies -- the host's string packer (the lists of reference
 * _base.py:13-16, `match(from_list, to_list)`) writes offsets and code units straight into it instead of into a buffer that is then
 * copied into it.  Valid until the next upload or download on this context. */
int pfz_stage_reserve(pfz_ctx *ctx, int64_t bytes, void **host);
/* block until event slot `slot` has fired (recorded by pfz_event_record, or by pfz_cossim_topn_ranges for its row ranges -- those
 * are also announced through a word in pinned host memory, which this call polls instead of sleeping on the runtime's event) */
int pfz_event_wait(pfz_ctx *ctx, int32_t slot);
/* per-kernel profile: when enabled, every launch of the named hot kernels is
 * bracketed by its own event pair (adds a little launch overhead: ~2 % of a 100k x 100k step).
 * on = 1: every profiled kernel; on = 2: only the dominant ones (k3_cossim_topn, k4_indel, k5_gemm_panel). */
int pfz_prof_enable(pfz_ctx *ctx, int32_t on);
int pfz_prof_reset(pfz_ctx *ctx);
/* total ms and launch count of kernel `name` since the last reset (blocks).  Every form of K3 is timed as
 * `k3_cossim_topn`; `k3_lockstep` (0 ms, a count only) says how many of those launches the lock-step form served.
 * K4: `k4_indel` (every launch of a call), `k4_indel_general` (its general-kernel launch, merge included), `k4_general_rows`
 * (0 ms; the count is the number of from-rows the general kernel took), `k4_quad_launches` (0 ms; the count is the number of
 * quad / octo launches: several short from-strings per workgroup pass).
 * K8: `k8_jaro` (every launch of a call), `k8_jaro_general` (its general-kernel launches), `k8_pairs_scored` (0 ms; the
 * count is the number of pairs whose float64 score was computed).
 * K9: `k9_lev` (every launch of a call), `k9_lev_general` (its general-kernel launches), `k9_pairs_walked` (0 ms; the count is
 * the number of pairs whose recurrence was walked -- the others fell to the length bound).
 * K11: `k11_join` (the walk of a call), `k11_join_general` (its general-kernel launch), `k11_sort_unpack` (the hits sorted and
 * turned into CSR).
 * K12: `k12_walk` (the walk of a call, hooks included), `k12_walk_general` (its general-kernel launch), `k12_flatten` (the
 * forest turned into labels).
 * K14: `k14_join` (the tile kernel of a call), `k14_sort_unpack` (the hits sorted with their scores and turned into CSR),
 * `k14_components` (forest, tile kernel with its hooks, labels).
 * K15: `k15_join` (the row walk of a call), `k15_sort_unpack` (the hits sorted with their scores and turned into CSR),
 * `k15_components` (forest, row walk with its hooks, labels).
 * K16: `k16_keys_sort` (keys, sort and row pointers), `k16_pairs_join` (the scoring launches of a call, either sink),
 * `k16_pairs_join_general` (its general-kernel launch), `k16_compact` (the join's scan and compaction).
 * K17 (the key entries): K16's scopes -- `k16_keys_sort` then holds the row pointers alone --, `k17_items` (the work items: count,
 * scan, fill); pfz_cossim_join_dev: `k15_join` once per launch, `k15_sort`.
 * K22: `k22_search` (the 16-bit tile kernel, both runs of a repeated search), `k22_rescore` (the candidates scored on the fp32
 * vectors; for the components with forest and labels), `k22_sort_unpack`. */
int pfz_prof_get(pfz_ctx *ctx, const char *name, double *total_ms, int64_t *launches);

/* ---- CSR matrices --------------------------------------------------------
 * The layout scipy.sparse.csr_matrix uses for TfidfVectorizer output
 * (reference _tfidf.py:110-111): indptr[n_rows+1], indices[nnz] sorted per
 * row, data[nnz].  Values are converted to fp32 by the caller. */
int pfz_csr_upload(pfz_ctx *ctx, int64_t n_rows, int64_t n_cols,
                   const int64_t *indptr, const int32_t *indices, const float *data,
                   pfz_csr **out);
int pfz_csr_shape(const pfz_csr *m, int64_t *n_rows, int64_t *n_cols, int64_t *nnz);
/* blocks; any of the three output pointers may be NULL */
int pfz_csr_download(pfz_ctx *ctx, const pfz_csr *m, int64_t *indptr, int32_t *indices, float *data);
void pfz_csr_free(pfz_csr *m);

/* ---- K3: sparse cosine top-n ---------------------------------------------
 * Replaces sparse_dot_topn.awesome_cossim_topn(from, to.T, top_n+1, min_sim)
 * as called at reference polyfuzz/models/_utils.py:82, fused with the
 * diagonal removal of _utils.py:84-87 and the per-row top-n extraction of
 * _utils.py:89-91,128-146.
 *
 * pfz_index_build: device-side inverted index (n-gram id -> postings, split
 * by to-row block) of the to-side matrix; built once per fit and kept
 * resident (reference keeps self.tf_idf_to, _tfidf.py:110).  */
int pfz_index_build(pfz_ctx *ctx, const pfz_csr *to_matrix, pfz_index **out);
void pfz_index_free(pfz_index *ix);
/* bytes of postings + offset table (for the bench's byte accounting) */
int pfz_index_info(const pfz_index *ix, int64_t *n_rows, int64_t *n_cols, int64_t *nnz,
                   int64_t *block_cols, int64_t *n_blocks, int64_t *table_bytes);
/* the index stores every (n-gram, to-block) posting list padded to whole pieces of `piece_postings`
 * (16) postings = one 128-byte line each: number of pieces (index bytes = 128 * (n_pieces + 1)) */
int pfz_index_pieces(const pfz_index *ix, int64_t *n_pieces, int64_t *piece_postings);
/* how often pfz_cossim_topn[_rows] on this index took the symmetric form (a list against itself, reference
 * _tfidf.py:113-116 -> _utils.py:82-87: every unordered pair of rows scored once, csrc/k3_symmetric.hip), and how many
 * from-rows those launches covered -- the bench prices its roofline by the kernel that ran */
int pfz_index_symmetric_launches(const pfz_index *ix, int64_t *launches, int64_t *rows);
/* census of the LAST symmetric launch on this index (waits for the stream): rows taken out of the hand-over because of
 * their low own-block threshold ("magnets": they fetch their matches below their own block themselves) and rows that were
 * sent more candidates than their push slots hold and were recomputed row-major -- what the tests of those two paths assert
 * (nothing to replace in the reference: the exchange only exists because every unordered pair is scored once) */
int pfz_index_symmetric_census(const pfz_index *ix, int64_t *magnet_rows, int64_t *recomputed_rows);

int pfz_topn_alloc(pfz_ctx *ctx, int64_t n_rows, int32_t ntop, pfz_topn **out);
void pfz_topn_free(pfz_topn *t);
/* set every entry to "no match" (idx -1, score 0); enqueues */
int pfz_topn_clear(pfz_ctx *ctx, pfz_topn *t);
/* blocks; out_idx / out_val are [n_rows * ntop] row-major host buffers */
int pfz_topn_download(pfz_ctx *ctx, const pfz_topn *t, int32_t *out_idx, float *out_val);
/* download rows [row_begin, row_end) as soon as the event recorded in `event_slot` (pfz_event_record) has fired: the
 * copy goes through a side stream, so work enqueued on the context stream after the event is not waited for.  Blocks. */
int pfz_topn_download_rows_after(pfz_ctx *ctx, const pfz_topn *t, int64_t row_begin, int64_t row_end,
                                 int32_t event_slot, int32_t *out_idx, float *out_val);
/* The same in two halves, without the copy into caller buffers: _begin enqueues the side stream's wait for the event and the two
 * device-to-host copies into pinned staging half `half` (0 / 1) and returns; _finish waits for them and hands out the pinned
 * pointers (valid until the next _begin on that half).  A caller that consumes range i while range i + 1 is already on its way
 * (the frame's column fills of reference _utils.py:104-125) alternates the halves. */
int pfz_topn_rows_begin(pfz_ctx *ctx, const pfz_topn *t, int64_t row_begin, int64_t row_end, int32_t event_slot, int32_t half);
int pfz_topn_rows_finish(pfz_ctx *ctx, int32_t half, const int32_t **idx, const float **val);
/* fill a result buffer from host arrays [n_rows * ntop] (results computed elsewhere, e.g. another rank's block) */
int pfz_topn_upload(pfz_ctx *ctx, pfz_topn *t, const int32_t *idx, const float *val);
/* raw device pointers (for an RCCL all-gather issued by the caller) */
int pfz_topn_device_ptrs(const pfz_topn *t, void **idx_dev, void **val_dev, int64_t *n_rows, int32_t *ntop);

/* For every from-row i: the ntop largest cosine scores C[i][j] = sum_k
 * A[i][k] * B[j][k] with C[i][j] > lower_bound (strict, as sparse_dot_topn),
 * ordered by (score desc, j asc).  Every product is computed in fp32, scaled by
 * 2^30 / (norm bound) and truncated to int32; the sums are int32 (order-
 * independent, bit-reproducible).  Truncation makes the error one-sided and lets it grow with the rows: a score is at
 * most c * 2^-30 * (norm bound) + 3e-7 below the exact one for a pair with c columns in common -- ~1e-8 for company
 * names (c ~ 13), inside 1e-5 up to about 10 000 shared n-grams per pair, beyond it for longer documents
 * (docs/K3_DOCUMENT_ROWS.md).  exclude_diag != 0 drops j == i + diag_offset (self-match,
 * _utils.py:84-87; diag_offset = global index of from-row 0 when the from
 * side is a row shard).  lower_bound < 0 is treated as 0 (non-positive scores
 * are "no match" in the reference's output contract, _utils.py:122-123).
 * When from_matrix IS the matrix the index was built from, exclude_diag != 0 and diag_offset == 0 -- a list against
 * itself -- lists of 20 480 to 250 000 rows (ntop <= 32) take the symmetric form: C is symmetric bit for bit in this
 * arithmetic, so every unordered pair of rows is scored once and handed to both rows; same results (PFZ_K3_SYM=0 / 1:
 * never / whenever possible).
 * Limits: ntop >= 1 (above 128 a larger, slower candidate buffer; above 1024 passes of 1024, each continuing below the
 * last key of the one before -- the reference clips top_n to the number of distinct to-strings only, _utils.py:54-56); fewer than 2^25
 * 16-posting index pieces (4 GiB) in the to-side; n_cols equal on both sides.  `out` may have MORE rows than the from-matrix (a padded
 * shard buffer for the equal-sized all-gather): the extra rows are not touched.
 * Enqueues on the context stream. */
int pfz_cossim_topn(pfz_ctx *ctx, const pfz_index *to_index, const pfz_csr *from_matrix,
                    int32_t ntop, float lower_bound, int32_t exclude_diag, int64_t diag_offset,
                    pfz_topn *out);

/* The same for from-rows [row_begin, row_end) only (results into the same rows of `out`; exclude_diag still means
 * j == global from-row + diag_offset).  Lets a caller split one match into launches and consume the first part
 * (pfz_event_record + pfz_topn_download_rows_after) while the next one runs.  (Row ranges of a self-match that ascend
 * from row 0 without gaps, into the same `out`, continue one symmetric session; any other order is served row by row.) */
int pfz_cossim_topn_rows(pfz_ctx *ctx, const pfz_index *to_index, const pfz_csr *from_matrix,
                         int64_t row_begin, int64_t row_end, int32_t ntop, float lower_bound,
                         int32_t exclude_diag, int64_t diag_offset, pfz_topn *out);

/* The whole match, its results handed on in n_ranges ascending row ranges: range i = from-rows [range_ends[i-1], range_ends[i])
 * (the last one ends at the matrix' last row); event slot first_event + i fires when the rows of range i are final in `out`
 * (consume them with pfz_topn_rows_begin / _finish or pfz_topn_download_rows_after while the device works on).  What
 * `TFIDF.match` (reference _tfidf.py:68-100 -> _utils.py:82-125) enqueues for a big list, so that the frame's columns are built
 * under the device's work.  A list against itself in the symmetric form with range ends on multiples of 2048 rows runs ONE
 * pass-1 launch whose ranges are merged on a side stream as their blocks complete; anything else is a launch per range.
 * host_idx / host_val (may be NULL): where that streamed form runs, *host_idx / *host_val come back as int32 [n_rows][ntop] /
 * fp32 [n_rows][ntop] in PINNED HOST memory of the context that the device fills beside `out` -- rows of range i are there once
 * pfz_event_wait(first_event + i) has returned; valid until the next call with a mirror on this context --, NULL otherwise (then:
 * pfz_topn_rows_begin / _finish).  diag_offset is 0.  Enqueues. */
int pfz_cossim_topn_ranges(pfz_ctx *ctx, const pfz_index *to_index, const pfz_csr *from_matrix, int32_t ntop, float lower_bound,
                           int32_t exclude_diag, int32_t n_ranges, const int64_t *range_ends, int32_t first_event, pfz_topn *out,
                           const int32_t **host_idx, const float **host_val);

/* One-shot host convenience: upload both CSR matrices, build the index, run
 * pfz_cossim_topn, download.  Blocks. */
int pfz_cossim_topn_host(pfz_ctx *ctx,
                         int64_t n_from, int64_t n_to, int64_t n_cols,
                         const int64_t *from_indptr, const int32_t *from_indices, const float *from_data,
                         const int64_t *to_indptr, const int32_t *to_indices, const float *to_data,
                         int32_t ntop, float lower_bound, int32_t exclude_diag,
                         int32_t *out_idx, float *out_val);

/* ---- K1/K2: char-n-gram TF-IDF vectorisation ------------------------------
 * Replaces TfidfVectorizer(min_df=1, analyzer=TFIDF._create_ngrams)
 * .fit/.transform as used at reference _tfidf.py:102-118 (sklearn
 * feature_extraction/text.py: vocabulary = sorted distinct n-grams, tf = raw
 * count, idf = ln((1+n)/(1+df))+1, rows L2-normalised).
 *
 * Strings are passed as code units of `char_width` bytes (1: Latin-1/ASCII
 * code points, 4: UTF-32 code points), concatenated, with n+1 offsets (in
 * code units).  Cleaning (reference _tfidf.py:142-146) of ASCII input is done
 * on the device; the host must pre-clean strings that contain non-ASCII code
 * points (str.lower() is Unicode-aware) and pass clean = 0 for those. */
int pfz_strings_upload(pfz_ctx *ctx, const void *chars, const int64_t *offsets, int64_t n_strings,
                       int32_t char_width, pfz_strings **out);
void pfz_strings_free(pfz_strings *s);

typedef struct pfz_tfidf_params {
    int32_t ngram_lo, ngram_hi;   /* inclusive, reference n_gram_range */
    int32_t clean;                /* reference clean_string (ASCII fast path) */
    int32_t remove_space_ngrams;  /* reference remove_space_ngrams */
} pfz_tfidf_params;

/* Fit the vocabulary and idf on the concatenation docs_a + docs_b (either may
 * be NULL) -- reference: fit(to_list + from_list), _tfidf.py:109,114. */
int pfz_tfidf_fit(pfz_ctx *ctx, const pfz_tfidf_params *params,
                  const pfz_strings *docs_a, const pfz_strings *docs_b, pfz_tfidf **out);
void pfz_tfidf_free(pfz_tfidf *v);
/* vocabulary size, number of fitted documents, bits of the packed n-gram code */
int pfz_tfidf_info(const pfz_tfidf *v, int64_t *vocab_size, int64_t *n_docs, int32_t *code_bits);
/* blocks; ngrams[vocab * ngram_hi] = the vocabulary in column order, each
 * n-gram as ngram_hi UTF-32 code points (shorter n-grams 0-padded on the
 * right) -- independent of the device-side code packing; idf[vocab] fp64
 * (sklearn idf_), df[vocab].  Any pointer may be NULL. */
int pfz_tfidf_export(pfz_ctx *ctx, const pfz_tfidf *v, uint32_t *ngrams, double *idf, int64_t *df);
/* Re-create a fitted vectoriser from exported state (joblib load path,
 * reference polyfuzz.py:429-457).  ngrams must be sorted as exported. */
int pfz_tfidf_import(pfz_ctx *ctx, const pfz_tfidf_params *params, int64_t vocab_size, int64_t n_docs,
                     const uint32_t *ngrams, const double *idf, pfz_tfidf **out);
/* Vectorise a string list with a fitted vocabulary (out-of-vocabulary n-grams
 * are ignored, sklearn text.py:1271-1273).  Enqueues; result resident. */
int pfz_tfidf_transform(pfz_ctx *ctx, const pfz_tfidf *v, const pfz_strings *docs, pfz_csr **out);

/* ---- K4: all-pairs Indel ratio + row arg-max ------------------------------
 * Replaces the hot loop of EditDistance._calculate_edit_distance
 * (reference polyfuzz/models/_distance.py:89-102) with scorer =
 * rapidfuzz.fuzz.ratio (_distance.py:4,32): for every from-string the FIRST
 * to-string with the maximal ratio (np.argmax, _distance.py:99) and that
 * ratio as float64 = (1 - (|a|+|b|-2*LCS)/(|a|+|b|)) * 100 (100 when both
 * are empty).  skip_idx (host, one entry per from-string of the whole list, or
 * NULL) restates list.remove(from_string) of the self-match path
 * (_distance.py:93-96): skip_idx[i] is the index of the FIRST to-entry equal
 * to from-string i (-1: none) and is not a candidate for row i.  A code
 * skip_idx[i] <= -2 leaves out EVERY to-entry up to and including -2 - skip_idx[i]:
 * the RapidFuzz matcher's shared list that shrinks as its rows are processed
 * (_rapidfuzz.py:103-104 with n_jobs = 1: -2 - i for row i); a row that is left
 * without a candidate gets index -1, score 0.  One call uses one of the two
 * forms (entries >= 0, or codes <= -2; -1 goes with either): PFZ_ERR_INVALID otherwise.
 * Rows [from_begin, from_end) are scored (a row shard); out_idx / out_score
 * are host buffers of from_end - from_begin entries.  Blocks. */
int pfz_indel_argmax(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings,
                     const int32_t *skip_idx, int64_t from_begin, int64_t from_end,
                     int32_t *out_idx, double *out_score);
/* pfz_indel_argmax with the result left on the device in the layout the sharded jobs all-gather: `out` must have 2
 * columns and >= from_end - from_begin rows; row r gets idx[r][0] = the first arg-max (idx[r][1] = -1) and the
 * float64 ratio's bits in its two value lanes.  Enqueues. */
int pfz_indel_argmax_dev(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings,
                         const int32_t *skip_idx, int64_t from_begin, int64_t from_end, pfz_topn *out);
/* every ratio of rows [from_begin, from_end) x all to-strings as float64,
 * row-major host buffer (test / small-input entry point).  Blocks. */
int pfz_indel_matrix_host(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings,
                          int64_t from_begin, int64_t from_end, double *out_matrix);
/* The ntop best choices of every from-string of rows [from_begin, from_end) under rapidfuzz.fuzz.ratio: extends
 * the np.argmax / np.max of the reference's loop (polyfuzz/models/_distance.py:89-102) to what
 * np.argsort(-scores, kind="stable")[:ntop] gives on the scores that loop computes -- float64 ratio descending, equal
 * ratios by ascending to-index -- so column 0 is pfz_indel_argmax's result.  out_idx / out_score: host buffers of
 * (from_end - from_begin) * ntop entries, row-major; the slots beyond the choices a row has (skip_idx as in
 * pfz_indel_argmax; ntop may exceed the to-list) carry -1 / 0.0.  Exact: every pair is scored, every wave keeps one
 * sorted list of ntop keys (csrc/topn_wave.h).  ntop < 1: PFZ_ERR_INVALID; ntop > 64: PFZ_ERR_UNSUPPORTED.  Blocks. */
int pfz_indel_topn(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings,
                   const int32_t *skip_idx, int64_t from_begin, int64_t from_end, int32_t ntop,
                   int32_t *out_idx, double *out_score);
/* K4's preparation of a to-list -- alphabet (distinct code points of the to-list), to-strings sorted by
 * length into groups of 64, symbols packed per group on the device -- depends on the to-list alone: it is
 * built on the first pfz_indel_* call that uses the handle as the to-side and cached on it, so matching
 * further from-lists against the same pfz_strings (reference PolyFuzz.transform, polyfuzz.py:234-240)
 * costs no preparation.  This entry builds the plan if needed and reports it: alphabet size, groups,
 * and sum over to-strings of their padded length (x n_from x ceil(|from| / word) = the kernel's word-steps). */
int pfz_indel_plan_info(pfz_ctx *ctx, const pfz_strings *to_strings, int64_t *n_symbols, int64_t *n_groups,
                        int64_t *char_steps);

/* ---- K7: the per-pair rapidfuzz scorers -------------------------------------
 * Replaces process.extractOne(from_string, to_list, scorer=..., score_cutoff=...) of the reference's RapidFuzz
 * matcher (_rapidfuzz.py:99-113; scorer default fuzz.WRatio, _rapidfuzz.py:48) for the scorers that build a
 * different string pair per (from, to): the best choice (first maximum) of every from-string of rows
 * [from_begin, from_end) among all to-strings.
 * Everything is prepared on the device from the two resident lists: the three forms of every string -- 0: the string,
 * 1: its whitespace tokens (Python's str.split()) sorted and joined by one space (fuzz.token_sort_ratio's operand),
 * 2: its DISTINCT tokens sorted and joined (fuzz.token_set_ratio's) -- are built once per list and cached on its
 * handle; the to-side plan (alphabet of the to-list, token table, length-sorted groups of 64 with symbols / token ids /
 * character-class histograms) once per to-list, cached on ITS handle, so matching further from-lists against the same
 * pfz_strings (reference PolyFuzz.transform, polyfuzz.py:234-240) costs no preparation.
 * scorer: 0 WRatio, 1 partial_ratio, 2 token_set_ratio, 3 token_ratio, 4 partial_token_sort_ratio,
 * 5 partial_token_set_ratio, 6 partial_token_ratio (ratio / QRatio / token_sort_ratio are one string per list
 * element: pfz_indel_argmax).  skip_idx (host, one entry per from-string of the whole list, or NULL): a to-index
 * left out for from-string i (self-match: the first list element equal to it), or a code <= -2: every to-index up to
 * and including -2 - skip_idx[i] is left out (the reference's shared, shrinking list, _rapidfuzz.py:103-104; see pfz_indel_argmax).
 * out_idx[i] = -1 / out_score[i] = 0 when there is no choice; scores are rapidfuzz's 0..100 float64.
 * Strings of any length and token count are accepted: from-strings beyond 256 characters or 32 distinct tokens (and
 * to-strings beyond 32 distinct tokens) take a general -- slow -- kernel.  out_idx / out_score: host buffers of
 * from_end - from_begin entries.  Blocks. */
int pfz_fuzz_extract_one(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, int32_t scorer,
                         const int32_t *skip_idx, int64_t from_begin, int64_t from_end, int32_t *out_idx, double *out_score);
/* The same with the result left on the device, in the layout the sharded jobs all-gather ("shard
 * from-strings, replicate to-strings"): `out` must have 2 columns and >= from_end - from_begin rows; row r gets
 * idx[r][0] = the first best index (idx[r][1] = -1) and the float64 score's bits in its two value lanes.  Enqueues.
 * work_counters (host, 4 entries, or NULL): pairs whose upper bound was computed, pairs scored exactly, 64-bit
 * word-steps of the scored pairs (an estimate from their lengths), 0 -- the bench's work accounting; blocks if given. */
int pfz_fuzz_extract_one_dev(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, int32_t scorer,
                             const int32_t *skip_idx, int64_t from_begin, int64_t from_end, pfz_topn *out,
                             uint64_t *work_counters);
/* builds (once) and describes K7's cached plan of a to-list: alphabet size, groups of 64, distinct tokens over all
 * strings, strings with more than 32 distinct tokens (scored by the general kernel) */
int pfz_fuzz_plan_info(pfz_ctx *ctx, const pfz_strings *to_strings, int64_t *n_symbols, int64_t *n_groups, int64_t *n_tokens,
                       int64_t *n_general_strings);

/* ---- K18: all pairs at or above a score of the per-pair rapidfuzz scorers, and their components ----
 * The threshold form of K7: where the reference's RapidFuzz matcher keeps process.extractOne's single best choice
 * (_rapidfuzz.py:99-113), this is rapidfuzz.process.cdist(from, to, scorer=..., score_cutoff=c) /
 * process.extract(..., limit=None, score_cutoff=c) -- every pair that reaches the cutoff.
 * score(i, j) is exactly the float64 pfz_fuzz_extract_one computes for the pair (rapidfuzz's 0..100 scale), `scorer` as there
 * (0 WRatio .. 6 partial_token_ratio).  A pair is a hit iff score >= score_cutoff, float64 against float64 (equal is a hit).
 * pfz_fuzz_join: two lists -- every pair (from i, to j).  to_strings == NULL or the from-list's own handle is the self-join: every
 * pair i < j once, as row i, to-index j, scored as scorer(strings[i], strings[j]); never (i, i); equal strings at other positions
 * are pairs like any other (a string without a token scores 0 with its copy under WRatio and the token-set scorers, and is then
 * no pair above a cutoff of 0).  Row i of a self-join scores the choices behind it: K7's "up to" skip code -2 - i
 * (pfz_fuzz_extract_one), which the entry generates itself.
 * The output is CSR over the from-rows in host buffers -- out_row_ptr int64[n_from + 1], and per hit out_idx (the to-index,
 * ascending within a row) and out_score (the 0..100 float64); the same call gives the same bytes every time.  capacity: the
 * hits the two arrays have room for (they may be NULL when it is 0); *out_total is always the exact number of hits; when it
 * exceeds `capacity` the call returns PFZ_OK, has written NONE of the three output arrays (the device never writes a hit past the
 * capacity either) and is to be repeated with capacity >= *out_total.  out_counters: NULL, or int64[3] -- [0] pairs whose upper
 * bound was computed, [1] pairs scored exactly, [2] 64-bit word-steps of the scored pairs (K7's estimate from their lengths).
 * Exact: a pair is left unscored only where K7's upper bound of its score, plus K7's slack, is below the cutoff
 * (csrc/k18_core.h); the score of a pair that reaches the cutoff is exact (csrc/k7_core.h: fz_score with a fixed floor).
 * From-strings beyond 256 characters or 32 distinct tokens (and to-strings beyond 32 distinct tokens) take a general -- slow --
 * kernel.  The preparation is pfz_fuzz_extract_one's, cached on the handles.
 * scorer outside 0..6, a NaN score_cutoff or one outside [0, 100], capacity < 0: PFZ_ERR_INVALID.  K7's list limits (2^31 - 65
 * strings), and a capacity beyond 2^32 - 1: PFZ_ERR_UNSUPPORTED.  Blocks. */
int pfz_fuzz_join(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, int32_t scorer, double score_cutoff,
                  int64_t capacity, int64_t *out_row_ptr, int32_t *out_idx, double *out_score, int64_t *out_total,
                  int64_t *out_counters);
/* The connected components of "score >= score_cutoff" over ONE list (reference _rapidfuzz.py:99-113 asks for the one best choice
 * only; polyfuzz/linkage.py groups greedily over such a frame).  The pairs are those of pfz_fuzz_join(ctx, strings, NULL, scorer,
 * score_cutoff, ...), found by the same kernels and united where they are found in the lock-free union-find of csrc/k12_core.h:
 * O(n) device memory, no pair is stored.  out_label: host buffer int32[n], out_label[i] = the SMALLEST position in i's component;
 * deterministic.  *out_pairs == pfz_fuzz_join's *out_total; *out_components counts singletons too; out_counters as above.
 * strings->n == 0: PFZ_OK, *out_pairs = *out_components = 0, nothing else is written (out_label may be NULL).
 * Errors as pfz_fuzz_join (there is no capacity).  Blocks. */
int pfz_fuzz_components(pfz_ctx *ctx, const pfz_strings *strings, int32_t scorer, double score_cutoff, int32_t *out_label,
                        int64_t *out_pairs, int64_t *out_components, int64_t *out_counters);
/* K19: the ntop best choices of every from-string of rows [from_begin, from_end) under the per-pair scorers --
 * rapidfuzz.process.extract(query, choices, scorer=fuzz.WRatio, limit=ntop, score_cutoff=c), where the reference's matcher
 * (_rapidfuzz.py:99-113) asks for the one best.  Per row: the choices not left out (skip_idx as in pfz_fuzz_extract_one: >= 0 one
 * choice, <= -2 every choice up to -2 - code, -1 none) whose score -- exactly the float64 pfz_fuzz_extract_one computes for the
 * pair -- is >= score_cutoff (equal is kept), in the order np.argsort(-scores, kind="stable")[:ntop]: score descending, equal
 * scores by ascending to-index.  Column 0 at score_cutoff = 0 is pfz_fuzz_extract_one's result.  out_idx / out_score: host
 * buffers of (from_end - from_begin) * ntop entries, row-major; the slots beyond the choices a row has (ntop may exceed the
 * to-list) carry -1 / 0.0.  An empty row range writes nothing; an empty to-list gives rows of -1 / 0.0; neither launches a kernel.
 * out_counters: NULL, or uint64[3] as pfz_fuzz_join's ([0] pairs bounded, [1] pairs scored, [2] word-steps).
 * Exact: the walk is pfz_fuzz_join's with the floor moving -- a pair is left unscored only where K7's upper bound of its score,
 * plus K7's slack, is STRICTLY below the score of the ntop-th best choice the wave holds (or below score_cutoff before it holds
 * ntop), so a tie with the ntop-th best is still scored and placed by its index (csrc/k7_join_walk.h, csrc/topn_wave.h).
 * Argument checks: a NULL handle, scorer outside 0..6, a row range outside the from-list, ntop < 1, a NaN score_cutoff or one
 * outside [0, 100], skip_idx mixing both code forms: PFZ_ERR_INVALID.  ntop > 64 (one list entry per lane of a wave), K7's list
 * limits: PFZ_ERR_UNSUPPORTED.  Blocks. */
int pfz_fuzz_topn(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, int32_t scorer, const int32_t *skip_idx,
                  int64_t from_begin, int64_t from_end, int32_t ntop, double score_cutoff, int32_t *out_idx, double *out_score,
                  uint64_t *out_counters);

/* ---- K8: all-pairs Jaro / Jaro-Winkler similarity + row arg-max --------------
 * Replaces the hot loop of EditDistance._calculate_edit_distance (reference
 * polyfuzz/models/_distance.py:89-102) with the `scorer` argument (_distance.py:32) set to
 * jellyfish.jaro_similarity (scorer = 0) or jellyfish.jaro_winkler_similarity (scorer = 1), the scorer of
 * the reference's custom-model tutorial: for every from-string of rows [from_begin, from_end) the FIRST
 * to-string with the maximal score (np.argmax, _distance.py:99) and that score, float64 on jellyfish's
 * 0..1 scale, on code points, with jellyfish's default arguments (no long_tolerance):
 *   r = max(max(|a|,|b|) / 2 - 1, 0); greedy matches within r positions, m of them; t = the number of k whose
 *   k-th matched characters of a and of b differ, halved rounding down;
 *   w = (m/|a| + m/|b| + (m - t)/m) / 3, 0 when m = 0 (so 0 when either string is empty);
 *   Jaro-Winkler: w > 0.7 becomes w + (l * 0.1) * (1 - w), l = common prefix, at most 4.
 * skip_idx, the row range and the -1 / 0 result of a row without a candidate: as pfz_indel_argmax.
 * Any length and any alphabet: from-strings of up to 64 characters against to-strings of up to 256 run in
 * registers, all other pairs in a general -- slow -- kernel.  The to-side preparation is pfz_indel_*'s,
 * cached on the to-list's handle.  PARITY UNPINNED: the scorers restate jellyfish's definition; jellyfish itself
 * is compared wherever it is installed (tests/test_jaro_cpu.py).
 * scorer outside {0, 1}: PFZ_ERR_INVALID.  out_idx / out_score: host buffers of from_end - from_begin
 * entries.  Blocks. */
int pfz_jaro_argmax(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, int32_t scorer,
                    const int32_t *skip_idx, int64_t from_begin, int64_t from_end, int32_t *out_idx, double *out_score);
/* pfz_jaro_argmax with the result left on the device in the layout of pfz_indel_argmax_dev (_distance.py:89-102): `out`
 * must have 2 columns and >= from_end - from_begin rows; row r gets idx[r][0] = the first arg-max (idx[r][1] = -1)
 * and the float64 score's bits in its two value lanes.  Enqueues. */
int pfz_jaro_argmax_dev(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, int32_t scorer,
                        const int32_t *skip_idx, int64_t from_begin, int64_t from_end, pfz_topn *out);
/* every score (_distance.py:32,97) of rows [from_begin, from_end) x all to-strings as float64, row-major host buffer
 * (test / small-input entry point).  Blocks. */
int pfz_jaro_matrix_host(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, int32_t scorer,
                         int64_t from_begin, int64_t from_end, double *out_matrix);

/* ---- K20: all pairs at or above a Jaro / Jaro-Winkler score, and their components ------
 * The threshold form of K8, the textbook rule of record linkage ("Jaro-Winkler >= 0.9"): every pair (from i, to j) with
 * w(i, j) >= min_similarity, w as defined for K8 (scorer = 0: Jaro, 1: Jaro-Winkler) and computed by the very function
 * pfz_jaro_argmax / pfz_jaro_matrix_host score with -- the same bits --, float64 against float64: equal is a hit, below is a
 * miss.  An empty string on either side scores 0.0: a hit iff min_similarity == 0.
 * pfz_jaro_join: the contract is pfz_lev_join's, word for word, without the distance array: to_strings == NULL or the
 * from-list's own handle is the self-join (every unordered pair i < j once, as row i, to-index j, scored as w(i, j) = w(j, i);
 * never (i, i); equal strings at different positions are pairs); the output is CSR over the from-rows in host buffers, the
 * to-index ascending within a row, out_sim[p] = w; the same call gives the same bytes every time; *out_total is always the
 * exact number of hits, and when it exceeds `capacity` the call returns PFZ_OK, has written NONE of the three output arrays
 * (the device never writes a hit past the capacity either) and is to be repeated with capacity >= *out_total.
 * out_counters: NULL, or int64[4] of work counts -- [0] pairs inside the length window (pairs of the call, in a self-join the
 * unordered ones, whose lengths alone do not put them below min_similarity), [1] those of them alive after the matching sweep
 * (not abandoned in it, their number of matches not below what min_similarity needs), [2] those of them whose float64 score
 * was computed, [3] to-characters the matching sweep walked for lanes still alive.
 * Exact: a pair is left out of the window, abandoned or left unscored only where K8's float32 upper bound of its score -- with
 * every character of the shorter string matched, or with the matches it has plus the to-characters still to come, none
 * transposed and the longest common prefix it can have, or with its own matches, prefix and transpositions -- plus the bound's
 * margin is below min_similarity (csrc/k8_core.h).
 * From-strings of up to 64 characters against to-strings of up to 256 run in registers, all other pairs (and alphabets whose
 * match table exceeds 60 KiB) in a general -- slow -- kernel that scores every pair of the window to its end.  The to-side
 * preparation is pfz_indel_*'s, cached on the to-list's handle.
 * Limits (PFZ_ERR_UNSUPPORTED beyond): K8's on lists and strings; a capacity of at most 2^32 - 1 hits.  scorer outside
 * {0, 1}, a NaN min_similarity or one outside [0, 1], capacity < 0: PFZ_ERR_INVALID.  Blocks. */
int pfz_jaro_join(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, int32_t scorer,
                  double min_similarity, int64_t capacity, int64_t *out_row_ptr, int32_t *out_idx, double *out_sim,
                  int64_t *out_total, int64_t *out_counters);
/* pfz_jaro_components: pfz_lev_components's contract under these scores -- out_label[i] = the smallest position in i's
 * component of the graph of pfz_jaro_join's self-join, found by the same walk, the pairs united on the device (csrc/k12_core.h)
 * and never stored: O(n) device memory, no capacity, no repeat; deterministic.  *out_pairs == pfz_jaro_join's *out_total for
 * the same arguments, *out_components counts singletons too; out_counters: NULL or int64[4] as above.  Equal non-empty strings
 * always share a component (they score 1.0); empty ones score 0.0 and stay apart above min_similarity = 0.  strings->n == 0:
 * PFZ_OK, *out_pairs = *out_components = 0, nothing else is written.  Errors as pfz_jaro_join's.  Blocks. */
int pfz_jaro_components(pfz_ctx *ctx, const pfz_strings *strings, int32_t scorer, double min_similarity, int32_t *out_label,
                        int64_t *out_pairs, int64_t *out_components, int64_t *out_counters);
/* K21: the ntop best choices of every from-string of rows [from_begin, from_end) under Jaro (scorer = 0) or Jaro-Winkler
 * (scorer = 1) -- rapidfuzz.process.extract(query, choices, scorer=JaroWinkler.similarity, limit=ntop, score_cutoff=c), where the
 * reference's loop (_distance.py:89-102) keeps the one np.argmax.  Per row: the choices not left out (skip_idx: pfz_jaro_argmax's
 * codes -- >= 0 one choice, <= -2 every choice up to -2 - code, -1 none) whose score -- exactly the float64 pfz_jaro_argmax /
 * pfz_jaro_matrix_host compute for the pair -- is >= score_cutoff (a number in [0, 1]; equal is kept), in the order
 * np.argsort(-scores, kind="stable")[:ntop]: score descending, equal scores by ascending to-index.  Column 0 at score_cutoff = 0
 * is pfz_jaro_argmax's result.  out_idx / out_score: host buffers of (from_end - from_begin) * ntop entries, row-major; the slots
 * beyond the choices a row has (ntop may exceed the to-list) carry -1 / 0.0.  An empty row range writes nothing; an empty
 * to-list gives rows of -1 / 0.0; neither launches a kernel.
 * out_counters: NULL, or uint64[4] of work counts -- [0] pairs whose matching sweep began (a real to-string in a group that was
 * not skipped), [1] those alive after it, [2] those whose float64 score was computed, [3] to-characters the matching sweep
 * walked for lanes still alive.  The counters depend on the order the waves run in; the result does not.
 * Exact: the walk is pfz_jaro_join's with the floor moving -- a pair is skipped, abandoned or left unscored only where K8's
 * float32 upper bound of its score plus the bound's margin is below the floor F = max(score_cutoff, the score of the ntop-th
 * best choice a wave of the row's workgroup holds), so a tie with the ntop-th best is still scored and placed by its index
 * (csrc/k8_core.h, csrc/k21_jaro_topn.hip, csrc/topn_wave.h).  From-strings of up to 64 characters against to-strings of up to 256
 * run in registers, all other pairs (and alphabets whose match table exceeds 60 KiB) in a general -- slow -- kernel that scores
 * every pair.
 * Argument checks: a NULL handle or output, scorer outside {0, 1}, a row range outside the from-list, ntop < 1, a NaN
 * score_cutoff or one outside [0, 1], skip_idx mixing both code forms: PFZ_ERR_INVALID.  ntop > 64 (one list entry per lane of
 * a wave), K8's list limits: PFZ_ERR_UNSUPPORTED.  Blocks. */
int pfz_jaro_topn(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, int32_t scorer, const int32_t *skip_idx,
                  int64_t from_begin, int64_t from_end, int32_t ntop, double score_cutoff, int32_t *out_idx, double *out_score,
                  uint64_t *out_counters);

/* ---- K9: all-pairs Levenshtein / OSA similarity + row arg-max -----------------
 * Replaces the hot loop of EditDistance._calculate_edit_distance (reference
 * polyfuzz/models/_distance.py:89-102) with the `scorer` argument (_distance.py:32) set to rapidfuzz's
 * Levenshtein.normalized_similarity (scorer = 0) or OSA.normalized_similarity (scorer = 1), default arguments, on
 * code points: for every from-string of rows [from_begin, from_end) the FIRST to-string with the maximal score
 * (np.argmax, _distance.py:99) and that score (np.max), float64 on the 0..1 scale, unscaled:
 *   d = the fewest unit-cost insertions, deletions and substitutions that turn a into b (Levenshtein); OSA (optimal
 *   string alignment) also counts the transposition of two adjacent characters as one edit, no substring edited
 *   twice: osa("CA","ABC") = 3 (unrestricted Damerau: 2), osa("ab","ba") = 1 (Levenshtein: 2);
 *   M = max(|a|, |b|);  sim = 1.0 - (double)d / (double)M, 1.0 when M = 0: one division, one subtraction, not fused.
 * skip_idx, the row range and the -1 / 0 result of a row without a candidate: as pfz_indel_argmax.
 * Any length and any alphabet: from-strings of up to 64 characters run in registers against to-strings of any
 * length, longer ones (and alphabets whose match table exceeds 60 KiB) in a general -- slow -- kernel.  The arg-max
 * walks a from-string's to-strings from the nearest length outwards and stops where d >= ||a| - |b|| puts every
 * further one strictly below the best so far.  The to-side preparation is pfz_indel_*'s, cached on the to-list's
 * handle.  PARITY UNPINNED: the scorers restate rapidfuzz's definition; rapidfuzz itself is compared wherever it
 * is installed (tests/test_levenshtein_cpu.py).
 * scorer outside {0, 1}: PFZ_ERR_INVALID.  out_idx / out_score: host buffers of from_end - from_begin
 * entries.  Blocks. */
int pfz_lev_argmax(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, int32_t scorer,
                   const int32_t *skip_idx, int64_t from_begin, int64_t from_end, int32_t *out_idx, double *out_score);
/* pfz_lev_argmax with the result left on the device in the layout of pfz_indel_argmax_dev (_distance.py:89-102): `out`
 * must have 2 columns and >= from_end - from_begin rows; row r gets idx[r][0] = the first arg-max (idx[r][1] = -1)
 * and the float64 score's bits in its two value lanes.  Enqueues. */
int pfz_lev_argmax_dev(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, int32_t scorer,
                       const int32_t *skip_idx, int64_t from_begin, int64_t from_end, pfz_topn *out);
/* The ntop best choices of every from-string of rows [from_begin, from_end) under the Levenshtein (scorer = 0) or OSA
 * (scorer = 1) similarity: extends the np.argmax / np.max of the reference's loop (polyfuzz/models/_distance.py:89-102)
 * to what np.argsort(-scores, kind="stable")[:ntop] gives on the scores that loop computes -- float64 score descending,
 * equal scores by ascending to-index -- so column 0 is pfz_lev_argmax's result.  out_idx / out_score: host buffers of
 * (from_end - from_begin) * ntop entries, row-major; the slots beyond the choices a row has (skip_idx as in
 * pfz_indel_argmax; ntop may exceed the to-list) carry -1 / 0.0.  Exact: a to-string is left unwalked only where
 * d >= ||a| - |b|| puts it strictly below a score that ntop walked choices of the row have reached (csrc/topn_wave.h).
 * ntop < 1: PFZ_ERR_INVALID; ntop > 64: PFZ_ERR_UNSUPPORTED.  Blocks. */
int pfz_lev_topn(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, int32_t scorer,
                 const int32_t *skip_idx, int64_t from_begin, int64_t from_end, int32_t ntop,
                 int32_t *out_idx, double *out_score);
/* every DISTANCE d of rows [from_begin, from_end) x all to-strings as int32, row-major host buffer (test / small-input
 * entry point; every pair is walked).  The similarity follows in one IEEE division and subtraction.  Blocks. */
int pfz_lev_matrix_host(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, int32_t scorer,
                        int64_t from_begin, int64_t from_end, int32_t *out_matrix);

/* ---- K11: all pairs at or above a Levenshtein / OSA similarity -----------------
 * The threshold form of K9, what deduplication and record linkage ask of the scores of the reference's loop
 * (polyfuzz/models/_distance.py:89-102; TFIDF has it as min_similarity, polyfuzz/models/_tfidf.py): every pair
 * (from i, to j) with sim(i, j) >= min_similarity, sim and d as defined for K9 (scorer = 0: Levenshtein, 1: OSA), float64
 * against float64 -- rapidfuzz's score_cutoff convention: equal is a hit, below is a miss.
 * to_strings == NULL, or the from-list's own handle: the self-join.  Every unordered pair i < j is reported once, as row i,
 * to-index j; never (i, i); equal strings at different positions are pairs.
 * Output, host buffers: CSR over the from-rows.  out_row_ptr int64[n_from + 1]; hit p of row i, out_row_ptr[i] <= p <
 * out_row_ptr[i + 1]: out_idx[p] the to-index (ascending within a row), out_dist[p] = d, out_sim[p] = sim.  The same call
 * gives the same bytes every time.
 * capacity: the hits out_idx / out_dist / out_sim have room for (they may be NULL when it is 0).  *out_total is always the
 * exact number of hits.  When it exceeds `capacity` the call still returns PFZ_OK, has written NONE of the four output arrays
 * (the device never writes a hit past the capacity either) and is to be repeated with capacity >= *out_total.
 * out_counters: NULL, or int64[3] of work counts -- [0] pairs inside the length window (pairs of the call, in a self-join
 * the unordered ones, whose lengths alone do not put them below min_similarity), [1] those of them walked to their end, not
 * abandoned, [2] recurrence steps (to-characters) lanes took for pairs still alive.
 * Exact: a pair is left unwalked or abandoned only where K9's formula, applied to a lower bound of d -- ||a| - |b||, or the
 * column's bottom cell less the to-characters still to come --, is < min_similarity (csrc/k11_core.h).
 * From-strings of up to 64 characters run in registers; longer ones (and alphabets whose match table exceeds 60 KiB) in a
 * general -- slow -- kernel.  The to-side preparation is pfz_indel_*'s, cached on the to-list's handle.
 * Limits of the packed hit (PFZ_ERR_UNSUPPORTED beyond): lists of at most 2^24 strings, strings of at most 65 535
 * characters.  scorer outside {0, 1}, a NaN min_similarity or one outside [0, 1], capacity < 0: PFZ_ERR_INVALID.  Blocks. */
int pfz_lev_join(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, int32_t scorer,
                 double min_similarity, int64_t capacity, int64_t *out_row_ptr, int32_t *out_idx, int32_t *out_dist,
                 double *out_sim, int64_t *out_total, int64_t *out_counters);

/* ---- K12: connected components of "Levenshtein / OSA similarity >= t" ----------
 * Near-duplicate clusters of ONE list: positions i and j share a component iff a chain of pairs, each with
 * sim >= min_similarity (sim, d, scorer and the float64 comparison as for K11's self-join: equal is a hit), leads from i to j.
 * "A ~ B and B ~ C put A, B and C together" -- which the reference's greedy single_linkage (polyfuzz/linkage.py:5-53) over a
 * frame of pairs does not promise.  Equal strings always share a component (they score 1.0).
 * The pairs are those of pfz_lev_join(ctx, strings, NULL, scorer, min_similarity, ...), found by the same walk, but none is
 * stored: the lane that finds a hit unites the two positions in a lock-free union-find on the device (csrc/k12_core.h).
 * Device memory is O(n) whatever the number of hits; there is no capacity and no repeat.
 * out_label: host buffer int32[n]; out_label[i] = the SMALLEST position in i's component (so out_label[i] <= i, and
 * out_label[i] == i exactly for the one representative of each component).  Deterministic: the same call gives the same bytes
 * every time, whatever order the device's atomics took.
 * *out_pairs: the number of hits, == pfz_lev_join's *out_total for the same arguments.  *out_components: the number of
 * components (singletons included).  out_counters: NULL, or int64[3] with pfz_lev_join's meaning and, for the same call, its
 * values.
 * strings->n == 0: PFZ_OK, *out_pairs = *out_components = 0, nothing else is written (out_label may be NULL).
 * Limits: K11's packed-hit limits do not apply.  Positions and lengths are 32-bit: more than 2^31 - 65 strings, or a string
 * of 2^31 - 1 characters or more, is PFZ_ERR_UNSUPPORTED, as is a string beyond 64 characters whose match table in the general
 * kernel would exceed 8 GiB.  scorer outside {0, 1}, a NaN min_similarity or one outside [0, 1], a NULL out_pairs /
 * out_components: PFZ_ERR_INVALID.
 * From-strings of up to 64 characters run in registers; longer ones (and alphabets whose match table exceeds 60 KiB) in a
 * general -- slow -- kernel.  The preparation is pfz_indel_*'s, cached on the handle.  Blocks. */
int pfz_lev_components(pfz_ctx *ctx, const pfz_strings *strings, int32_t scorer, double min_similarity, int32_t *out_label,
                       int64_t *out_pairs, int64_t *out_components, int64_t *out_counters);

/* ---- K13: all pairs at or above an Indel similarity, and their components ------
 * The threshold form of K4's metric on the 0..1 scale: rapidfuzz.distance.Indel.normalized_similarity, default arguments, on
 * code points.  lcs = the length of the longest common subsequence of a and b, S = |a| + |b|, d = S - 2 lcs (the fewest
 * insertions and deletions that turn a into b);  sim = 1.0 - (double)d / (double)S, 1.0 when S = 0 -- one division, one
 * subtraction, not fused.  rapidfuzz.fuzz.ratio (pfz_indel_argmax) is this value times 100.
 * pfz_indel_join: every pair (from i, to j) with sim(i, j) >= min_similarity, float64 against float64 (equal is a hit).  The
 * contract is pfz_lev_join's, word for word, without the scorer argument: to_strings == NULL or the from-list's own handle is
 * the self-join (every unordered pair i < j once, as row i, to-index j; never (i, i)); the output is CSR over the from-rows in
 * host buffers, the to-index ascending within a row, out_dist[p] = d = S - 2 lcs, out_sim[p] = sim; the same call gives the same
 * bytes every time.  capacity: the hits the three arrays have room for (they may be NULL when it is 0); *out_total is always
 * the exact number of hits; when it exceeds `capacity` the call returns PFZ_OK, has written NONE of the four output arrays (the
 * device never writes a hit past the capacity either) and is to be repeated with capacity >= *out_total.  out_counters: NULL,
 * or int64[3] with pfz_lev_join's meaning -- [0] pairs inside the length window, [1] those walked to their end, [2] recurrence
 * steps of live lanes.
 * Exact: a pair is left unwalked or abandoned only where the formula, applied to an upper bound of lcs -- min(|a|, |b|), or the
 * LCS so far plus the to-characters still to come --, is < min_similarity (csrc/k13_core.h).
 * From-strings of up to 64 characters run in registers; longer ones (and alphabets whose match table exceeds 60 KiB) in a
 * general -- slow -- kernel.  The to-side preparation is pfz_indel_*'s, cached on the to-list's handle.
 * Limits of the packed hit (row, to-index, lcs; PFZ_ERR_UNSUPPORTED beyond): lists of at most 2^24 strings, strings of at most
 * 65 535 characters.  A NaN min_similarity or one outside [0, 1], capacity < 0: PFZ_ERR_INVALID.  Blocks. */
int pfz_indel_join(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, double min_similarity,
                   int64_t capacity, int64_t *out_row_ptr, int32_t *out_idx, int32_t *out_dist, double *out_sim,
                   int64_t *out_total, int64_t *out_counters);
/* The connected components of "Indel similarity >= min_similarity" over ONE list; the contract is pfz_lev_components's without
 * the scorer argument.  The pairs are those of pfz_indel_join(ctx, strings, NULL, min_similarity, ...), found by the same walk
 * and united where they are found in the lock-free union-find of csrc/k12_core.h: O(n) device memory, no pair is stored or
 * downloaded.  out_label: host buffer int32[n], out_label[i] = the SMALLEST position in i's component; deterministic.
 * *out_pairs == pfz_indel_join's *out_total; *out_components counts singletons too; out_counters as above.
 * strings->n == 0: PFZ_OK, *out_pairs = *out_components = 0, nothing else is written (out_label may be NULL).
 * Limits: the packed-hit limits do not apply.  Positions and the sum of two lengths are 32-bit: more than 2^31 - 65 strings, or
 * a string of 2^30 characters or more, is PFZ_ERR_UNSUPPORTED, as is a string beyond 64 characters whose match table in the
 * general kernel would exceed 8 GiB.  A NaN min_similarity or one outside [0, 1], a NULL out_pairs / out_components:
 * PFZ_ERR_INVALID.  Blocks. */
int pfz_indel_components(pfz_ctx *ctx, const pfz_strings *strings, double min_similarity, int32_t *out_label,
                         int64_t *out_pairs, int64_t *out_components, int64_t *out_counters);

/* ---- K10: a candidate table rescored by edit distance ----------------------
 * Blocking, then exact scoring: extends the reference's edit-distance loop (polyfuzz/models/_distance.py:89-102: scorer(from, to)
 * for every to-string, then the best) restricted to the candidates a cheap matcher left per from-string (the top_n table of
 * polyfuzz/models/_utils.py:82-91, e.g. a pfz_cossim_topn result of the TF-IDF matrices of the same two lists).  `candidates` is a
 * result buffer of at least from_strings->n rows whose idx half holds, per from-row, indices into `to_strings`; its val half is
 * ignored, and the table is read on the device, never downloaded.  An index outside [0, n_to), the -1 of an empty slot among
 * them, is skipped wherever it stands; real indices are distinct within a row (not checked: pfz_dense_rescore_topn's contract).
 * For every candidate j of row i: score(from[i], to[j]) under `scorer` -- the float64 value, bit for bit, that pfz_indel_argmax
 * (ratio, 0..100, 100.0 for two empty strings), pfz_lev_argmax (Levenshtein / OSA, 0..1) and pfz_jaro_argmax (Jaro /
 * Jaro-Winkler, 0..1) compute for that pair, on the raw strings as uploaded.  Every valid candidate is scored; nothing is pruned.
 * out_idx / out_score: host buffers of from_strings->n * ntop entries, row-major: a row's candidates by (float64 score
 * descending, to-index ascending) -- np.argsort(-scores, kind="stable")[:ntop] over the row's valid candidates taken in
 * ascending index order --, the first ntop of them, then (-1, 0.0); ntop may exceed the candidates a row has.  The position of a
 * candidate inside its row does not influence the result.  Any length and any alphabet: from-strings of up to 64 characters run
 * in registers (Jaro: against candidates of up to 256 characters), everything else, and alphabets whose match table exceeds
 * 60 KiB, in a general -- slow -- kernel.  The to-side preparation is pfz_indel_*'s, cached on the to-list's handle.
 * PFZ_ERR_INVALID: a NULL argument, a scorer outside 0 .. 4, ntop < 1, fewer candidate rows than from-strings;
 * PFZ_ERR_UNSUPPORTED: more than 1024 candidates per row, ntop > 64 (one list entry per lane of a wave, csrc/topn_wave.h).
 * from_strings->n == 0: PFZ_OK, nothing is done.  Blocks. */
#define PFZ_PAIR_RATIO 0
#define PFZ_PAIR_LEVENSHTEIN 1
#define PFZ_PAIR_OSA 2
#define PFZ_PAIR_JARO 3
#define PFZ_PAIR_JARO_WINKLER 4
int pfz_pairs_rescore_topn(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings,
                           const pfz_topn *candidates, int32_t scorer, int32_t ntop, int32_t *out_idx, double *out_score);

/* ---- K16: the candidate pairs at or above an edit-distance similarity, and their components ----
 * The threshold form of K10: blocking, then "score >= min_similarity" on the few pairs the blocking left -- the record-linkage
 * rule ("Jaro-Winkler >= 0.9") at a size where all pairs (K11) are not an option, and the only threshold form Jaro and
 * Jaro-Winkler have.  `candidates` is K10's input: a result buffer of at least from_strings->n rows whose idx half holds, per
 * from-row, up to candidates->ntop indices into the to-list, read on the device, never downloaded; its val half is ignored.  An
 * index outside [0, n_to), the -1 of an empty slot among them, is skipped wherever it stands, and -- unlike K10 -- an index that
 * occurs twice in a row counts once.
 * Two lists: the candidate pairs are {(i, j) : j in row i}.
 * to_strings == NULL, or the from-list's own handle: the self-join.  The candidate pairs are the SYMMETRISED table: the unordered
 * {i, j}, i != j, with j in row i or i in row j.  Each is scored once and reported once as row min(i, j), to-index max(i, j),
 * with score(strings[min], strings[max]): the lower position is the from-string.  A row's own index in its row is skipped;
 * equal strings at different positions are a pair.
 * scorer: PFZ_PAIR_LEVENSHTEIN, _OSA, _JARO, _JARO_WINKLER (1 .. 4).  PFZ_PAIR_RATIO (0) is refused with PFZ_ERR_INVALID: it
 * lives on 0 .. 100, where a min_similarity in [0, 1] is ambiguous.  A pair's score is the float64 value, bit for bit, that
 * pfz_pairs_rescore_topn computes for it.  A pair is a hit iff score >= min_similarity, float64 against float64: equal is kept.
 * Exact among the candidate pairs: every one is scored to its end (no window, no abandon rule, no bound -- the table is short);
 * a pair the table does not hold is never scored.
 * Output of pfz_pairs_join, host buffers: CSR over the from-rows.  out_row_ptr int64[n_from + 1]; hit p of row i,
 * out_row_ptr[i] <= p < out_row_ptr[i + 1]: out_idx[p] the to-index (ascending within a row), out_sim[p] its score.
 * Deterministic: equal inputs give equal bytes, whatever order the columns of the table's rows stand in.
 * capacity: the hits out_idx / out_sim have room for (they may be NULL when it is 0).  *out_total is always the exact number of
 * hits.  When it exceeds `capacity` the call still returns PFZ_OK, has written NONE of the three output arrays (the device never
 * writes a hit past the capacity either) and is to be repeated with capacity >= *out_total.
 * out_counters: NULL, or int64[3] -- [0] the table cells that are a candidate pair (inside [0, n_to), not the row's own index
 * in a self-join; a repeated cell counts every time), [1] the distinct pairs scored, [2] the hits (== *out_total).
 * from_strings->n == 0, an empty to-list or candidates->ntop == 0: PFZ_OK, zero row pointers, *out_total = 0, no launch.
 * pfz_pairs_components: out_label int32[n], out_label[i] = the SMALLEST position in i's connected component of the graph whose
 * edges are the hits of pfz_pairs_join(ctx, strings, NULL, candidates, ...).  The hits are united where they are found, in the
 * lock-free forest of pfz_lev_components (csrc/k12_core.h), and never stored: no capacity, no repeat; deterministic.
 * *out_pairs == that join's *out_total, *out_components counts singletons too, out_counters as above.  strings->n == 0: PFZ_OK,
 * *out_pairs = *out_components = 0, nothing else is written (out_label may be NULL); candidates->ntop == 0: every string its
 * own label, no launch.
 * Any length and any alphabet: from-strings of up to 64 characters run in registers (Jaro: against partners of up to 256
 * characters), everything else, and alphabets whose match table exceeds 60 KiB, in a general -- slow -- kernel.  The to-side
 * preparation is pfz_indel_*'s, cached on the to-list's handle.  One wave serves a from-string's partners 64 at a time, however
 * many the symmetrised table gives it.
 * Call-scoped device memory: 8 B per table cell for the keys and 8 B per cell, the cells rounded up to a power of two, for
 * their sorted copy; pfz_pairs_join adds 8 B per cell for the scores and 4 B for the hit flags the scan runs over.
 * PFZ_ERR_INVALID: a NULL argument, scorer 0 or outside 1 .. 4, a NaN min_similarity or one outside [0, 1], capacity < 0, NULL
 * outputs with capacity > 0, fewer candidate rows than from-strings.  PFZ_ERR_UNSUPPORTED, with the limit in the message:
 * more than 1024 candidates per row (K10's limit), a list of 2^31 strings or more, n_from * candidates->ntop of 2^31 table cells
 * or more (the scan over them is 32-bit), a string of 2^30 - 1 characters or more.  Blocks. */
int pfz_pairs_join(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, const pfz_topn *candidates,
                   int32_t scorer, double min_similarity, int64_t capacity, int64_t *out_row_ptr, int32_t *out_idx,
                   double *out_sim, int64_t *out_total, int64_t *out_counters);
int pfz_pairs_components(pfz_ctx *ctx, const pfz_strings *strings, const pfz_topn *candidates, int32_t scorer,
                         double min_similarity, int32_t *out_label, int64_t *out_pairs, int64_t *out_components,
                         int64_t *out_counters);

/* ---- K17: a threshold join as the blocking key of K16 ----
 * A candidate table holds a fixed number of neighbours per row; a list whose clusters have thousands of members wants a
 * similarity instead.  pfz_pairs is a threshold join's result left on the device: n_from, n_to, a self flag, `count` distinct keys
 * row << 32 | col in ascending order and the float32 score beside each.  It belongs to the context that made it.
 * pfz_cossim_join_dev: pfz_cossim_join (K15) without the way back -- the same walk, then the sort; nothing is unpacked, nothing
 * but the call's state words is downloaded.  Operands, hit rule, limits and errors are pfz_cossim_join's; out_counters is its
 * int64[3], of the last launch.  The capacity is handled inside: the first launch has room for capacity_hint hits (0: max(4096,
 * 4 per from-row)); when the exact total exceeds that room there is exactly ONE repeat, with room for the exact total.
 * capacity_hint < 0: PFZ_ERR_INVALID.  An empty list on either side, or a threshold no sum reaches: a valid handle with count 0.
 * 2^31 pairs or more: PFZ_ERR_UNSUPPORTED (the scan of the kernels that walk the keys is 32-bit).  Device memory of the handle: 12
 * bytes per pair, the pairs rounded up to a power of two.  Profiling scopes: `k15_join` (once per launch), `k15_sort`.  Blocks
 * until the walk's total is known; the sort is enqueued.
 * pfz_pairs_free: NULL is allowed.  pfz_pairs_count: the number of pairs; pfz_pairs_shape: the sizes of the two lists the handle
 * was made for and whether it is a self-join's (any of the three outputs may be NULL).  pfz_pairs_download: the CSR pfz_cossim_join would
 * have returned for the same call, byte for byte -- out_row_ptr int64[n_from + 1], out_idx int32[count], out_sim float[count]
 * (the last two may be NULL when count is 0); for tests and for callers that want the pairs themselves.  Blocks.
 * pfz_pairs_join_keys / pfz_pairs_components_keys: pfz_pairs_join / pfz_pairs_components with the handle in place of the table.
 * The candidate pairs are exactly the handle's keys: (row, col) of a two-list handle; of a self handle the unordered pairs, each
 * once with row < col, scored with the lower position as the from-string.  Score, hit rule (score >= min_similarity, equal is
 * kept), output, order, capacity rule (NONE of the arrays written when *out_total exceeds the capacity), determinism and the
 * scorers (1 .. 4; PFZ_PAIR_RATIO is refused with the same message) are K16's; so are the components' labels, *out_pairs and
 * *out_components.  A handle with count 0, or an empty list: zero row pointers (every string its own label), no launch.
 * The keys are walked as they lie: no key kernel, no sort.  Where K16 gives a wave a from-row with all its partners, these entries
 * deal WORK ITEMS, (row, slice) with at most 64 partners (csrc/k17_core.h): behind a threshold a row's partners have no bound,
 * and a row of thousands would keep one wave busy long after the others are done.  Items are built on the device from the row
 * pointers (count, scan, fill); each sets up and clears its row's match table itself.  Jaro's hand-over of a partner beyond 256
 * characters to the general kernel is decided per item, so every pair is scored exactly once.
 * out_counters: NULL, or int64[4] -- [0] the keys, [1] the distinct pairs scored (== [0]), [2] the hits, [3] the work items.
 * Call-scoped device memory: 4 B per from-row for the row pointers, 8 B per from-row and 13 B per item for the items;
 * pfz_pairs_join_keys adds 12 B per key for the scores and the hit flags.
 * PFZ_ERR_INVALID: a NULL argument, scorer 0 or outside 1 .. 4, a NaN min_similarity or one outside [0, 1], capacity < 0, NULL
 * outputs with capacity > 0, a handle of another context, lists whose sizes differ from the handle's n_from / n_to, a self handle
 * with a to-list that is not the from-list's own handle, a two-list handle without a to-list, pfz_pairs_components_keys with a
 * two-list handle.  PFZ_ERR_UNSUPPORTED: K16's limits on the lists and their strings.  Blocks. */
int pfz_cossim_join_dev(pfz_ctx *ctx, const pfz_index *to_index, const pfz_csr *from_matrix, int32_t self_join,
                        double min_similarity, int64_t capacity_hint, pfz_pairs **out, int64_t *out_counters);
void pfz_pairs_free(pfz_pairs *pairs);
int pfz_pairs_count(const pfz_pairs *pairs, int64_t *out_count);
int pfz_pairs_shape(const pfz_pairs *pairs, int64_t *out_n_from, int64_t *out_n_to, int32_t *out_self_join);
int pfz_pairs_download(pfz_ctx *ctx, const pfz_pairs *pairs, int64_t *out_row_ptr, int32_t *out_idx, float *out_sim);
int pfz_pairs_join_keys(pfz_ctx *ctx, const pfz_strings *from_strings, const pfz_strings *to_strings, const pfz_pairs *pairs,
                        int32_t scorer, double min_similarity, int64_t capacity, int64_t *out_row_ptr, int32_t *out_idx,
                        double *out_sim, int64_t *out_total, int64_t *out_counters);
int pfz_pairs_components_keys(pfz_ctx *ctx, const pfz_strings *strings, const pfz_pairs *pairs, int32_t scorer,
                              double min_similarity, int32_t *out_label, int64_t *out_pairs, int64_t *out_components,
                              int64_t *out_counters);

/* ---- K5: dense cosine top-n -----------------------------------------------
 * Replaces cosine_similarity on dense embedding matrices
 * (reference _utils.py:74-77,95; Embeddings.match _embeddings.py:127-133):
 * rows are L2-normalised on the device (true cosine, as the sklearn branch),
 * fp32 MFMA product, fused per-row top-n. Host buffers; blocks. */
int pfz_dense_cossim_topn_host(pfz_ctx *ctx, const float *from_vec, int64_t n_from,
                               const float *to_vec, int64_t n_to, int64_t dim,
                               int32_t ntop, float lower_bound, int32_t exclude_diag,
                               int32_t *out_idx, float *out_val);
/* The same without the normalisation: raw dot products.  This is what the reference's
 * "sparse" back-end computes on dense input (_utils.py:74-82: the ndarrays are wrapped in
 * csr_matrix and multiplied as they are); Embeddings._embed hands it unit-norm rows
 * (_embeddings.py:136-145), user-supplied embeddings need not be. */
int pfz_dense_dot_topn_host(pfz_ctx *ctx, const float *from_vec, int64_t n_from,
                            const float *to_vec, int64_t n_to, int64_t dim,
                            int32_t ntop, float lower_bound, int32_t exclude_diag,
                            int32_t *out_idx, float *out_val);

/* The same operator with device-resident operands -- the to-side embeddings stay in HBM between
 * Embeddings.match(..., re_train=False) calls (reference polyfuzz.py:234-240) and a row shard of the
 * from-side is matched against a replicated to-side on every GPU (BASELINE config 5).  normalize != 0:
 * rows are scaled by 1/||row|| (true cosine), 0: raw dot products.  pfz_dense_topn enqueues on the
 * context stream and leaves (idx, score) in `out` (rows [0, n_from)); exclude_diag drops
 * j == i + diag_offset.  ntop >= 1 (beyond 1024 in passes of 1024 over the same score panel, each continuing below the last key of
 * the one before: the reference clips top_n to the number of distinct to-strings only, _utils.py:54-56). */
typedef struct pfz_dense pfz_dense;
int pfz_dense_upload(pfz_ctx *ctx, const float *vec, int64_t n, int64_t dim, int32_t normalize, pfz_dense **out);
int pfz_dense_shape(const pfz_dense *m, int64_t *n, int64_t *dim);
void pfz_dense_free(pfz_dense *m);
int pfz_dense_topn(pfz_ctx *ctx, const pfz_dense *from_vectors, const pfz_dense *to_vectors, int32_t ntop,
                   float lower_bound, int32_t exclude_diag, int64_t diag_offset, pfz_topn *out);

/* 16-bit operands for the same operator (reference _embeddings.py:127-133 on float16 / bfloat16 embedding matrices,
 * _utils.py:74-77,94-102): the vectors are kept as 16-bit values (half the HBM footprint) and multiplied on the 16-bit
 * matrix cores with fp32 accumulation; the scores are the cosines (dot products) OF THE 16-BIT VECTORS, to fp32 accuracy.
 * `dtype` is PFZ_DENSE_F16 or PFZ_DENSE_BF16.  `source` says what `vec` holds: PFZ_DENSE_SRC_SAME = n x dim 16-bit values
 * of that type, copied as they are; PFZ_DENSE_SRC_F32 = n x dim float32 values, rounded to nearest even on the device.
 * The width is padded with zeros to a multiple of the 64-value k-chunk.  pfz_dense_topn takes two operands of one
 * type (PFZ_ERR_INVALID otherwise: it never converts); pfz_dense_dtype tells a handle's. */
#define PFZ_DENSE_F32 0
#define PFZ_DENSE_F16 1
#define PFZ_DENSE_BF16 2
#define PFZ_DENSE_SRC_SAME 0
#define PFZ_DENSE_SRC_F32 1
int pfz_dense_upload16(pfz_ctx *ctx, const void *vec, int64_t n, int64_t dim, int32_t normalize, int32_t dtype,
                       int32_t source, pfz_dense **out);
int pfz_dense_dtype(const pfz_dense *m, int32_t *dtype);

/* 8-bit integer operands for the same operator (reference _embeddings.py:127-133 on scalar-quantised int8 embedding
 * matrices, _utils.py:74-77,94-102): the vectors are kept as int8 values (a quarter of the fp32 footprint) and multiplied on
 * the integer matrix cores with int32 accumulation, which is exact; the scores are the cosines (dot products) OF THE INT8
 * VECTORS, to fp32 rounding of the final scaling.  `source` says what `vec` holds: PFZ_DENSE_SRC_SAME = n x dim int8 values
 * (signed), copied as they are; PFZ_DENSE_SRC_F32 = n x dim float32 values, quantised on the device, symmetric per row:
 * m = max |x| over the row, q = (int8) rintf((x / m) * 127.0f) (fp32 division and product, round to nearest even), row scale
 * m / 127.0f; a row of zeros gives zeros and scale 0.  Non-finite input is outside the contract.  The factor of a row in the
 * score is 1 / ||q|| with normalize != 0 (the cosine does not depend on the row scale); with normalize == 0 it is the row
 * scale (the dot products of the dequantised vectors), or 1 for int8 given as it is (integer dot products, exact in the
 * float result up to 2^24).  The width is padded with zeros to a multiple of the 128-value k-chunk; dim <= 131071, so that
 * a dot product (|.| <= 16384 dim) fits its int32 sum: PFZ_ERR_UNSUPPORTED beyond.  pfz_dense_dtype reports PFZ_DENSE_I8;
 * pfz_dense_topn takes two int8 operands (PFZ_ERR_INVALID for a mix with another type). */
#define PFZ_DENSE_I8 3
int pfz_dense_upload8(pfz_ctx *ctx, const void *vec, int64_t n, int64_t dim, int32_t normalize, int32_t source,
                      pfz_dense **out);

/* 1-bit operands for the same operator: binary embeddings (sentence-transformers' precision="ubinary", np.packbits(x > 0)),
 * 1/32 of the fp32 footprint.  A row is dim_bits bits in np.packbits order -- bit k of the row is bit 7 - k % 8 of byte k / 8 --
 * in (dim_bits + 7) / 8 bytes, the bits of the last byte beyond dim_bits zero (not checked).  `source` says what `vec` holds:
 * PFZ_DENSE_SRC_SAME = n such rows, copied as they are; PFZ_DENSE_SRC_F32 = n x dim_bits float32 values, packed on the device,
 * bit = x > 0 (NaN and +-0 give 0).  There is no matrix instruction for XOR / popcount: the tile program (k5_hamming_panel) runs
 * on the vector ALU and fills the same score panel and block maxima as the others, so the top-n, its deep passes and the
 * rescoring are shared.  With h = the number of differing bits of two rows, the score is that of the +-1 vectors the bits stand
 * for: normalize != 0 their cosine, float(dim_bits - 2 h) / float(dim_bits) as ONE correctly rounded fp32 division; normalize
 * == 0 their dot product float(dim_bits - 2 h).  Both are exact functions of h for dim_bits < 2^24: PFZ_ERR_UNSUPPORTED
 * beyond.  Scores take only dim_bits + 1 values, so ties are the normal case: the order (score descending, column ascending)
 * carries the result.  pfz_dense_dtype reports PFZ_DENSE_B1 and pfz_dense_shape dim_bits; pfz_dense_topn takes two such
 * operands of equal dim_bits and equal `normalize` (PFZ_ERR_INVALID otherwise, also for a mix with another type), and a result
 * of it is a candidate table for pfz_dense_rescore_topn like any other. */
#define PFZ_DENSE_B1 4
int pfz_dense_upload1(pfz_ctx *ctx, const void *vec, int64_t n, int64_t dim_bits, int32_t normalize, int32_t source,
                      pfz_dense **out);

/* Exact rescoring of a coarse top-n, the companion of the 16-bit, int8 and 1-bit operands (reference _embeddings.py:127-133 asks for
 * the cosines of the vectors as given; quantised embedding search keeps them by searching top_n x k candidates on the cheap
 * operands and scoring those few against the full-precision vectors).  `candidates` is a result buffer of at least
 * from_exact->n rows whose idx half holds, per from-row, column indices into `to_exact` -- a pfz_dense_topn result of the
 * 16-bit / int8 uploads of the same vectors; its val half is ignored.  An index outside [0, n_to), the -1 of an empty slot
 * among them, is skipped wherever it stands; real indices are distinct within a row (not checked).  For every candidate j of
 * row i: score = f_from[i] * f_to[j] * sum_k x_i[k] x_j[k] with the operands' own row factors (1 / ||row||, or 1 with
 * normalize == 0), summed in float64 in one fixed order per pair and rounded to fp32 once: equal to-rows get equal scores,
 * and the order of a row's candidates does not change its result.  `out` (at least from_exact->n rows of ntop columns, not
 * the candidate buffer itself) receives the candidates with score > max(lower_bound, 0) by (score descending, column
 * ascending), the first ntop of them, then (-1, 0).  1 <= ntop <= candidates per row.  Enqueues on the context stream.
 * PFZ_ERR_INVALID: an operand that is not PFZ_DENSE_F32, unequal widths, fewer candidate rows than from-rows, a result
 * buffer of another shape; PFZ_ERR_UNSUPPORTED: more than 1024 candidates per row. */
int pfz_dense_rescore_topn(pfz_ctx *ctx, const pfz_dense *from_exact, const pfz_dense *to_exact, const pfz_topn *candidates,
                           int32_t ntop, float lower_bound, pfz_topn *out);

/* Mixed rescoring: the float32 from-vectors against a to-side that is kept ONLY in its quantised form (reference
 * _embeddings.py:127-133 scores the vectors as given; sentence-transformers' quantised search keeps the corpus as int8 or packed
 * bits alone and rescores the float32 queries against that corpus itself, "binary search, int8 rescoring").  The contract is
 * pfz_dense_rescore_topn's -- candidate table, skipped indices, bound, order, (-1, 0) fill, one summation order per pair, so equal
 * to-rows get equal scores and the order of a row's candidates does not change its result -- except for `to_coarse`, a
 * PFZ_DENSE_I8 or PFZ_DENSE_B1 operand of the same width (typically the operand the candidates were searched on, or an int8
 * operand beside a 1-bit one); no float32 to-side exists.  For candidate j of row i, float64 sums rounded to fp32 once:
 *   int8: f_from[i] * f_to[j] * sum_k x_i[k] q_j[k] with the handle's own factor f_to -- 1 / ||q_j|| (normalize != 0: the cosine
 *         of the float vector and the int8 vector), the row's quantisation scale (normalize == 0, quantised from float32: the
 *         dot product with the dequantised row) or 1 (normalize == 0, int8 given as it is).
 *   bits: with s_j[k] = +1 / -1 for a set / clear bit, f_from[i] * sum_k x_i[k] s_j[k] / sqrt(dim_bits) (normalize != 0: the cosine
 *         of the float vector and the +-1 vector, the vectors the Hamming score speaks of), or the sum itself (normalize == 0).
 * The columns are the float32 top-n only as far as the quantised to-side ranks them so.  Enqueues on the context stream.
 * PFZ_ERR_INVALID: from-vectors that are not PFZ_DENSE_F32, to-vectors that are neither PFZ_DENSE_I8 nor PFZ_DENSE_B1, unequal
 * widths, a 1-bit to-side whose `normalize` differs from the from-side's, candidates == out, fewer candidate rows than
 * from-rows, ntop outside 1 .. candidates per row, a NaN bound, a result buffer of another shape; PFZ_ERR_UNSUPPORTED: more than
 * 1024 candidates per row.  No from-rows: PFZ_OK, nothing is done. */
int pfz_dense_rescore_topn_mixed(pfz_ctx *ctx, const pfz_dense *from_exact, const pfz_dense *to_coarse, const pfz_topn *candidates,
                                 int32_t ntop, float lower_bound, pfz_topn *out);

/* ---- K14: all pairs at or above a cosine, and their components ------------------
 * The threshold form of K5, what near-duplicate mining and semantic de-duplication ask of the cosine matrix of the reference's
 * Embeddings matcher (polyfuzz/models/_utils.py:74-77): every pair (from i, to j) whose cosine is >= min_similarity.  The score
 * of a pair is the float32 pfz_dense_topn computes for it, bit for bit -- dot product of the stored rows times 1 / ||a|| times
 * 1 / ||b|| -- and the comparison is (double)score >= min_similarity: equal is a hit.  fp32 operands uploaded with normalize = 1
 * (pfz_dense_upload) only: 16-bit, int8 and 1-bit handles, and handles uploaded without normalize, are PFZ_ERR_INVALID.
 * to == NULL, or the from-vectors' own handle: the self-join.  Only the tiles on or above the diagonal are computed; every
 * unordered pair i < j is reported once, as row i, to-index j, with the score of (i, j) (that of (j, i) may differ in the last bit
 * and is never computed); never (i, i); equal vectors at different positions are pairs.  A row of zeros scores 0 with everything.
 * Output, host buffers: CSR over the from-rows.  out_row_ptr int64[n_from + 1]; hit p of row i, out_row_ptr[i] <= p <
 * out_row_ptr[i + 1]: out_idx[p] the to-index (ascending within a row), out_sim[p] the score.  The same call gives the same bytes
 * every time.
 * capacity: the hits out_idx / out_sim have room for (they may be NULL when it is 0).  *out_total is always the exact number of
 * hits.  When it exceeds `capacity` the call still returns PFZ_OK, has written NONE of the three output arrays (the device never
 * writes a hit past the capacity either) and is to be repeated with capacity >= *out_total.
 * out_counters: NULL, or int64[2] of work counts -- [0] the 128 x 128 tiles executed (a self-join of T = ceil(n / 128) row tiles:
 * T (T + 1) / 2), [1] the 64 x 64 wave corners that contained a hit (the others left without touching memory).
 * No score panel is written: device memory beyond the operands is 12 bytes per hit of capacity plus the sort's copy.
 * An empty list on either side: PFZ_OK, *out_total = 0, out_row_ptr all zero.
 * Limits (PFZ_ERR_UNSUPPORTED beyond): at most 2^31 tiles in one call (two lists of 5.9 million rows each, a self-join of 8.3
 * million), fewer than 2^31 rows per list; a call of 2^24 workgroups or more (a self-join of 740 000 rows) is several launches.  A NaN min_similarity or one outside [0, 1], capacity < 0, unequal widths, another
 * operand type: PFZ_ERR_INVALID.  Profiling scopes: `k14_join` (the tile kernel), `k14_sort_unpack`.  Blocks. */
int pfz_dense_join(pfz_ctx *ctx, const pfz_dense *from_vectors, const pfz_dense *to_vectors, double min_similarity,
                   int64_t capacity, int64_t *out_row_ptr, int32_t *out_idx, float *out_sim, int64_t *out_total,
                   int64_t *out_counters);
/* The connected components of "cosine >= min_similarity" over ONE list: the pairs of pfz_dense_join(ctx, vectors, NULL,
 * min_similarity, ...), found by the same tiles, but none is stored -- the lane that finds a hit unites the two positions in the
 * lock-free union-find of csrc/k12_core.h.  Device memory beyond the operands is O(n) whatever the number of hits; there is no
 * capacity and no repeat.  out_label: host buffer int32[n], out_label[i] = the SMALLEST position in i's component (so
 * out_label[i] <= i); deterministic, whatever order the device's atomics took.  *out_pairs == pfz_dense_join's *out_total;
 * *out_components counts singletons too; out_counters as above.  vectors->n == 0: PFZ_OK, *out_pairs = *out_components = 0,
 * nothing else is written (out_label may be NULL).  Operands, limits and errors as pfz_dense_join, and a NULL out_pairs /
 * out_components is PFZ_ERR_INVALID.  Profiling scope: `k14_components` (forest, tile kernel and labels).  Blocks. */
int pfz_dense_components(pfz_ctx *ctx, const pfz_dense *vectors, double min_similarity, int32_t *out_label,
                         int64_t *out_pairs, int64_t *out_components, int64_t *out_counters);

/* ---- K22: K14's two entries searched on the 16-bit matrix cores, scored exactly --
 * The same question -- every pair (from i, to j) whose cosine is >= min_similarity -- answered in two stages: a search on float16
 * / bfloat16 copies of the vectors (K5's 16-bit tile program with K14's end) finds candidates, and every candidate is scored on
 * the fp32 vectors.  The score of a pair is the one pfz_dense_rescore_topn computes for it, bit for bit: f_from[i] * f_to[j] *
 * sum_k x_i[k] x_j[k], summed in float64 in one fixed order per pair and rounded to fp32 once; it is symmetric in its two rows, so
 * a self-join pair has one score.  The comparison is (double)score >= min_similarity: equal is a hit.
 * The search copy: pfz_dense_derive16 makes it on the device from an fp32 handle uploaded with normalize = 1 (PFZ_ERR_INVALID
 * otherwise) -- value k of a row is round16(x[k] * inv32), the fp32 product with the row's 1 / ||row|| rounded to nearest even to
 * `dtype` (PFZ_DENSE_F16 or PFZ_DENSE_BF16): every value lies in [-1, 1], which float16 needs; the copy has its own 1 / ||row||;
 * the matrix is uploaded once.  The handle is an ordinary 16-bit operand (pfz_dense_topn takes it; pfz_dense_free frees it).
 * The margin: a pair at or above min_similarity is a candidate because the search compares the 16-bit score with ts32 = the
 * largest float32 <= min_similarity - eps, where, with u = 2^-8 for bfloat16, u = 2^-11 for float16 and ld the copy's padded width
 * (a multiple of 64),
 *     eps = 2 asin(u + 2^-24 + sqrt(ld) 2^-25) + (ld + 8) 2^-23
 * (pfz_dense_search_margin, a pure host function: no device is touched).  The first term is derived: a rounding of relative size
 * u turns a vector by at most asin(u), the cosine is 1-Lipschitz in the angle, 2^-24 is the fp32 pre-scaling and sqrt(ld) 2^-25
 * float16's subnormals.  The second term rests on an assumption about the matrix core -- that an fp32 accumulation of exact 16-bit
 * products loses at most one ulp of the running sum per product (the two row factors and the final rounding add the rest); it is
 * held by measurement (tests/test_dense_join16_gpu.py), not proved.
 * The candidate buffer is the library's, not the caller's: cand_capacity keys of 8 bytes (0: the library chooses, four per
 * from-row and at least 4096).  When the search counts more candidates than the buffer holds, a buffer of the exact count is made
 * and the search runs once more: two runs at most.  Device memory beyond the operands is O(candidates), for the components too.
 * Output, order, self-join rule, *out_total and the capacity rule are K14's on the final hits: *out_total is always the exact
 * number of hits; when it exceeds `capacity` the call still returns PFZ_OK, has written NONE of the three output arrays and is
 * to be repeated with capacity >= *out_total; out_idx ascending within a row; never (i, i); the same call gives the same bytes
 * every time.  to16 == NULL, or from16 itself: the self-join (to32 NULL or from32 itself then).
 * out_counters: NULL, or int64[3] -- [0] the 256 x 256 tiles executed, [1] the 64 x 64 wave corners that held a candidate (both
 * add up over the two runs of a repeated search), [2] the candidates.
 * from32 == NULL (to32 NULL too): the plain 16-bit join, for a corpus that exists only in 16 bits -- margin 0, the search keeps its
 * scores and there is no second stage: the score of a pair is the float32 pfz_dense_topn computes on the 16-bit handles, bit for
 * bit (in a self-join that of (i, j), i < j), compared as K14 compares; cand_capacity is ignored and [2] is the number of hits.
 * PFZ_ERR_INVALID: a 16-bit handle that is not PFZ_DENSE_F16 / PFZ_DENSE_BF16 with normalize = 1, two 16-bit handles of different
 * types or widths, an exact handle that is not PFZ_DENSE_F32 with normalize = 1, unequal shapes between a 16-bit handle and its
 * exact handle, a self-join with a second exact handle or two lists without the to-side's, a NaN min_similarity or one outside [0, 1], capacity or
 * cand_capacity < 0.  Limits (PFZ_ERR_UNSUPPORTED beyond): at most 2^31 tiles in one call, fewer than 2^31 rows per list; a call
 * of 2^23 workgroups or more is several launches.  Profiling scopes: `k22_search`, `k22_rescore`, `k22_sort_unpack`.  Blocks. */
int pfz_dense_derive16(pfz_ctx *ctx, const pfz_dense *exact, int32_t dtype, pfz_dense **out);
int pfz_dense_search_margin(int32_t dtype, int64_t ld, double *out_eps);
int pfz_dense_join16(pfz_ctx *ctx, const pfz_dense *from16, const pfz_dense *to16, const pfz_dense *from32, const pfz_dense *to32,
                     double min_similarity, int64_t capacity, int64_t cand_capacity, int64_t *out_row_ptr, int32_t *out_idx,
                     float *out_sim, int64_t *out_total, int64_t *out_counters);
/* The connected components of "exact score >= min_similarity" over ONE list: the pairs of pfz_dense_join16(ctx, v16, NULL, v32,
 * NULL, min_similarity, ...), but no hit is stored -- the lane that scores one unites the two positions in the union-find of
 * csrc/k12_core.h.  Labels, *out_pairs and *out_components as pfz_dense_components; out_counters and cand_capacity as above.
 * Unlike K14's O(n), device memory beyond the operands is O(candidates): the candidate keys are stored.  Both handles are
 * required.  Profiling scopes: `k22_search`, `k22_rescore` (forest, scoring and labels).  Blocks. */
int pfz_dense_components16(pfz_ctx *ctx, const pfz_dense *v16, const pfz_dense *v32, double min_similarity, int64_t cand_capacity,
                           int32_t *out_label, int64_t *out_pairs, int64_t *out_components, int64_t *out_counters);

/* ---- K23: all pairs of binary codes within a Hamming distance, and their components --
 * The threshold form of the 1-bit operator: every pair (from i, to j) of PFZ_DENSE_B1 rows (pfz_dense_upload1) of equal dim_bits
 * that differ in h <= max_distance bits -- SimHash near-duplicates, perceptual hashes, de-duplication of a corpus kept as
 * "ubinary" embeddings.  The tiles are k5_hamming_panel's (128 x 128, XOR / popcount on the vector ALU); the comparison is made
 * on the integer counts in registers, so no score panel is written, nothing is divided and the result is exact.  The entries
 * threshold h itself and do not read the handles' `normalize`.
 * to_codes == NULL or == from_codes: the self-join -- only the tiles on or above the diagonal run, and the result holds every pair
 * i < j once (row i, column j), never (i, i); equal codes at different positions are pairs with h = 0.
 * Output, order, determinism, capacity, *out_total and the repeat protocol are pfz_dense_join's, with out_dist[p] = the pair's h in
 * place of a score; out_counters: NULL, or int64[2] -- [0] the 128 x 128 tiles executed, [1] the waves (32 rows x 128 columns) that
 * held a hit (the others left without touching memory).  An empty list on either side: PFZ_OK, *out_total = 0, out_row_ptr all
 * zero.  PFZ_ERR_INVALID: an operand of another type (the message names it), unequal widths, max_distance outside [0, dim_bits],
 * capacity < 0; PFZ_ERR_UNSUPPORTED: 2^31 rows or more in a list, more than 2^31 tiles in one call.  Profiling scopes: `k23_join`
 * (the tile kernel), `k23_sort_unpack`.  Blocks. */
int pfz_hamming_join(pfz_ctx *ctx, const pfz_dense *from_codes, const pfz_dense *to_codes, int64_t max_distance, int64_t capacity,
                     int64_t *out_row_ptr, int32_t *out_idx, int32_t *out_dist, int64_t *out_total, int64_t *out_counters);
/* The connected components of "h <= max_distance" over ONE list: the pairs of pfz_hamming_join(ctx, codes, NULL, max_distance,
 * ...), found by the same tiles and united in the union-find of csrc/k12_core.h; none is stored.  Labels, *out_pairs,
 * *out_components, the empty list and the NULL rules as pfz_dense_components; operands, limits and errors as pfz_hamming_join;
 * out_counters as above.  Profiling scope: `k23_components` (forest, tile kernel and labels).  Blocks. */
int pfz_hamming_components(pfz_ctx *ctx, const pfz_dense *codes, int64_t max_distance, int32_t *out_label, int64_t *out_pairs,
                           int64_t *out_components, int64_t *out_counters);
/* The distance that stands for a similarity: *out_max_distance = the largest h in [0, dim_bits] for which the score
 * pfz_dense_topn reports for normalised 1-bit operands, (double)(float(dim_bits - 2 h) / float(dim_bits)), is >= min_similarity
 * (compared as pfz_dense_join compares: float64, equal is kept); -1 if no h passes.  Found by evaluating that rule, not by a
 * closed form.  A pure host function: no device is touched.  PFZ_ERR_INVALID: dim_bits outside [1, 2^24), a NaN min_similarity
 * or one outside [0, 1]. */
int pfz_hamming_max_distance(int64_t dim_bits, double min_similarity, int64_t *out_max_distance);

/* ---- K24: the same two results through a block index, for small distances ---------
 * K23 computes every pair.  For a small max_distance on short codes (64-bit SimHash fingerprints at 3) nearly all of that work is
 * thrown away.  The block index is the exact filter (csrc/k24_core.h): cut the dim_bits bits into m = max_distance + 1 blocks,
 * block b = bits [b dim_bits / m, (b + 1) dim_bits / m) in np.packbits order; two codes within max_distance agree completely on at
 * least one block.  A block's KEY is its first min(width, 32) bits; a pair is a CANDIDATE in block b iff its two keys of block b
 * are equal (self-join: column > row only), and a candidate is reported iff its full distance is <= max_distance and no earlier
 * block has equal keys -- every pair exactly once, nothing approximate: the result is pfz_hamming_join's, bit for bit.
 * The to-rows' m n_to sort keys (block << 56 | key << 24 | position) are sorted once; every (from-row, block) probe finds its run
 * of partners by binary search; the runs are cut into work items of at most 64 partners (K17's deal) and a wave computes an
 * item's distances, XOR / popcount over 16-byte pieces, leaving a pair as soon as it passes max_distance.
 * A (dim_bits, max_distance) is INDEXABLE iff 1 <= m <= min(dim_bits, 256); a call also needs fewer than 2^24 rows in both lists,
 * m n_to < 2^31 and m n_from < 2^31, and fewer than 2^31 work items.
 * mode: PFZ_HAMMING_INDEX_BLOCKS -- the index runs, or the call returns PFZ_ERR_UNSUPPORTED and the message names the limit;
 * PFZ_HAMMING_INDEX_AUTO -- the index runs iff the call is indexable and checks * R <= all pairs (n_from n_to, or n (n - 1) / 2
 * for a self-join), R the measured constant pfz_hamming_index_plan reports; otherwise K23's tile program runs inside the same
 * call.  The decision falls behind the sort and the searches, where `checks` is known.
 * Everything else -- operands, the self-join, output, order, capacity, *out_total, the repeat protocol, the empty lists, the other
 * errors -- is pfz_hamming_join's.  out_counters: NULL, or int64[5] -- [0] the blocks m, [1] the narrowest block's width in bits,
 * [2] checks: the (pair, block) candidates, a function of the input alone, [3] the work items, [4] the route: 1 = the index, 0 =
 * the tiles ([0] and [1] are 0 where (dim_bits, max_distance) is not indexable, [2] and [3] where the searches did not run).
 * Profiling scopes: `k24_keys`, `k24_sort`, `k24_ranges` (searches and scan), `k24_probe`, `k24_sort_unpack`; on the tile route
 * K23's.  Blocks. */
#define PFZ_HAMMING_INDEX_BLOCKS 1
#define PFZ_HAMMING_INDEX_AUTO 2
int pfz_hamming_join_indexed(pfz_ctx *ctx, const pfz_dense *from_codes, const pfz_dense *to_codes, int64_t max_distance, int32_t mode,
                             int64_t capacity, int64_t *out_row_ptr, int32_t *out_idx, int32_t *out_dist, int64_t *out_total,
                             int64_t *out_counters);
/* pfz_hamming_components through the same index: the hits are united in the union-find of csrc/k12_core.h where they are found;
 * *out_pairs equals the join's total.  mode and out_counters as above; the rest as pfz_hamming_components.  Profiling scope of the
 * forest, the probe kernel and the labels: `k24_components`.  Blocks. */
int pfz_hamming_components_indexed(pfz_ctx *ctx, const pfz_dense *codes, int64_t max_distance, int32_t mode, int32_t *out_label,
                                   int64_t *out_pairs, int64_t *out_components, int64_t *out_counters);
/* The index of a width and a distance: out = int64[4] -- [0] the blocks m, [1] the narrowest and [2] the widest block in bits,
 * [3] R.  A pure host function: no device is touched.  PFZ_ERR_UNSUPPORTED: not indexable (the message says why: more blocks than
 * bits, more than 256 blocks); PFZ_ERR_INVALID: dim_bits outside [1, 2^24), max_distance outside [0, dim_bits], NULL. */
int pfz_hamming_index_plan(int64_t dim_bits, int64_t max_distance, int64_t *out);

/* ---- K25: SimHash fingerprints of a string list, as a 1-bit operand ---------------
 * The codes K23 / K24 join, made on the device from a resident list (csrc/k25_core.h is the rule).  Analyzer: TFIDF's -- `params` as
 * pfz_tfidf_fit takes them: with clean (1-byte code units only) lower-case, keep [a-z0-9 ], collapse runs of ' ', strip; every window
 * of n consecutive symbols for n in ngram_lo .. ngram_hi, every occurrence; with remove_space_ngrams the windows that hold a ' ' are
 * dropped.  A symbol is the code point as uint32.  Hash, all mod 2^64: G = 0x9E3779B97F4A7C15; mix(z): z ^= z >> 30, z *=
 * 0xBF58476D1CE4E5B9, z ^= z >> 27, z *= 0x94D049BB133111EB, z ^= z >> 31; g = mix(G), then g = mix(g ^ c) for the window's symbols in
 * order; word 0 of the window's hash is g, word q >= 1 is mix(g + q G).  Vote V[64 q + b] = the sum over the windows of +1 where bit b
 * (least significant = 0) of word q is set, else -1; fingerprint bit k = V[k] > 0 (a tie gives 0), in np.packbits order.  So the first
 * 64 bits of a wider fingerprint are the 64-bit fingerprint.  A string without a window has an all-zero fingerprint and NO ROW in the
 * handle: it is nobody's partner.
 * *out_codes: a fresh PFZ_DENSE_B1 handle (pfz_dense_free) of the strings with a window, in list order, `bits` wide, normalize = 1,
 * in pfz_dense_upload1's layout.  out_row: host [n], a string's row in the handle, -1 = no window.  out_windows: host [n] or NULL,
 * the windows of every string.  out_bytes: host [n][bits / 8] or NULL, every string's fingerprint.
 * n = 0, and a list in which no string has a window, give a handle of 0 rows.  PFZ_ERR_INVALID: a NULL argument, bits that are no
 * multiple of 64 in [64, 1024], ngram_lo / ngram_hi that do not satisfy 1 <= lo <= hi <= 8, clean on 4-byte code units;
 * PFZ_ERR_UNSUPPORTED: 2^31 strings or more.  No limit on a string's length.  Profiling scopes: `k25_fingerprint`, `k25_compact`.
 * Blocks. */
int pfz_simhash(pfz_ctx *ctx, const pfz_strings *strings, const pfz_tfidf_params *params, int32_t bits, pfz_dense **out_codes,
                int32_t *out_row, int32_t *out_windows, uint8_t *out_bytes);

/* ---- K15: all pairs at or above a sparse cosine, and their components -----------
 * The threshold form of K3, what de-duplication asks of the reference's TF-IDF matcher: every pair (from-row i, to-row j) whose
 * cosine is >= min_similarity, however many partners a row has -- no top_n to guess, no n x top_n table.  to_index is the
 * inverted index of the to-side (pfz_index_build), from_matrix the from-rows (CSR, the same vocabulary).
 * The hit rule: the score of a pair is the float32 pfz_cossim_topn reports for it, bit for bit -- (float)sum * 2^-k of K3's
 * fixed-point sum -- and the comparison is (double)score >= min_similarity: equal is a hit.  A pair that shares no n-gram
 * (sum 0) is never a hit, also at min_similarity = 0.  That score is at most c * 2^-30 * (norm bound) + 3e-7 below the exact
 * cosine of a pair with c shared n-grams, so at min_similarity = 1.0 equal strings are hits only where their truncated sum
 * still rounds to 1.0.  The device compares integers: the host finds the smallest passing sum by evaluating the rule.
 * self_join != 0: from_matrix must be the matrix to_index was built from (its serial is compared; PFZ_ERR_INVALID otherwise).
 * Every unordered pair i < j is reported once, as row i, to-index j -- K3's sums are symmetric bit for bit, row i walks the
 * to-blocks from its own on --; never (i, i); equal rows at different positions are pairs.  self_join == 0: every (i, j), also
 * where both lists hold the same strings.
 * Output, host buffers: CSR over the from-rows.  out_row_ptr int64[n_from + 1]; hit p of row i, out_row_ptr[i] <= p <
 * out_row_ptr[i + 1]: out_idx[p] the to-index (ascending within a row), out_sim[p] the score.  The same call gives the same bytes
 * every time.
 * capacity: the hits out_idx / out_sim have room for (they may be NULL when it is 0).  *out_total is always the exact number of
 * hits.  When it exceeds `capacity` the call still returns PFZ_OK, has written NONE of the three output arrays (the device never
 * writes a hit past the capacity either) and is to be repeated with capacity >= *out_total.
 * out_counters: NULL, or int64[3] of work counts -- [0] the (from-row, to-block) visits that had postings, [1] those of them an
 * exact upper bound of the block's sums skipped (rows of at most 64 n-grams only; longer rows go unpruned), [2] the sweep steps
 * (256 to-rows of one from-row) that contained a hit; the others touched no memory.
 * Device memory beyond the operands is 12 bytes per hit of capacity plus the sort's copy.
 * An empty list on either side, or a threshold no sum reaches: PFZ_OK, *out_total = 0, out_row_ptr all zero.
 * Limits: fewer than 2^31 rows per list (PFZ_ERR_UNSUPPORTED beyond), and the index's own limits (pfz_index_build).  A NaN
 * min_similarity or one outside [0, 1], capacity < 0, unequal n_cols: PFZ_ERR_INVALID.  Profiling scopes: `k15_join` (the row
 * walk), `k15_sort_unpack`.  Blocks. */
int pfz_cossim_join(pfz_ctx *ctx, const pfz_index *to_index, const pfz_csr *from_matrix, int32_t self_join,
                    double min_similarity, int64_t capacity, int64_t *out_row_ptr, int32_t *out_idx, float *out_sim,
                    int64_t *out_total, int64_t *out_counters);
/* The connected components of "cosine >= min_similarity" over ONE list: the pairs of pfz_cossim_join(ctx, index, matrix, 1,
 * min_similarity, ...), found by the same walk, but none is stored -- the lane that finds a hit unites the two positions in the
 * lock-free union-find of csrc/k12_core.h.  `matrix` must be the matrix `index` was built from (PFZ_ERR_INVALID otherwise).
 * Device memory beyond the operands is O(n) whatever the number of hits; there is no capacity and no repeat.  out_label: host
 * buffer int32[n], out_label[i] = the SMALLEST position in i's component (so out_label[i] <= i); deterministic, whatever order
 * the device's atomics took.  *out_pairs == pfz_cossim_join's *out_total; *out_components counts singletons too; out_counters as
 * above.  No rows: PFZ_OK, *out_pairs = *out_components = 0, nothing else is written (out_label may be NULL).  Limits and errors
 * as pfz_cossim_join, and a NULL out_pairs / out_components is PFZ_ERR_INVALID.  Profiling scope: `k15_components` (forest, row
 * walk and labels).  Blocks. */
int pfz_cossim_components(pfz_ctx *ctx, const pfz_index *index, const pfz_csr *matrix, double min_similarity,
                          int32_t *out_label, int64_t *out_pairs, int64_t *out_components, int64_t *out_counters);

/* ---- K6: reductions on the hot path's output --------------------------------
 * precision_recall_curve (reference polyfuzz/metrics.py:12-53): for every threshold p_k
 * (ascending, n_thresholds <= 4096) count_ge[k] = #{i : sim[i] >= p_k} and sum_ge[k] = the sum of
 * those similarities (recall = count / n, average precision = sum / count on the host).  NaN
 * similarities are never >= a threshold.  Sums are accumulated in 64-bit fixed point (bit-
 * reproducible): every value is rounded once to a multiple of 2^(e - 61), with frexp(n * max|sim|) =
 * (m, e), so a sum of c values is off by at most c * 2^(e - 62) plus its own rounding to a double
 * (absolute error of a mean below 1e-13 for similarities in [0, 100]).  Thresholds may repeat and be
 * negative, like the similarities.  PFZ_ERR_INVALID: no or more than 4096 thresholds, thresholds that
 * descend, an infinite similarity.  Blocks. */
int pfz_pr_curve_host(pfz_ctx *ctx, const double *sim, int64_t n, const double *thresholds,
                      int32_t n_thresholds, int64_t *count_ge, double *sum_ge);
/* single_linkage (reference polyfuzz/linkage.py:5-53) of a TOP-1 result of a list of unique strings
 * against itself: as PolyFuzz._create_groups builds it (polyfuzz.py:468-475: model.match(strings),
 * the diagonal excluded), or as a two-list match of the list with itself (model.match(strings,
 * strings), where a row's best match is usually the string itself).
 * row i = (From i, To = result idx[i][0], Similarity = round(score, 3)), rows with Similarity >
 * min_similarity (>= 0) walked in order with the reference's greedy, order-dependent rule -- cluster 0
 * is falsy, so the first cluster's members are re-assigned when met again.  A row without a match
 * (an index outside [0, n_rows), or a Similarity that rounds below 0.001) is not walked.  A kept row
 * with To == From does what the walk does: if the string is unmapped or in cluster 0 it
 * founds a cluster with itself, if it is mapped already the row is skipped.  out_cluster[i] = cluster
 * id of string i (-1: in no cluster); out_key[i] = position key of string i in the reference's dicts
 * (ascending key = insertion order; -1 where out_cluster is -1); out_info3 (may be NULL) = {first kept
 * row or -1, fixpoint rounds, clusters founded}.  `result` may hold more than one rank per row; only
 * rank 0 is read.  Blocks.
 * PFZ_ERR_INVALID: min_similarity < 0, 2^30 rows or more.  PFZ_ERR_UNSUPPORTED: one of the kernel's two
 * loops did not settle within its bound -- n_rows + 1 rounds of the activity fixpoint, ceil(log2
 * n_rows) + 2 rounds of pointer jumping; out_cluster and out_key are then left unwritten.  No input
 * reaches either bound (every top-1 graph on up to 7 rows is checked); the code is there so that
 * none can keep the device busy for ever. */
int pfz_linkage_top1(pfz_ctx *ctx, const pfz_topn *result, double min_similarity,
                     int32_t *out_cluster, int32_t *out_key, int32_t *out_info3);

/* ---- multi-GPU (one process per GPU: RCCL over xGMI; or one process, many contexts) ------
 * The from-side is row-sharded, the to-side replicated; the only exchange is
 * the all-gather of per-shard results.  Bootstrap: rank 0 calls
 * pfz_comm_unique_id, the 128-byte id is broadcast by the host launcher
 * (torch.distributed / MPI / a file), every rank calls pfz_comm_init. */
int pfz_comm_unique_id(uint8_t id128[128]);
int pfz_comm_init(pfz_ctx *ctx, const uint8_t id128[128], int32_t rank, int32_t world, pfz_comm **out);
/* NCCL_VERSION_CODE of the rccl.h this library was compiled against, and ncclGetVersion() of the librccl the process resolved (a
 * torch wheel brings its own; the reference has no collective library at all -- joblib only, _distance.py:77).  pfz_comm_init
 * refuses (PFZ_ERR_RCCL) when the majors differ; bench.py prints both in its line. */
int pfz_rccl_versions(int32_t *header, int32_t *runtime);
void pfz_comm_destroy(pfz_comm *c);
/* The same communicator interface inside ONE process: `world` contexts -- on different GPUs or on the
 * same one -- each driven by its own host thread.  A collective is a host rendezvous of the ranks plus
 * event waits and device-to-device copies on every rank's stream (no RCCL).  Every rank must make the
 * same sequence of collective calls, from different threads.  The group outlives its communicators. */
typedef struct pfz_comm_group pfz_comm_group;
int pfz_comm_group_create(int32_t world, pfz_comm_group **out);
void pfz_comm_group_destroy(pfz_comm_group *g);
int pfz_comm_init_local(pfz_ctx *ctx, pfz_comm_group *g, int32_t rank, pfz_comm **out);
/* all-gather equal-sized shards of top-n results: `local` holds rows
 * [rank*rows_per_rank, (rank+1)*rows_per_rank); `global` has world *
 * rows_per_rank rows.  Enqueues on the context stream. */
int pfz_comm_allgather_topn(pfz_comm *c, const pfz_topn *local, pfz_topn *global);
/* The other sharding (BASELINE north_star: "row-sharded from/to lists ... all-gather of per-shard top-n candidates"):
 * every rank indexes a SHARD OF THE TO-ROWS and matches all from-rows against it; `local` = its top-n per from-row
 * with to-indices local to the shard, to_offset = global index of the shard's first to-row.  All-gathers the ranks'
 * candidates and leaves in `out` (same shape as `local`), on every rank, the top-n by (score desc, global to-index asc).
 * Needed only when the to-side does not fit one GPU; world x ntop <= 1024.  Enqueues. */
int pfz_comm_merge_to_shards(pfz_comm *c, const pfz_topn *local, int64_t to_offset, pfz_topn *out);
int pfz_comm_barrier(pfz_comm *c);
/* The self-match of a list against itself (reference _tfidf.py:113-116 -> _utils.py:82-91) cut over the communicator's GPUs in
 * K3's symmetric form (every unordered pair of rows scored once over all GPUs; csrc/k3_symmetric.hip): every
 * rank holds the whole list's matrix A and its index; rank r works on the rows r, r + world, ...; the ranks' pass-0 thresholds
 * and their per-row candidate lists (n x ntop 64-bit keys per rank) are all-gathered; `out` (n_rows x ntop) holds the FULL result
 * on every rank, bit-identical to pfz_cossim_topn(..., exclude_diag = 1) on one GPU.  PFZ_ERR_UNSUPPORTED when
 * pfz_index_symmetric_ok says no (then: row shards + pfz_comm_allgather_topn). */
int pfz_comm_cossim_topn_symmetric(pfz_comm *c, const pfz_index *ix, const pfz_csr *A, int32_t ntop, float lower_bound,
                                   pfz_topn *out);
int pfz_index_symmetric_ok(const pfz_index *ix, const pfz_csr *A, int32_t ntop, int32_t n_parts, int32_t *yes);
/* The same question asked by ALL ranks together (a collective: every rank calls it, it waits): *yes = 1 only if every rank's own
 * pfz_index_symmetric_ok says yes AND every rank could allocate the session buffers of its index.  What a rank reads from its own
 * environment or gets from its own allocator must not send it into pfz_comm_cossim_topn_symmetric while a peer goes to
 * pfz_comm_allgather_topn: ask this once per job (sizes fixed), then every rank takes the same branch of reference
 * _tfidf.py:113-116 -> _utils.py:82-91's self-match.  A rank that fails INSIDE pfz_comm_cossim_topn_symmetric afterwards aborts
 * the communicator (its peers' collectives return PFZ_ERR_RCCL instead of waiting for it). */
int pfz_comm_symmetric_ok(pfz_comm *c, const pfz_index *ix, const pfz_csr *A, int32_t ntop, int32_t *yes);
int pfz_comm_info(const pfz_comm *c, int32_t *rank, int32_t *world);
/* pfz_tfidf_fit over a corpus that is split across the ranks of `comm`:
 * `replicated` (may be NULL) is identical on every rank and counted once --
 * the to-list -- and `local_shard` is this rank's part of the from-list.  The
 * vocabulary is the union over ranks (all-gather of the code bitmaps) and df /
 * n_docs are all-reduced, so every rank ends with the SAME fitted vectoriser
 * the single-GPU fit on the concatenated lists would produce. */
int pfz_tfidf_fit_sharded(pfz_ctx *ctx, pfz_comm *comm, const pfz_tfidf_params *params,
                          const pfz_strings *replicated, const pfz_strings *local_shard, pfz_tfidf **out);

#ifdef __cplusplus
}
#endif
#endif /* POLYFUZZ_HIP_H */
