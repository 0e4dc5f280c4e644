"""SimHash -- strings to binary fingerprints on the device (K25), then Hamming's three questions on them without a host round trip:
every pair within a bit distance (`join`: K23 / K24), the clusters of that relation (`components`) and the n best choices (`match`:
K5's Hamming top-n).

A fingerprint is the character-n-gram SimHash of the string under TFIDF's analyzer (clean_string, n_gram_range,
remove_space_ngrams): every window votes +1 / -1 on each of `bits` bits through a 64-bit mixing hash, a bit is set where the votes
are positive (csrc/k25_core.h is the rule, include/polyfuzz_hip.h spells it out).  Strings that share most of their n-grams get
fingerprints that differ in few bits, so "within max_distance bits" stands in for "TF-IDF cosine above a threshold" at list sizes
where neither K11's exact self-join nor K15's TF-IDF join is affordable; it is a sketch, and docs/SIMHASH_MEASURED.md has its recall.

A string without a window (shorter than the smallest n-gram once cleaned) has an all-zero fingerprint and is never a partner of
anything -- as in TFIDF.join, where a pair without a common n-gram is never a hit.
"""
import time
from typing import List

import numpy as np
import pandas as pd

from .. import _lib
from . import _hamming
from ._base import BaseMatcher
from ._tfidf import upload_strings
from ._utils import clip_top_n, topn_to_frame


class SimHash(BaseMatcher):
    """
    Join, cluster and match lists of strings by the Hamming distance of their SimHash fingerprints

    Arguments:
        bits: the fingerprint's width, a multiple of 64 in [64, 1024].  The first 64 bits of a wider fingerprint are the 64-bit one.
        n_gram_range: (lo, hi), 1 <= lo <= hi <= 8: the window lengths
        clean_string: TFIDF's cleaning -- lower-case, keep [a-z0-9 ], collapse spaces
        remove_space_ngrams: drop the windows that hold a ' '
        model_id: The name of the particular instance, used when comparing models

    fingerprints: the codes themselves, uint8 [n, bits / 8] in np.packbits order -- what Hamming takes as `embeddings`.
    join:         every pair within a distance, Hamming.join's frame and rules; rows are positions in the caller's lists.
    components:   int32 labels, the smallest position of each component; polyfuzz_amd.linkage.connected_components(strings,
                  SimHash(), 0.9) turns them into single_linkage's three dicts.
    match:        each from-string's top_n nearest to-strings, Hamming.match's frame.

    Thresholds as Hamming's: exactly one of `max_distance` (an int in [0, bits]) and `min_similarity` (a number in [0, 1], turned
    into the distance it stands for by _lib.hamming_max_distance).  The attribute `index` takes Hamming's values -- None (K23's
    tiles), "blocks" (K24's block index), "auto" (the library's measured rule) -- and defaults to "auto".

    last_timings holds "fingerprint" (pack, upload and K25, ms) beside "device" and "frame"; last_counts holds "windowless", the
    strings without a window, beside what Hamming reports.
    """

    def __init__(self,
                 bits: int = 64,
                 n_gram_range=(3, 3),
                 clean_string: bool = True,
                 remove_space_ngrams: bool = True,
                 model_id: str = None):
        super().__init__(model_id)
        self.type = "Embeddings"
        self.bits = _lib.check_simhash_bits(bits)
        self.n_gram_range = _lib.check_simhash_grams(n_gram_range)
        self.clean_string = clean_string
        self.remove_space_ngrams = remove_space_ngrams
        self.index = "auto"

    @property
    def index(self):
        return getattr(self, "_index", "auto")

    @index.setter
    def index(self, value):
        self._index = _hamming.check_index(value)

    # ---- K25 ----------------------------------------------------------------------------------------------------------------
    def _codes(self, strings, want_bytes=False):
        """-> what _lib.simhash returns for the list: (handle of the strings with a window, row, windows[, bytes])"""
        bits = _lib.check_simhash_bits(self.bits)
        lo, hi = _lib.check_simhash_grams(self.n_gram_range)
        dev = upload_strings(strings, self.clean_string)
        # (a list with code points > 0xFF was cleaned on the host: 4-byte units go through as they are)
        params = _lib.TfidfParams(lo, hi, int(bool(self.clean_string) and dev.char_width == 1), int(bool(self.remove_space_ngrams)))
        return _lib.simhash(_lib.Context.default(), dev, params, bits, want_bytes)

    def _threshold(self, min_similarity, max_distance):
        bits = _lib.check_simhash_bits(self.bits)
        _lib.check_simhash_grams(self.n_gram_range)
        hmax = _hamming.cutoff(bits, min_similarity, max_distance)
        _hamming.check_index_plan(_hamming.check_index(self.index), bits, hmax)
        return bits, hmax

    def fingerprints(self, strings: List[str]) -> np.ndarray:
        """ The fingerprints of `strings`: np.uint8 [n, bits / 8], np.packbits order, zeros where a string has no window. """
        t0 = time.perf_counter()
        _, row, _, out = self._codes(strings, want_bytes=True)
        self.last_timings = {"fingerprint": (time.perf_counter() - t0) * 1e3}
        self.last_counts = {"windowless": int((row < 0).sum())}
        return out

    def join(self,
             from_list: List[str],
             to_list: List[str] = None,
             min_similarity: float = None,
             *,
             max_distance: int = None) -> pd.DataFrame:
        """ Every pair of strings whose fingerprints differ in at most `max_distance` bits: Hamming.join's frame From, To,
        Similarity, Distance, one row per pair, ordered by from-position, then to-position.  to_list None: the self-join, every
        unordered pair of positions i < j once.  A string without a window has no row on either side.  Exact on the fingerprints.
        Sets last_timings and last_counts. """
        bits, hmax = self._threshold(min_similarity, max_distance)
        t0 = time.perf_counter()
        f_dev, f_row, _ = self._codes(from_list)
        t_dev, t_row = (None, f_row) if to_list is None else self._codes(to_list)[:2]
        t1 = time.perf_counter()
        if hmax < 0 or f_dev.n == 0 or (t_dev is not None and t_dev.n == 0):
            row_ptr, idx, dist, counts = _hamming.empty_join(f_dev.n)
        else:
            row_ptr, idx, dist, counts = _hamming.join_handles(_lib.Context.default(), f_dev, t_dev, hmax, self.index)
        t2 = time.perf_counter()
        # compact rows -> positions in the caller's lists (both increasing: the order of the pairs stays)
        f_pos, t_pos = np.flatnonzero(f_row >= 0).astype(np.int32), np.flatnonzero(t_row >= 0).astype(np.int32)
        frm = np.repeat(f_pos, np.diff(row_ptr))
        matches = _hamming.join_frame(from_list, from_list if to_list is None else to_list, frm, t_pos[idx], dist, bits)
        self.last_timings = {"fingerprint": (t1 - t0) * 1e3, "device": (t2 - t1) * 1e3, "frame": (time.perf_counter() - t2) * 1e3}
        self.last_counts = {**counts, "windowless": int((f_row < 0).sum()) + (0 if to_list is None else int((t_row < 0).sum()))}
        return matches

    def components(self,
                   strings: List[str],
                   min_similarity: float = None,
                   *,
                   max_distance: int = None) -> np.ndarray:
        """ Near-duplicate clusters of `strings`: int32 labels, label[i] = the smallest position in i's connected component of the
        graph whose edges are the pairs `join(strings, ...)` reports under the same threshold.  A string with no partner, and
        every string without a window, is its own component.  Sets last_timings and last_counts. """
        bits, hmax = self._threshold(min_similarity, max_distance)
        t0 = time.perf_counter()
        dev, row, _ = self._codes(strings)
        t1 = time.perf_counter()
        label = np.arange(len(strings), dtype=np.int32)
        pairs, components, work = 0, dev.n, {}
        if hmax >= 0 and dev.n > 0:
            compact, pairs, components, work = _hamming.components_handle(_lib.Context.default(), dev, hmax, self.index)
            pos = np.flatnonzero(row >= 0).astype(np.int32)
            label[pos] = pos[compact]                     # (pos is increasing: the smallest row is the smallest position)
        windowless = len(strings) - dev.n
        self.last_timings = {"fingerprint": (t1 - t0) * 1e3, "device": (time.perf_counter() - t1) * 1e3, "frame": 0.0}
        self.last_counts = {"pairs": pairs, "components": components + windowless, **work, "windowless": windowless}
        return label

    def match(self,
              from_list: List[str],
              to_list: List[str] = None,
              top_n: int = 1) -> pd.DataFrame:
        """ The top_n nearest to-strings of every from-string by fingerprint distance (K5's Hamming top-n on the two resident
        handles): Hamming.match's frame, Similarity = float32(bits - 2 h) / float32(bits) rounded to 3 decimals.  to_list None: the
        self-match, which leaves out the row itself.  A from-string without a window gets None / 0.0; a to-string without one is
        never chosen. """
        bits = _lib.check_simhash_bits(self.bits)
        t0 = time.perf_counter()
        f_dev, f_row, _ = self._codes(from_list)
        self_match = to_list is None
        t_dev, t_row = (f_dev, f_row) if self_match else self._codes(to_list)[:2]
        t1 = time.perf_counter()
        top_n = clip_top_n(top_n, to_list)
        width = max(top_n, 1)
        idx, val = np.full((len(from_list), width), -1, np.int32), np.zeros((len(from_list), width), np.float32)
        if f_dev.n > 0 and t_dev.n > 0:
            ctx = _lib.Context.default()
            c_idx, c_val = _lib.dense_topn(ctx, f_dev, t_dev, width, 0.0, exclude_diag=self_match).download()
            c_idx = np.asarray(c_idx).reshape(f_dev.n, width)
            t_pos = np.flatnonzero(t_row >= 0).astype(np.int32)
            f_pos = np.flatnonzero(f_row >= 0)
            idx[f_pos] = np.where(c_idx >= 0, t_pos[np.maximum(c_idx, 0)], -1)
            val[f_pos] = np.asarray(c_val).reshape(f_dev.n, width)
        t2 = time.perf_counter()
        frame = topn_to_frame(idx, val, from_list, from_list if self_match else to_list, top_n)
        self.last_timings = {"fingerprint": (t1 - t0) * 1e3, "device": (t2 - t1) * 1e3, "frame": (time.perf_counter() - t2) * 1e3}
        self.last_counts = {"windowless": int((f_row < 0).sum()) + (0 if self_match else int((t_row < 0).sum()))}
        return frame
