"""Hamming -- packed binary codes with all three questions answered on the device: the best or n best choices (`match`:
K5's Hamming tile program, through Embeddings with binary="ubinary"), every pair within a bit distance (`join`: K23) and the
clusters of that relation (`components`: K23).

"All pairs within Hamming distance k" is the query binary codes exist for: SimHash near-duplicate detection (64-bit
fingerprints, k = 3), perceptual image hashes (64 to 256 bits, k <= 10), de-duplication of a corpus that is kept only as
sentence-transformers "ubinary" embeddings.  `Embeddings.join` / `.components` keep refusing `binary`; the threshold forms live
here, as JaroWinkler's live beside an EditDistance that refuses them.

The score of two codes of d bits that differ in h is the cosine of the +-1 vectors the bits stand for,
float32(d - 2 h) / float32(d) -- what `Embeddings.match` reports for `binary` under a true cosine.  It is an exact function of the
integer h, so the device compares h itself and the result is exact by construction.
"""
import time
from typing import List

import numpy as np
import pandas as pd

from .. import _lib
from ._base import BaseMatcher
from ._embeddings import Embeddings
from ._utils import gather_column


class Hamming(BaseMatcher):
    """
    Match, join and cluster lists of strings by the Hamming distance of their binary codes

    Arguments:
        model_id: The name of the particular instance, used when comparing models

    The codes are always handed in (`embeddings_from`, `embeddings_to`, `embeddings`), as what DeviceDense.upload_bits takes:
    packed np.uint8 ("ubinary") or np.int8 ("binary") rows [n, B] of d = 8 B bits in np.packbits order, used as they are, or a
    float array [n, d], packed on the device with bit = x > 0.

    match:      each from-string's best (or top_n best) to-strings -- an internal Embeddings with binary = "ubinary", true cosine,
                that matcher's frame and code path.
    join:       every pair within a distance, exact (K23; K24 with `index`).
    components: the connected components of the self-join's graph (K23; K24 with `index`); polyfuzz_amd.linkage.connected_components(strings,
                Hamming(), 0.9, embeddings=codes) turns them into single_linkage's three dicts.

    A threshold is either `max_distance`, the largest number of differing bits (an int in [0, d]), or `min_similarity`, a number
    in [0, 1] that is turned into the distance it stands for: the largest h whose score, as float64, is >= min_similarity
    (_lib.hamming_max_distance; equal is kept).  Exactly one of the two is given.

    The attribute `index` chooses how `join` and `components` find their pairs; the results are the same, bit for bit.
        None      (the default) K23: every pair's distance is computed, tile by tile.
        "blocks"  K24's block index: the d bits are cut into max_distance + 1 blocks -- two codes within the distance agree
                  completely on at least one -- and only codes that share a block's bits are compared.  For small distances on
                  many codes (64-bit fingerprints at 3).  A (d, distance) without an index -- more than 256 blocks, or more
                  blocks than bits -- is a ValueError before any device call.
        "auto"    the index where the library's measured rule says it is cheaper (_lib.hamming_index_plan), K23's tiles otherwise.
    On the two indexed routes last_counts also holds _lib.HAMMING_INDEX_COUNTERS ("route": 1 = the index ran, 0 = the tiles).
    """
    INDEXES = (None, "blocks", "auto")

    def __init__(self, model_id: str = None):
        super().__init__(model_id)
        self.type = "Embeddings"
        self.index = None

    @property
    def index(self):
        return getattr(self, "_index", None)

    @index.setter
    def index(self, value):
        self._index = check_index(value)

    def _check_index(self, bits, hmax):
        """index == "blocks": a ValueError that names the limit when (bits, hmax) has no block index (no device is touched)"""
        check_index_plan(self.index, bits, hmax)

    def match(self,
              from_list: List[str],
              to_list: List[str] = None,
              embeddings_from: np.ndarray = None,
              embeddings_to: np.ndarray = None,
              top_n: int = 1) -> pd.DataFrame:
        """ The top_n best to-strings of every from-string: Embeddings(min_similarity=0.0, top_n=top_n, cosine_method="hip") with
        binary = "ubinary", its `match`, frame and code path (K5's Hamming top-n).  to_list None: the self-match. """
        best = Embeddings(min_similarity=0.0, top_n=top_n, cosine_method="hip", model_id=self.model_id)
        best.binary = "ubinary"
        return best.match(from_list, to_list, embeddings_from=embeddings_from, embeddings_to=embeddings_to)

    @staticmethod
    def _codes(strings, embeddings, side):
        if not isinstance(embeddings, np.ndarray):
            raise ValueError(f"Hamming compares binary codes that are handed in: {side} is required (packed uint8 / int8 rows, or a "
                             "float array whose signs are packed on the device)")
        if embeddings.ndim != 2 or embeddings.shape[0] != len(strings):
            raise ValueError(f"{side} has shape {embeddings.shape} for {len(strings)} strings")
        if embeddings.dtype in (np.uint8, np.int8):
            return embeddings, 8 * embeddings.shape[1]
        if embeddings.dtype.kind == "f":
            return embeddings, embeddings.shape[1]
        raise ValueError(f"binary vectors are packed uint8 / int8 rows or a float array, got {embeddings.dtype} for {side}")

    @staticmethod
    def _cutoff(bits, min_similarity, max_distance):
        """the one threshold of a call as a distance (-1: nothing passes); both or neither given, or one out of range: ValueError"""
        return cutoff(bits, min_similarity, max_distance)

    def join(self,
             from_list: List[str],
             to_list: List[str] = None,
             min_similarity: float = None,
             embeddings_from: np.ndarray = None,
             embeddings_to: np.ndarray = None,
             *,
             max_distance: int = None) -> pd.DataFrame:
        """ Every pair of codes that differ in at most `max_distance` bits (K23): the frame From, To, Similarity, Distance with
        one row per pair, ordered by from-index, then to-index.  A from-string without a partner has no row.  Distance is the
        number h of differing bits, Similarity the float64 of float32(d - 2 h) / float32(d), unrounded (_lib.hamming_similarity).
        Exact: every such pair is found, whatever their number, and no score matrix is written.

        to_list None: the self-join of from_list -- every unordered pair of positions i < j once, as From = from_list[i],
        To = from_list[j]; never a string with itself, but equal codes at different positions are a pair (h = 0).  Only the
        half of the distance matrix above the diagonal is computed.

        Exactly one of min_similarity (a number in [0, 1]) and max_distance (an int in [0, d]); embeddings_from is required, and
        embeddings_to with a to_list -- both of one width in bits (ValueError otherwise, before any device call).  The frame
        has the columns single_linkage reads; for the clusters of the self-join's graph see `components`, which never builds
        the frame.  Sets last_timings and last_counts = {"pairs": hits}. """
        if to_list is None and isinstance(embeddings_to, np.ndarray):
            raise ValueError("embeddings_to is given without a to_list: the self-join has one list and one matrix, embeddings_from")
        vec_from, bits = self._codes(from_list, embeddings_from, "embeddings_from")
        vec_to = None
        if to_list is not None:
            vec_to, bits_to = self._codes(to_list, embeddings_to, "embeddings_to")
            if bits_to != bits:
                raise ValueError(f"Hamming distance needs two code arrays of equal width, got {bits} and {bits_to} bits" + _lib.BITS_WIDTH_HINT)
        hmax = self._cutoff(bits, min_similarity, max_distance)
        self._check_index(bits, hmax)
        t0 = time.perf_counter()
        if hmax < 0:
            row_ptr, idx, dist, counts = empty_join(len(from_list))
        else:
            ctx = _lib.Context.default()
            f_dev = _lib.DeviceDense.upload_bits(ctx, vec_from)
            t_dev = None if vec_to is None else _lib.DeviceDense.upload_bits(ctx, vec_to)
            row_ptr, idx, dist, counts = join_handles(ctx, f_dev, t_dev, hmax, self.index)
        t1 = time.perf_counter()
        frm = np.repeat(np.arange(len(from_list), dtype=np.int32), np.diff(row_ptr))
        matches = join_frame(from_list, from_list if to_list is None else to_list, frm, idx, dist, bits)
        self.last_timings = {"device": (t1 - t0) * 1e3, "frame": (time.perf_counter() - t1) * 1e3}
        self.last_counts = counts
        return matches

    def components(self,
                   strings: List[str],
                   min_similarity: float = None,
                   embeddings: np.ndarray = None,
                   *,
                   max_distance: int = None) -> np.ndarray:
        """ Near-duplicate clusters of `strings` (K23): int32 labels, label[i] = the smallest position in i's connected component
        of the graph whose edges are the pairs `join(strings, ...)` reports under the same threshold -- "A ~ B and B ~ C put A, B
        and C together".  A string with no partner is its own component (label[i] == i).  Exact and deterministic.  The pairs
        are united on the device where they are found and never stored: device memory beyond the codes is O(len(strings))
        whatever their number.

        Threshold and `embeddings` as `join`.  Sets last_timings and last_counts = {"pairs": hits, "components": components}. """
        vec, bits = self._codes(strings, embeddings, "embeddings")
        hmax = self._cutoff(bits, min_similarity, max_distance)
        self._check_index(bits, hmax)
        t0 = time.perf_counter()
        if hmax < 0 or len(strings) == 0:
            label, pairs, components, work = np.arange(len(strings), dtype=np.int32), 0, len(strings), {}
        else:
            ctx = _lib.Context.default()
            label, pairs, components, work = components_handle(ctx, _lib.DeviceDense.upload_bits(ctx, vec), hmax, self.index)
        self.last_timings = {"device": (time.perf_counter() - t0) * 1e3, "frame": 0.0}
        self.last_counts = {"pairs": pairs, "components": components, **work}
        return label


# ---- what join and components do behind their uploads, on handles (SimHash runs the same on the handles K25 makes) -----------------

def empty_join(n_from):
    """the result of a join in which nothing passes: (row_ptr, idx, dist, counts)"""
    return np.zeros(n_from + 1, np.int64), np.empty(0, np.int32), np.empty(0, np.int32), {"pairs": 0}


def join_handles(ctx, f_dev, t_dev, hmax, index):
    """every pair of two bit handles (t_dev None: the self-join) within hmax >= 0 bits, by the route `index` names (Hamming.INDEXES)
    -> (row_ptr, idx, dist, counts) as _lib.hamming_join"""
    if index is None:
        return _lib.hamming_join(ctx, f_dev, t_dev, hmax)
    return _lib.hamming_join_indexed(ctx, f_dev, t_dev, hmax, auto=index == "auto", counters=True)


def components_handle(ctx, dev, hmax, index):
    """the components of one bit handle's self-join within hmax >= 0 bits -> (label, pairs, components, the indexed routes' counters)"""
    if index is None:
        return _lib.hamming_components(ctx, dev, hmax) + ({},)
    return _lib.hamming_components_indexed(ctx, dev, hmax, auto=index == "auto", counters=True)


def join_frame(from_list, names, frm, idx, dist, bits):
    """the frame From, To, Similarity, Distance of the pairs (from_list[frm[p]], names[idx[p]]) at dist[p] of `bits` bits"""
    sim = _lib.hamming_similarity(dist, max(bits, 1)).astype(np.float64)
    return pd.DataFrame({"From": gather_column(from_list, frm), "To": gather_column(names, idx), "Similarity": sim, "Distance": dist},
                        copy=False)


def check_index(value):
    if value is not None and not (isinstance(value, str) and value in Hamming.INDEXES):
        raise ValueError(f'index must be None, "blocks" or "auto", not {value!r}')
    return value


def check_index_plan(index, bits, hmax):
    """index == "blocks": a ValueError that names the limit when (bits, hmax) has no block index (no device is touched)"""
    if index == "blocks" and hmax >= 0:
        try:
            _lib.hamming_index_plan(bits, hmax)
        except _lib.PfzUnsupported as e:
            raise ValueError(f'index = "blocks": {e}; use index = "auto" or None') from None


def cutoff(bits, min_similarity, max_distance):
    """the one threshold of a call as a distance (-1: nothing passes); both or neither given, or one out of range: ValueError"""
    if (min_similarity is None) == (max_distance is None):
        raise ValueError("give exactly one of min_similarity and max_distance"
                         + (" (both are set)" if min_similarity is not None else " (neither is set)"))
    if max_distance is not None:
        if isinstance(max_distance, bool) or not isinstance(max_distance, (int, np.integer)) or not 0 <= int(max_distance) <= bits:
            raise ValueError(f"max_distance must be an int in [0, {bits}] (the codes' width in bits), not {max_distance!r}")
        return int(max_distance)
    t = _lib.check_min_similarity(min_similarity)
    if not 1 <= bits < 1 << 24:
        raise ValueError(f"the codes have {bits} bits: a similarity is defined for 1 to 2**24 - 1")
    return _lib.hamming_max_distance(bits, t)
