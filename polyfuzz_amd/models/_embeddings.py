"""Embeddings -- the reference's embedding matcher (polyfuzz/models/_embeddings.py:15-145) on the MI355X
engine, for the part of it that is on the hot path: cosine top-n over ready-made embedding matrices
(SURVEY.md §8 row A12).

The reference embeds the strings with Flair/word-embedding models that have to be downloaded; those
models are out of scope.  What is mirrored here is the matcher: `match(from_list, to_list,
embeddings_from=..., embeddings_to=..., re_train=...)` with the reference's argument meaning, the stored
`embeddings_to` for `re_train=False`, and the similarity operator on dense input.  An `embedding_method`
may be any callable `list[str] -> ndarray[n, d]` (the rows are L2-normalised like _embeddings.py:145);
without one, the embeddings must be passed in.
"""
import time
from typing import Callable, List, Optional

import numpy as np
import pandas as pd

from .. import _lib
from ._base import BaseMatcher
from ._utils import gather_column, topn_to_frame, clip_top_n, _METHODS


class Embeddings(BaseMatcher):
    """
    Match two lists of strings by the cosine similarity of their embeddings

    Arguments (reference _embeddings.py:60-65):
        embedding_method: callable mapping a list of strings to an ndarray of row vectors, or None when
                          the embeddings are always supplied to `match`
        min_similarity: The minimum similarity between strings, otherwise return 0 similarity
        top_n: The number of best matches you want returned
        cosine_method: "sparse" (raw dot product of the vectors as given, honours `min_similarity`),
                       "sklearn" / "knn" (true cosine, ignore `min_similarity`) -- the reference's
                       semantics, _utils.py:59-102 -- or "hip" (true cosine, honours `min_similarity`)
        model_id: The name of the particular instance, used when comparing models

    Attribute (ours; the constructor keeps the reference's signature, tests/test_reference_interface_cpu.py):
        compute_dtype: None / "float32" (default): fp32 operands.  "float16" / "bfloat16": the embeddings are kept as
                       16-bit values on the device (a np.float16 array, or raw bfloat16 bits as np.uint16, is taken as it
                       is; float32 / float64 embeddings are rounded to nearest even) and multiplied on the 16-bit matrix
                       cores with fp32 accumulation.  The similarity is then that of the 16-bit vectors: rounding float32
                       vectors changes the scores by about 1e-3 (float16) or 1e-2 (bfloat16) relative per element, which
                       is why this is opt-in: `m = Embeddings(...); m.compute_dtype = "float16"`.  Anything else raises
                       ValueError; it is kept through pickling, and the resident to-side is re-uploaded when it changes.
        precision: None (default) or "int8", the keyword of sentence-transformers' quantised embeddings:
                   `m = Embeddings(...); m.precision = "int8"`.  The embeddings are kept as signed 8-bit values on the device
                   (a quarter of the fp32 footprint) and multiplied on the integer matrix cores with exact int32 sums.  An
                   np.int8 array is taken as it is; float arrays -- also what an `embedding_method` returns -- are quantised
                   per row, q = rint(x / max|x| * 127).  The score is the cosine (with cosine_method "sparse" the dot
                   product: of the integers as given, or of the dequantised rows) OF THE INT8 VECTORS, exact to fp32
                   rounding.  What quantising float32 embeddings costs: on 300 x 2 000 unit-Gaussian vectors of width 768
                   the worst |cosine_int8 - cosine_fp32| is 2.1e-3 and the top-1 stays in 293 of 300 rows
                   (tests/test_dense8_gpu.py prints the figures), which is why this is opt-in.  Signed values only (np.uint8 raises), width <= 131071.
                   Anything else raises ValueError; with a `compute_dtype` other than None / "float32" `match` raises
                   ValueError.  Kept through pickling; the resident to-side is re-uploaded when it changes.
        rescore_multiplier: None (default: `match` is exactly as above) or an int >= 1, for the 16-bit and int8 operand types:
                   `m.precision = "int8"; m.rescore_multiplier = 4`.  The search on the cheap operands then keeps
                   top_n x rescore_multiplier candidates per row (clipped to the to-strings there are; at most 1024), and
                   those few are scored against the float32 vectors, which are kept on the device beside the cheap ones
                   (k5_rescore_topn: float64 sums, rounded once).  What is exact: every Similarity is the fp32 path's score
                   of the ORIGINAL vectors (1e-5), `min_similarity` cuts on that score, and the order is that of those
                   scores.  What is not: the set of columns is the fp32 top-n only where that lies within the coarse
                   candidates.  Measured on 300 x 2 000 unit-Gaussian vectors of width 768, top-5
                   (tests/test_dense_rescore_gpu.py prints the figures): plain int8 returns other columns than the float64 oracle in 75 of 300 rows and plain bfloat16 in 15; of the 1 500 exact top-5 entries the int8 candidates
                   miss 26 at a multiplier of 1 and none at 2 or 4 (bfloat16: 2 and none), and with rescore_multiplier = 4 both types agree
                   with the oracle in all 300 rows.  A guarantee it is not: data whose coarse ranking is off by more than
                   the multiplier's margin loses those columns.
                   `match` raises ValueError when it is set and the operands are float32 (nothing to rescore), or when
                   the embeddings handed in are np.int8 / np.float16 / raw bfloat16 (np.uint16) arrays: there are no
                   full-precision vectors to rescore against.  Kept through pickling; changing it alone re-uploads nothing.
        binary: None (default: `match` is exactly as above) or "binary" / "ubinary", sentence-transformers' names for packed
                   sign bits, np.packbits(x > 0): `m = Embeddings(...); m.binary = "ubinary"`.  Both names select the same
                   device path; what is handed in decides how it is read: an np.uint8 array [n, B] is "ubinary" rows of
                   d = 8 B bits, an np.int8 array is "binary" (ubinary - 128, brought to the same bytes), and float arrays
                   -- also what an `embedding_method` returns -- are packed on the device, bit = x > 0, d = their width.  The
                   device keeps 1/32 of the fp32 footprint.  The Similarity of two rows with h differing bits is the cosine of
                   the +-1 vectors the bits stand for, float32(d - 2 h) / float32(d) (cosine_method "sparse": their dot
                   product d - 2 h), exact and full of ties, which the column order resolves.  Both sides need the same d: a
                   float side whose width is not a multiple of 8 cannot be paired with packed rows.  `rescore_multiplier`
                   works with it as with the other cheap operands -- the usual way to use such embeddings -- and raises
                   for packed uint8 / int8 arrays (no full-precision vectors).  `match` raises ValueError when it is set
                   together with `precision` or a `compute_dtype` other than None / "float32".  Anything else raises
                   ValueError; kept through pickling; the resident to-side is re-uploaded when it changes.
        rescore_to: None (default: `rescore_multiplier` scores against the float32 vectors of both sides, as above) or "int8" /
                   "binary" / "ubinary": `m.binary = "ubinary"; m.rescore_multiplier = 16; m.rescore_to = "int8"`.  The
                   candidates are then scored with the float32 FROM-vectors against the TO-side in that form (k5_mixed_rescore:
                   float64 sums, rounded once), the way sentence-transformers rescores a quantised corpus: the to-side never
                   exists as float32 on the device -- at 500 000 x 768, 48 MB of bits (+ 0.38 GB with "int8") instead of
                   1.54 GB beside them.  The pairs are precision="int8" with "int8", `binary` with "binary" / "ubinary", and
                   `binary` with "int8" ("binary search, int8 rescoring"); anything else, a 16-bit `compute_dtype`, or no
                   `rescore_multiplier` makes `match` raise ValueError.  The Similarity is the cosine (cosine_method "sparse":
                   the dot product) of the float from-vector and the int8 to-vector -- dequantised, for float to-vectors
                   quantised here -- or of the float from-vector and the +-1 vector the bits stand for, to 1e-5;
                   `min_similarity` cuts on it.  The columns are the fp32 top-n only as far as the quantised to-side ranks
                   them so.  `embeddings_from` must be float (np.int8 / packed arrays raise "no full-precision vectors");
                   `embeddings_to` may be float, or for equal forms the np.int8 array or the packed np.uint8 / np.int8 array
                   itself -- a corpus that exists only in quantised form.  Validated when set, kept through pickling; the
                   to-side of the rescoring is resident like the coarse one and re-made when `rescore_to` or the to-side
                   changes.

        search_dtype: None (default: `join` and `components` run K14, the fp32 tile kernel) or "bfloat16" / "float16":
                   `m = Embeddings(...); m.search_dtype = "bfloat16"`.  `join` and `components` then upload the fp32 vectors once,
                   derive a 16-bit search copy on the device (every row scaled to unit length, then rounded to nearest even),
                   find candidates on the 16-bit matrix cores and score every candidate on the fp32 vectors (K22).  A threshold
                   makes that exact, which a top-n is not: rounding moves a cosine by at most a known margin (0.0079 for
                   bfloat16, 0.0011 for float16 at width 768; _lib.dense_search_margin), the search runs that far below
                   min_similarity, and the exact score decides -- every pair at or above the threshold is found, and there is no
                   multiplier to choose.  Similarity is the exact score of `rescore_multiplier`'s second stage: a float64 sum
                   rounded to float32 once, symmetric in the two rows; it may differ from K14's fp32-summed score in the last
                   bits, so a pair within float32 rounding of the threshold can fall on the other side.  `match` raises ValueError
                   while it is set.  Anything else raises ValueError when assigned; kept through pickling.

    Beside `match` (each string's best): `join` -- every pair whose cosine is at least a threshold -- and `components` -- the
    near-duplicate clusters of one list -- on fp32 vectors (K14), or searched in 16 bits and scored in fp32 (K22, `search_dtype`);
    see the two methods.
    """
    def __init__(self,
                 embedding_method: Optional[Callable[[List[str]], np.ndarray]] = None,
                 min_similarity: float = 0.75,
                 top_n: int = 1,
                 cosine_method: str = "sparse",
                 model_id: str = None):
        super().__init__(model_id)
        self.type = "Embeddings"
        if embedding_method is not None and not callable(embedding_method):
            raise TypeError("polyfuzz_amd.Embeddings: embedding_method must be a callable list[str] -> ndarray "
                            "(Flair embedding objects are not supported: their models need downloads)")
        self.embedding_method = embedding_method
        self.min_similarity = min_similarity
        self.top_n = top_n
        self.cosine_method = cosine_method
        self.embeddings_to = None
        self._dev_to = None            # _lib.DeviceDense of the to-side
        self._dev_to_normalize = None
        self._compute_dtype = None
        self._dev_to_dtype = None      # operand type the resident to-side was uploaded with
        self._precision = None
        self._rescore_multiplier = None
        self._dev_to_exact = None      # float32 DeviceDense of the to-side, beside _dev_to, while rescoring is on
        self._binary = None
        self._rescore_to = None
        self._dev_to_exact_form = None  # what _dev_to_exact holds: "float32", or the checked rescore_to it was made for
        self._search_dtype = None

    @property
    def compute_dtype(self) -> Optional[str]:
        return self._compute_dtype

    @compute_dtype.setter
    def compute_dtype(self, value: Optional[str]):
        _lib.check_compute_dtype(value)
        self._compute_dtype = value

    @property
    def precision(self) -> Optional[str]:
        return self._precision

    @precision.setter
    def precision(self, value: Optional[str]):
        self._precision = _lib.check_precision(value)

    @property
    def rescore_multiplier(self) -> Optional[int]:
        return self._rescore_multiplier

    @rescore_multiplier.setter
    def rescore_multiplier(self, value: Optional[int]):
        self._rescore_multiplier = _lib.check_rescore_multiplier(value)

    @property
    def binary(self) -> Optional[str]:
        return self._binary

    @binary.setter
    def binary(self, value: Optional[str]):
        self._binary = _lib.check_binary(value)

    @property
    def rescore_to(self) -> Optional[str]:
        return self._rescore_to

    @rescore_to.setter
    def rescore_to(self, value: Optional[str]):
        _lib.check_rescore_to(value)
        self._rescore_to = value

    @property
    def search_dtype(self) -> Optional[str]:
        return self._search_dtype

    @search_dtype.setter
    def search_dtype(self, value: Optional[str]):
        if value is not None and value not in ("bfloat16", "float16"):
            raise ValueError(f"search_dtype must be None, 'bfloat16' or 'float16', got {value!r}")
        self._search_dtype = value

    def match(self,
              from_list: List[str],
              to_list: List[str] = None,
              embeddings_from: np.ndarray = None,
              embeddings_to: np.ndarray = None,
              re_train: bool = True) -> pd.DataFrame:
        """ Matches the two lists of strings to each other and returns the best mapping
        (reference _embeddings.py:87-135) """
        if self.search_dtype is not None:
            raise ValueError(f"search_dtype={self.search_dtype!r} is the 16-bit search of join and components, where a threshold "
                             "makes it exact; match's own two-stage route is compute_dtype + rescore_multiplier (leave "
                             "search_dtype at None)")
        if not isinstance(embeddings_from, np.ndarray):
            embeddings_from = self._embed(from_list)
        explicit_to = isinstance(embeddings_to, np.ndarray)     # the caller's own to-side always wins (_embeddings.py:117-133)
        if not explicit_to:
            if not re_train:
                embeddings_to = self.embeddings_to
                if embeddings_to is None:
                    raise ValueError("This Embeddings instance holds no to-side embeddings yet: "
                                     "call match(..., re_train=True) first")
            elif to_list is None:
                embeddings_to = self._embed(from_list) if self.embedding_method is not None else embeddings_from
            else:
                embeddings_to = self._embed(to_list)
        if self.cosine_method not in _METHODS:
            raise ValueError(f"cosine_method must be one of {_METHODS}")
        bits = _lib.check_binary(self.binary) is not None
        if bits:
            if self.precision is not None or _lib.check_compute_dtype(self.compute_dtype) != "float32":
                raise ValueError(f"binary={self.binary!r} is set together with precision={self.precision!r} / "
                                 f"compute_dtype={self.compute_dtype!r}: they name two operand types, leave those at None")
            dtype = _lib.BINARY

            def upload(ctx, vec, operand, normalize):
                return _lib.DeviceDense.upload_bits(ctx, vec, normalize) if operand == _lib.BINARY \
                    else _lib.DeviceDense.upload_as(ctx, vec, operand, normalize)
        else:
            dtype = _lib.operand_type(self.compute_dtype, self.precision)
            upload = _lib.DeviceDense.upload_as
        multiplier = _lib.check_rescore_multiplier(self.rescore_multiplier)
        rescore_to = _lib.check_rescore_to(self.rescore_to)
        if rescore_to is not None:
            if multiplier is None:
                raise ValueError(f"rescore_to={self.rescore_to!r} is set without a rescore_multiplier: there are no candidates "
                                 "to rescore (set rescore_multiplier to an int >= 1, or leave rescore_to at None)")
            if dtype in ("float16", "bfloat16"):
                raise ValueError(f"rescore_to={self.rescore_to!r} is set together with compute_dtype={self.compute_dtype!r}: "
                                 'the to-side is rescored in its int8 or binary form (set precision="int8" or binary)')
            if dtype != "float32":
                _lib.check_mixed_pair(dtype, rescore_to)
        if multiplier is not None:
            if dtype == "float32":
                raise ValueError("rescore_multiplier is set but the operands are float32: there is nothing to rescore "
                                 '(set precision="int8" or a 16-bit compute_dtype, or leave rescore_multiplier at None)')
            sides = (("embeddings_from", embeddings_from), ("embeddings_to", embeddings_to))
            if rescore_to is not None:
                to = np.asarray(embeddings_to)
                if to.dtype == np.int8 or (bits and to.dtype == np.uint8):      # the to-side as the search itself reads it
                    if dtype != rescore_to:
                        raise ValueError(f"embeddings_to is already a {to.dtype} array, the {dtype} search's own form: "
                                         f"rescore_to={self.rescore_to!r} can only name the same form then (pass float "
                                         "embeddings to have both forms made here)")
                    sides = sides[:1]
            for side, vec in sides:
                if np.asarray(vec).dtype in (np.int8, np.float16, np.uint16) + ((np.uint8,) if bits else ()):
                    raise ValueError(f"rescore_multiplier is set but {side} is already a {np.asarray(vec).dtype} array: "
                                     "there are no full-precision vectors to rescore against (pass float32 embeddings)")
        ctx = _lib.Context.default()
        normalize = self.cosine_method != "sparse"        # "sparse": raw dot products (reference _utils.py:74-82)
        lower = float(self.min_similarity) if self.cosine_method in ("sparse", "hip") else 0.0
        # the to-side stays in HBM: match(..., re_train=False) (PolyFuzz.transform, polyfuzz.py:234-240) uploads
        # the new from-vectors only; an explicitly passed to-side is uploaded unless it IS the resident one
        stale = explicit_to and embeddings_to is not self.embeddings_to
        if re_train or stale or self._dev_to is None or self._dev_to_normalize != normalize or self._dev_to_dtype != dtype:
            self._dev_to = upload(ctx, embeddings_to, dtype, normalize)
            self._dev_to_normalize = normalize
            self._dev_to_dtype = dtype
            self._dev_to_exact = None
        exact_form = "float32" if rescore_to is None else rescore_to
        if multiplier is not None and (self._dev_to_exact is None or self._dev_to_exact_form != exact_form):
            # (follows every re-upload of the coarse to-side.)  With rescore_to no float32 to-side is made: the coarse handle
            # itself, or the int8 form beside the bits
            self._dev_to_exact = self._dev_to if exact_form == dtype else upload(ctx, embeddings_to, exact_form, normalize)
            self._dev_to_exact_form = exact_form
        self_match = to_list is None
        same = self_match and embeddings_to is embeddings_from
        from_dev = self._dev_to if same else upload(ctx, embeddings_from, dtype, normalize)
        if from_dev.dim != self._dev_to.dim:
            raise ValueError(f"dense cosine needs two 2-D arrays with equal width, got {from_dev.dim} and {self._dev_to.dim}"
                             + (_lib.BITS_WIDTH_HINT if bits else ""))
        top_n = clip_top_n(self.top_n, to_list)
        if multiplier is not None:
            from_exact = self._dev_to_exact if same and rescore_to is None else upload(ctx, embeddings_from, "float32", normalize)
            idx, val = _lib.dense_topn_rescored(ctx, from_dev, self._dev_to, from_exact, self._dev_to_exact, max(top_n, 1), lower,
                                                multiplier, exclude_diag=self_match).download()
        else:
            idx, val = _lib.dense_topn(ctx, from_dev, self._dev_to, max(top_n, 1), lower, exclude_diag=self_match).download()
        self.embeddings_to = embeddings_to
        return topn_to_frame(idx, val, from_list, from_list if self_match else to_list, top_n)

    def _threshold_operands_only(self, what, min_similarity):
        """join and components run K14: fp32 operands, the true cosine.  Everything that names another operand type or a
        second pass is refused here, before any device call."""
        if (isinstance(min_similarity, bool) or not isinstance(min_similarity, (int, float, np.integer, np.floating))
                or not 0.0 <= float(min_similarity) <= 1.0):      # (NaN compares false)
            raise ValueError(f"min_similarity must be a number in [0, 1], not {min_similarity!r}")
        for name, value in (("precision", self.precision), ("binary", self.binary), ("rescore_multiplier", self.rescore_multiplier),
                            ("rescore_to", self.rescore_to)):
            if value is not None:
                raise ValueError(f"Embeddings.{what} compares the fp32 cosine with the threshold on the GPU; {name}={value!r} is "
                                 f"set, which has no threshold kernel (leave {name} at None)")
        if _lib.check_compute_dtype(self.compute_dtype) != "float32":
            raise ValueError(f"Embeddings.{what} compares the fp32 cosine with the threshold on the GPU; "
                             f"compute_dtype={self.compute_dtype!r} is set, which has no threshold kernel (leave compute_dtype at None)")

    def _vectors(self, strings, embeddings, side):
        vec = embeddings if isinstance(embeddings, np.ndarray) else self._embed(strings)
        if vec.ndim != 2 or vec.shape[0] != len(strings):
            raise ValueError(f"{side} has shape {vec.shape} for {len(strings)} strings")
        return vec

    def join(self,
             from_list: List[str],
             to_list: List[str] = None,
             min_similarity: float = 0.8,
             embeddings_from: np.ndarray = None,
             embeddings_to: np.ndarray = None) -> pd.DataFrame:
        """ Every pair whose cosine is at least `min_similarity` (K14): the frame From, To, Similarity with one row per pair,
        ordered by from-index, then to-index.  A from-string without a partner has no row.  Similarity is the float32 cosine
        `match` computes for the pair (cosine_method "hip"), and a pair is kept iff that value, as float64, is >=
        min_similarity: equal is kept.  Exact in that sense: every such pair is found, whatever their number -- there is no top_n
        to guess, and no score matrix is written.

        Always the true cosine, whatever `cosine_method` says: a threshold in [0, 1] means a cosine.  `min_similarity` of the
        constructor and `top_n` play no part.

        to_list None: the self-join of from_list -- every unordered pair of positions i < j once, as From = from_list[i],
        To = from_list[j]; never a string with itself, but equal vectors at different positions are a pair.  Only the half of
        the similarity matrix above the diagonal is computed.

        embeddings_from / embeddings_to: ready-made row vectors (any float dtype; computed in float32), else the
        embedding_method embeds the lists.  min_similarity: a number in [0, 1] (ValueError otherwise).  `precision`, `binary`,
        a 16-bit `compute_dtype`, `rescore_multiplier` and `rescore_to` must be unset (ValueError): the threshold kernels take
        fp32 operands only.  The frame has the columns single_linkage reads; for the clusters of the self-join's graph see
        `components`, which never builds the frame.  Sets last_timings and last_counts = {"pairs": hits}.

        With `search_dtype` set the pairs are found by K22 instead -- a 16-bit search below the threshold by the rounding margin,
        every candidate scored exactly on the fp32 vectors: the same frame, order and self-join rule; Similarity is the float64-summed
        score, and last_counts has "candidates" (what the search handed to the scoring) beside "pairs". """
        self._threshold_operands_only("join", min_similarity)
        if to_list is None and isinstance(embeddings_to, np.ndarray):
            raise ValueError("embeddings_to is given without a to_list: the self-join has one list and one matrix, embeddings_from")
        vec_from = self._vectors(from_list, embeddings_from, "embeddings_from")
        vec_to = None if to_list is None else self._vectors(to_list, embeddings_to, "embeddings_to")
        if vec_to is not None and vec_to.shape[1] != vec_from.shape[1]:
            raise ValueError(f"dense cosine needs two 2-D arrays with equal width, got {vec_from.shape[1]} and {vec_to.shape[1]}")
        t0 = time.perf_counter()
        ctx = _lib.Context.default()
        f_dev = _lib.DeviceDense.upload(ctx, vec_from, True)
        t_dev = None if vec_to is None else _lib.DeviceDense.upload(ctx, vec_to, True)
        if self.search_dtype is None:
            row_ptr, idx, sim, counts = _lib.dense_join(ctx, f_dev, t_dev, float(min_similarity))
        else:
            row_ptr, idx, sim, counts = _lib.dense_join16(ctx, f_dev.derive16(self.search_dtype),
                                                          None if t_dev is None else t_dev.derive16(self.search_dtype), f_dev, t_dev,
                                                          float(min_similarity))
        t1 = time.perf_counter()
        names = from_list if to_list is None else to_list
        frm = np.repeat(np.arange(len(from_list), dtype=np.int32), np.diff(row_ptr))
        matches = pd.DataFrame({"From": gather_column(from_list, frm), "To": gather_column(names, idx), "Similarity": sim}, copy=False)
        self.last_timings = {"device": (t1 - t0) * 1e3, "frame": (time.perf_counter() - t1) * 1e3}
        self.last_counts = counts
        return matches

    def components(self,
                   strings: List[str],
                   min_similarity: float = 0.8,
                   embeddings: np.ndarray = None) -> np.ndarray:
        """ Near-duplicate clusters of `strings` (K14): int32 labels, label[i] = the smallest position in i's connected component
        of the graph whose edges are the pairs `join(strings, min_similarity=...)` reports -- "A ~ B and B ~ C put A, B and C
        together".  A string with no partner is its own component (label[i] == i).  Exact and deterministic.  The pairs are
        united on the device where they are found and never stored or downloaded: device memory beyond the vectors is
        O(len(strings)) whatever their number.  polyfuzz_amd.linkage.connected_components turns the labels into the three dicts
        single_linkage returns.

        embeddings: ready-made row vectors, else the embedding_method embeds the list.  Refusals as `join`.  Sets last_timings
        and last_counts = {"pairs": hits, "components": components}.

        With `search_dtype` set (K22) the candidates of the 16-bit search are stored before they are scored: device memory beyond
        the vectors is O(candidates) then, and last_counts has "candidates" too. """
        self._threshold_operands_only("components", min_similarity)
        vec = self._vectors(strings, embeddings, "embeddings")
        t0 = time.perf_counter()
        ctx = _lib.Context.default()
        dev = _lib.DeviceDense.upload(ctx, vec, True)
        if self.search_dtype is None:
            label, pairs, components = _lib.dense_components(ctx, dev, float(min_similarity))
            counts = {"pairs": pairs, "components": components}
        else:
            label, pairs, components, work = _lib.dense_components16(ctx, dev.derive16(self.search_dtype), dev, float(min_similarity),
                                                                     counters=True)
            counts = {"pairs": pairs, "components": components, "candidates": work["candidates"]}
        self.last_timings = {"device": (time.perf_counter() - t0) * 1e3, "frame": 0.0}
        self.last_counts = counts
        return label

    # a matcher is pickled by joblib (reference polyfuzz.py:429-457): the device copy stays behind
    def __getstate__(self):
        return {k: v for k, v in self.__dict__.items() if k not in ("_dev_to", "_dev_to_exact")}

    def __setstate__(self, state):
        self.__dict__.update(state)
        self.__dict__.setdefault("_compute_dtype", None)      # (pickled before the keywords existed)
        self.__dict__.setdefault("_precision", None)
        self.__dict__.setdefault("_rescore_multiplier", None)
        self.__dict__.setdefault("_binary", None)
        self.__dict__.setdefault("_rescore_to", None)
        self.__dict__.setdefault("_dev_to_exact_form", None)
        self.__dict__.setdefault("_search_dtype", None)
        self._dev_to = None
        self._dev_to_exact = None

    def _embed(self, strings: List[str]) -> np.ndarray:
        """ Embed with the user's callable and L2-normalise the rows (reference _embeddings.py:136-145) """
        if self.embedding_method is None:
            raise ValueError("polyfuzz_amd.Embeddings was created without an embedding_method: pass "
                             "embeddings_from / embeddings_to to match()")
        vec = np.asarray(self.embedding_method(list(strings)), dtype=np.float64)
        if vec.ndim != 2 or vec.shape[0] != len(strings):
            raise ValueError(f"embedding_method returned shape {vec.shape} for {len(strings)} strings")
        norms = np.sqrt((vec * vec).sum(axis=1, keepdims=True))
        norms[norms == 0.0] = 1.0
        return vec / norms
