"""BlockedEditDistance -- TF-IDF candidates rescored by an edit-distance scorer, both stages on the device.

The reference's edit-distance loop scores every from-string against every to-string (polyfuzz/models/_distance.py:89-102); that is
quadratic.  Record linkage at scale is done in two stages: a cheap, high-recall candidate search ("blocking") -- here the
character n-gram TF-IDF matcher's top `candidates` per from-string (polyfuzz/models/_utils.py:82-91), left in HBM by
TFIDF.match_device -- and an exact string scorer on those few pairs only: K10 (csrc/k10_pairs.hip), which scores the candidate
table under ratio / Levenshtein / OSA / Jaro / Jaro-Winkler and re-ranks every row.  K16 (csrc/k16_pairs_join.hip) holds the same
table against a threshold instead: the candidate pairs at or above a similarity, or their connected components.  With
`blocking_similarity` the threshold forms block by a TF-IDF THRESHOLD join instead of the table (K17): the pairs TFIDF.join reports,
left in HBM by TFIDF.join_device and walked there.
"""
import time
from typing import Callable, List, Tuple, Union

import numpy as np
import pandas as pd

from .. import _lib
from ._base import BaseMatcher
from ._distance import _device_scorer
from ._tfidf import TFIDF
from ._utils import clip_top_n, gather_column, object_column


def _check_count(name, value):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 1:
        raise ValueError(f"{name} must be an int >= 1, not {value!r}")
    return int(value)


class BlockedEditDistance(BaseMatcher):
    """
    The `top_n` best of a from-string's `candidates` nearest TF-IDF neighbours under an edit-distance scorer

    Arguments:
        scorer: "ratio" (rapidfuzz.fuzz.ratio, the default), "levenshtein", "osa", "jaro", "jaro_winkler" -- or any of the
                names and callables EditDistance resolves to one of these five (rapidfuzz.fuzz.ratio,
                rapidfuzz.distance.Levenshtein.normalized_similarity / OSA.normalized_similarity, jellyfish.jaro_similarity /
                jaro_winkler_similarity).  Every other scorer -- QRatio, token_sort_ratio, the per-pair scorers of K7, arbitrary
                callables -- has no pair kernel: NotImplementedError.
        candidates: TF-IDF neighbours per from-string that are scored (the blocking stage's top_n); at most 1024
        top_n: best choices per from-string that are kept, at most 64 and at most `candidates`
        min_similarity, n_gram_range, clean_string, remove_space_ngrams: the blocking TFIDF's (a candidate is a to-string whose
                TF-IDF cosine exceeds min_similarity)
        normalize: min-max normalise the similarity scores (reference _distance.py:83-86): ONE minimum and maximum over the
                cells that hold a choice; empty cells stay 0.0
        model_id: The name of the particular instance, used when comparing models
        blocking_similarity: None (the default): `join` and `components` score the top-`candidates` table.  A number b in [0, 1]:
                they score exactly the pairs TFIDF(n_gram_range, clean_string, remove_space_ngrams).join(from_list, to_list, b)
                reports (K15's rule: the float32 cosine as float64 >= b, never a pair without a common n-gram, a self-join's
                unordered pairs once) -- a row has as many candidates as it has such partners, thousands if need be.
                `candidates`, `top_n`, the constructor's min_similarity and `normalize` then play no part in these two calls, and
                the limit of 1024 candidates does not apply; `match` is unchanged: it ranks, and needs the table

    The frame has EditDistance.top_n's layout: From, To, Similarity[, To_2, Similarity_2, ...], the scorer's own float64 value,
    unrounded (ratio on 0..100, the others on 0..1), in the order (score descending, to-list index ascending); a cell without a
    choice is None / 0.0.  `candidates` and `top_n` are clipped to the number of distinct to-strings (reference _utils.py:54-56).

    What blocking means for the result:
      * it is the exact top-n AMONG THE CANDIDATES, not among all choices: a to-string the TF-IDF stage does not rank among a
        from-string's `candidates` nearest is never scored, however close its edit distance is;
      * a from-string that shares no n-gram with any to-string has no candidate and gets no match -- strings shorter than
        n_gram_range[0] after cleaning are such strings;
      * in a self-match (to_list=None) a row's own index is never a candidate and equal strings elsewhere in the list are: TF-IDF's
        self-match rule, not EditDistance's (which leaves out the first equal element of the list).

    join(from_list, to_list, min_similarity) and components(from_list, min_similarity) are the threshold forms (K16): every
    candidate pair whose score is >= min_similarity, as a frame of pairs or as one component label per string.  They are exact
    among the SYMMETRISED candidates -- in a self-join the unordered pairs {i, j} with j among i's candidates or i among j's, each
    scored once with the lower position as the from-string --; a row's own index is never a candidate; `top_n` and `normalize`
    play no part; "ratio" (0..100) is refused: the scorers are "levenshtein", "osa", "jaro" and "jaro_winkler".

    With blocking_similarity = b (K17) the two calls are exact among the pairs of the TF-IDF threshold join at b instead: every
    such pair is scored once, in a self-join with the lower position as the from-string; frame, order and labels are the same.

    match(..., re_train=False) reuses the fitted TF-IDF side, and the resident raw to-list when the list it is handed equals the
    one uploaded last (EditDistance's rule).  There is no CPU fallback.  Pickling leaves the device handles behind.
    """
    last_counts = None      # {"candidates", "scored", "pairs"[, "items"][, "components"]} of the last `join` / `components` call
    blocking_similarity = None      # (a matcher pickled before the attribute existed reads as None)

    def __init__(self,
                 scorer: Union[Callable, str, None] = "ratio",
                 candidates: int = 32,
                 top_n: int = 1,
                 min_similarity: float = 0.0,
                 n_gram_range: Tuple[int, int] = (3, 3),
                 clean_string: bool = True,
                 remove_space_ngrams: bool = True,
                 normalize: bool = True,
                 model_id: str = None,
                 blocking_similarity: float = None):
        super().__init__(model_id)
        self.type = "BlockedEditDistance"
        self._scorer_name = _device_scorer(scorer)
        if self._scorer_name not in _lib.PAIR_SCORERS:
            raise NotImplementedError(
                f"polyfuzz_amd.BlockedEditDistance rescores candidates under {tuple(_lib.PAIR_SCORERS)}; scorer {scorer!r} has no "
                "pair kernel and there is no CPU fallback")
        self.scorer = scorer
        self.candidates = _check_count("candidates", candidates)
        self.top_n = _check_count("top_n", top_n)
        if self.top_n > self.candidates:
            raise ValueError(f"top_n = {self.top_n} exceeds candidates = {self.candidates}: only candidates are ranked")
        if isinstance(min_similarity, bool) or not isinstance(min_similarity, (int, float, np.integer, np.floating)):
            raise ValueError(f"min_similarity must be a number, not {min_similarity!r}")
        try:
            lo, hi = n_gram_range
            if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in (lo, hi)) or not 1 <= lo <= hi:
                raise TypeError
        except TypeError:
            raise ValueError(f"n_gram_range must be a pair of ints 1 <= low <= high, not {n_gram_range!r}") from None
        self.min_similarity = float(min_similarity)
        self.n_gram_range = (int(lo), int(hi))
        self.clean_string = bool(clean_string)
        self.remove_space_ngrams = bool(remove_space_ngrams)
        self.normalize = normalize
        if blocking_similarity is not None:
            try:
                blocking_similarity = _lib.check_min_similarity(blocking_similarity)
            except ValueError:
                raise ValueError(f"blocking_similarity must be None or a number in [0, 1], not {blocking_similarity!r}") from None
        self.blocking_similarity = blocking_similarity
        self._tfidf = TFIDF(n_gram_range=self.n_gram_range, clean_string=self.clean_string, min_similarity=self.min_similarity,
                            top_n=self.candidates, remove_space_ngrams=self.remove_space_ngrams)
        self._to_dev = self._to_names = None     # device copy of the last raw to-list (+ the cached K4 plan K10 reads its alphabet from)
        self.last_timings = None

    def match(self,
              from_list: List[str],
              to_list: List[str] = None,
              re_train: bool = True) -> pd.DataFrame:
        """The top_n best candidates of every from-string (class docstring)."""
        idx, score, names, t = self._rescore(from_list, to_list, re_train)
        ntop = idx.shape[1]
        data = {"From": object_column(from_list)}
        for r in range(ntop):
            data["To" if r == 0 else f"To_{r + 1}"] = gather_column(names, np.ascontiguousarray(idx[:, r]))
            data["Similarity" if r == 0 else f"Similarity_{r + 1}"] = score[:, r].copy()
        matches = pd.DataFrame(data, copy=False)
        held = idx >= 0
        if self.normalize and held.any():      # _distance.py:83-86 over the cells that hold a choice
            lo, hi = score[held].min(), score[held].max()
            for r in range(ntop):
                c = "Similarity" if r == 0 else f"Similarity_{r + 1}"
                matches[c] = np.where(held[:, r], (score[:, r] - lo) / (hi - lo), 0.0)
        self.last_timings = {"tfidf": (t[1] - t[0]) * 1e3, "k10": (t[2] - t[1]) * 1e3, "frame": (time.perf_counter() - t[2]) * 1e3}
        return matches

    def _rescore(self, from_list, to_list, re_train):
        """(index int32[n, ntop], score float64[n, ntop], the choices' list, (start, candidates final, rescored) times)"""
        m = clip_top_n(self.candidates, to_list)                  # what TFIDF.match_device leaves per row (_utils.py:54-56)
        ntop = max(1, clip_top_n(self.top_n, to_list))
        if ntop > max(m, 1):
            raise ValueError(f"top_n = {ntop} exceeds the {m} candidates per from-string")
        if ntop > _lib.PAIR_MAX_TOP_N:
            raise _lib.PfzUnsupported(-4, f"BlockedEditDistance.top_n = {ntop} exceeds the limit of {_lib.PAIR_MAX_TOP_N} best choices per from-string")
        if m > _lib.PAIR_MAX_CANDIDATES:
            raise _lib.PfzUnsupported(-4, f"BlockedEditDistance.candidates = {m} exceeds the limit of {_lib.PAIR_MAX_CANDIDATES} per from-string")
        ctx, f_dev, t_dev, cand, names, t0, t1 = self._block(from_list, to_list, re_train)
        idx, score = _lib.pairs_rescore_topn(ctx, f_dev, t_dev, cand, self._scorer_name, ntop)
        return idx, score, names, (t0, t1, time.perf_counter())

    def _block(self, from_list, to_list, re_train, threshold=None):
        """The blocking stage and the two raw lists on the device: (context, from-list, to-list -- the from-list's own handle in a
        self-match --, the candidate table in HBM, the choices' list, start time, time when the table was final).  threshold: the
        candidates are the pairs of the TF-IDF threshold join at that cosine (a _lib.DevicePairs) instead of the table"""
        self_match = to_list is None
        ctx = _lib.Context.default()
        from ._rapidfuzz import upload_for
        t0 = time.perf_counter()
        names = from_list if self_match else to_list
        # the resident raw to-list stands for the list it was made from and for no other: compared by content (EditDistance._best)
        snap = None if self_match else tuple(to_list)
        reuse_to = re_train is False and not self_match and self._to_dev is not None and snap == self._to_names
        held = self._to_dev
        self._to_dev = self._to_names = None      # set again below, once this call's to-list is resident
        self._tfidf.top_n = self.candidates
        if threshold is None:
            cand = self._tfidf.match_device(from_list, to_list, re_train=re_train)      # enqueued: the table stays in HBM
        else:
            cand = self._tfidf.join_device(from_list, to_list, threshold, re_train=re_train)      # the sorted keys stay in HBM
        f_dev = upload_for(ctx, self._scorer_name, from_list)                      # (host work while the device blocks)
        if self_match:
            t_dev = f_dev
        else:
            t_dev = held if reuse_to else upload_for(ctx, self._scorer_name, names)
            self._to_dev, self._to_names = t_dev, snap
        ctx.sync()          # (for last_timings' split alone: K10's and K16's entries block behind the same stream anyway)
        return ctx, f_dev, t_dev, cand, names, t0, time.perf_counter()

    def _check_join(self, what, min_similarity, to_list):
        """the refusals of join / components, before any device call: the scorer, then the threshold -> float"""
        if self._scorer_name not in _lib.PAIR_JOIN_SCORERS:
            raise NotImplementedError(
                f"BlockedEditDistance.{what} runs on the GPU for the scorers {tuple(_lib.PAIR_JOIN_SCORERS)}; scorer "
                f"{self._scorer_name!r} lives on 0..100, where a min_similarity in [0, 1] is ambiguous, and has no threshold kernel")
        t = _lib.check_min_similarity(min_similarity)
        m = clip_top_n(self.candidates, to_list)                  # as _rescore clips it
        if self.blocking_similarity is None and m > _lib.PAIR_MAX_CANDIDATES:
            raise _lib.PfzUnsupported(-4, f"BlockedEditDistance.candidates = {m} exceeds the limit of {_lib.PAIR_MAX_CANDIDATES} per from-string")
        return t

    def join(self,
             from_list: List[str],
             to_list: List[str] = None,
             min_similarity: float = 0.8,
             re_train: bool = True) -> pd.DataFrame:
        """ Every CANDIDATE pair at least `min_similarity` similar under the scorer (K16): the frame From, To, Similarity with one
        row per pair, ordered by from-index, then to-index.  A from-string without such a partner has no row.  Similarity is the
        scorer's own float64, unrounded -- the value `match` computes for the pair -- and a pair is kept iff that float64 is >=
        min_similarity (equal is kept).

        The candidates are `match`'s: every from-string's `candidates` nearest TF-IDF neighbours (clipped to the number of distinct
        to-strings), found by the same blocking stage and left in HBM.  Exact among them: every candidate pair is scored to its
        end; a pair the blocking stage did not propose is never scored, however similar.

        to_list None: the self-join of from_list over the SYMMETRISED candidate table -- every unordered pair of positions {i, j},
        i != j, with j among i's candidates or i among j's, once, as From = from_list[min], To = from_list[max], scored with the
        lower position as the from-string.  A row's own index is never a candidate; equal strings at different positions are a pair.

        `normalize` is NOT applied: a rescaled score no longer means the threshold.  `top_n` plays no part.
        re_train=False reuses the fitted TF-IDF side and the resident raw to-list by `match`'s rule.

        Scorers "levenshtein", "osa", "jaro" and "jaro_winkler" (NotImplementedError otherwise: "ratio" lives on 0..100);
        min_similarity: a number in [0, 1] (ValueError otherwise).  Sets last_timings = {"tfidf", "k16", "frame"} and last_counts =
        {"candidates": table cells that are a candidate pair, "scored": distinct pairs scored, "pairs": hits}.

        With blocking_similarity = b (K17) the candidates are the pairs of the TF-IDF threshold join at b (class docstring), walked
        in HBM as (row, slice) work items; last_counts = {"candidates": the join's pairs, "scored" (== candidates), "pairs",
        "items": work items}; last_timings["tfidf"] is K15 with its sort. """
        t = self._check_join("join", min_similarity, to_list)
        b = self.blocking_similarity
        ctx, f_dev, t_dev, cand, names, t0, t1 = self._block(from_list, to_list, re_train, b)
        join = _lib.pairs_join if b is None else _lib.pairs_join_keys
        row_ptr, idx, sim, counts = join(ctx, f_dev, None if to_list is None else t_dev, cand, self._scorer_name, t, counters=True)
        t2 = time.perf_counter()
        frm = np.repeat(np.arange(len(from_list), dtype=np.int32), np.diff(row_ptr))
        matches = pd.DataFrame({"From": gather_column(from_list, frm), "To": gather_column(names, idx), "Similarity": sim}, copy=False)
        self.last_timings = {"tfidf": (t1 - t0) * 1e3, "k16": (t2 - t1) * 1e3, "frame": (time.perf_counter() - t2) * 1e3}
        self.last_counts = counts
        return matches

    def components(self,
                   from_list: List[str],
                   min_similarity: float = 0.8) -> np.ndarray:
        """ Clusters of from_list (K16 into K12's forest): int32 labels, label[i] = the smallest position in i's connected component
        of the graph whose edges are the pairs `join(from_list, min_similarity=...)` reports -- "A ~ B and B ~ C put A, B and C
        together".  A string with no partner is its own (label[i] == i).  Deterministic.  The pairs are united on the device where
        they are found and never stored or downloaded.  Blocked: two strings share a component only through chains of CANDIDATE
        pairs, so equal strings do whenever the blocking stage lists one for the other -- not when there are more copies than
        `candidates`, or when the string has no n-gram.  polyfuzz_amd.linkage.connected_components turns the labels into the three
        dicts single_linkage returns.

        `normalize` is NOT applied.  Scorers and min_similarity as for `join`.  Sets last_timings = {"tfidf", "k16", "frame"} and
        last_counts = {"candidates", "scored", "pairs", "components"}.

        With blocking_similarity = b (K17) the edges are the hits among the pairs of the TF-IDF threshold join at b: equal strings
        share a component however many copies there are, as long as they have an n-gram; last_counts gains "items". """
        t = self._check_join("components", min_similarity, None)
        b = self.blocking_similarity
        ctx, f_dev, _, cand, _, t0, t1 = self._block(from_list, None, True, b)
        comp = _lib.pairs_components if b is None else _lib.pairs_components_keys
        label, pairs, components, counts = comp(ctx, f_dev, cand, self._scorer_name, t, counters=True)
        self.last_timings = {"tfidf": (t1 - t0) * 1e3, "k16": (time.perf_counter() - t1) * 1e3, "frame": 0.0}
        self.last_counts = dict(counts, components=components)
        return label

    # a matcher is pickled by joblib (reference polyfuzz.py:429-457): device handles stay behind (the TFIDF keeps a host copy of its fit)
    def __getstate__(self):
        return {k: v for k, v in self.__dict__.items() if k not in ("_to_dev", "_to_names")}

    def __setstate__(self, state):
        self.__dict__.update(state)
        self._to_dev = self._to_names = None
