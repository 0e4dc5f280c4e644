"""EditDistance -- the reference's all-pairs edit-distance matcher
(polyfuzz/models/_distance.py:14-102) on the MI355X engine.

The reference scores every (from, to) pair with `scorer` (default
rapidfuzz.fuzz.ratio, _distance.py:32) in a Python loop / joblib pool and keeps the
first arg-max per from-string.  Here the whole score matrix + arg-max is one HIP
kernel (K4: bit-parallel LCS, fused first-max reduction).  `scorer` may be any
rapidfuzz.fuzz scorer (or its name): ratio / QRatio / token_sort_ratio run through K4,
WRatio / partial_ratio / token_set_ratio / token_ratio / partial_token_* through K7;
or jellyfish.jaro_similarity / jaro_winkler_similarity (the scorer of the reference's
custom-model tutorial, docs/tutorial/models/models.md:46-58), which run through K8;
or rapidfuzz's Levenshtein.normalized_similarity / OSA.normalized_similarity, which run
through K9; or rapidfuzz's Indel.normalized_similarity ("indel": the default ratio on the 0..1 scale), whose best matches are
K4's and whose threshold forms run through K13; any other callable raises -- there is no CPU path to fall back to.
"""
import time
from typing import Callable, List, Union

import numpy as np
import pandas as pd

from .. import _lib
from ._base import BaseMatcher
from ._utils import gather_column, object_column, pair_frame, pair_frame_blocks


_JARO_NAMES = {"jaro": "jaro", "jaro_similarity": "jaro", "jaro_winkler": "jaro_winkler", "jaro_winkler_similarity": "jaro_winkler"}
_JELLYFISH_FUNCTIONS = ("jaro_similarity", "jaro_winkler_similarity")


def _jaro_scorer(scorer) -> str:
    """K8's name ("jaro" / "jaro_winkler") of the jellyfish function `scorer` stands for, or '': one of the four names, a
    callable of jellyfish's that carries one of its two names, or -- compiled functions do not always say where they are
    from -- the very object jellyfish exports under that name.  A functools.partial (long_tolerance=True has no kernel) or
    somebody else's function of the same name is neither."""
    if isinstance(scorer, str):
        return _JARO_NAMES.get(scorer, "")
    name = getattr(scorer, "__name__", "")
    if name in _JELLYFISH_FUNCTIONS and (getattr(scorer, "__module__", "") or "").split(".")[0] == "jellyfish":
        return _JARO_NAMES[name]
    try:
        import jellyfish
    except ImportError:
        return ""
    return next((_JARO_NAMES[n] for n in _JELLYFISH_FUNCTIONS if getattr(jellyfish, n, None) is scorer), "")


_LEV_NAMES = {"levenshtein": "levenshtein", "levenshtein_normalized_similarity": "levenshtein", "osa": "osa",
              "osa_normalized_similarity": "osa"}
_LEV_MODULES = {"Levenshtein": "levenshtein", "Levenshtein_py": "levenshtein", "OSA": "osa", "OSA_py": "osa"}


def _lev_scorer(scorer) -> str:
    """K9's name ("levenshtein" / "osa") of the rapidfuzz function `scorer` stands for, or '': one of the four names; the very
    object rapidfuzz.distance.Levenshtein.normalized_similarity / rapidfuzz.distance.OSA.normalized_similarity (by identity:
    the check that counts); or a callable named `normalized_similarity` whose module is rapidfuzz.distance.Levenshtein,
    .Levenshtein_py, .OSA or .OSA_py -- what names rapidfuzz's compiled functions actually carry could not be looked up where
    this was written, rapidfuzz is not installed there.  normalized_distance, distance and similarity (an arg-max over a
    distance is a caller's mistake; similarity is not on the 0..1 scale), a functools.partial (weights, score_cutoff and
    processor have no kernel) and somebody else's function of the same name are none of these."""
    if isinstance(scorer, str):
        return _LEV_NAMES.get(scorer, "")
    try:
        from rapidfuzz.distance import OSA, Levenshtein
        for mod, name in ((Levenshtein, "levenshtein"), (OSA, "osa")):
            if getattr(mod, "normalized_similarity", None) is scorer:
                return name
    except ImportError:
        pass
    module = getattr(scorer, "__module__", "") or ""
    if getattr(scorer, "__name__", "") == "normalized_similarity" and module.startswith("rapidfuzz.distance."):
        return _LEV_MODULES.get(module.split(".")[-1], "")
    return ""


_INDEL_NAMES = ("indel", "indel_normalized_similarity")


def _indel_scorer(scorer) -> str:
    """"indel" when `scorer` stands for rapidfuzz.distance.Indel.normalized_similarity, else '': one of the two names; that very
    object (by identity); or a callable named `normalized_similarity` whose module is rapidfuzz.distance.Indel or .Indel_py.
    The rules, and what stays refused (distance, similarity, normalized_distance, partials), are _lev_scorer's."""
    if isinstance(scorer, str):
        return "indel" if scorer in _INDEL_NAMES else ""
    try:
        from rapidfuzz.distance import Indel
        if getattr(Indel, "normalized_similarity", None) is scorer:
            return "indel"
    except ImportError:
        pass
    module = getattr(scorer, "__module__", "") or ""
    if getattr(scorer, "__name__", "") == "normalized_similarity" and module in ("rapidfuzz.distance.Indel", "rapidfuzz.distance.Indel_py"):
        return "indel"
    return ""


def _device_scorer(scorer) -> str:
    """Name of the rapidfuzz.fuzz scorer (or K8's name of the jellyfish scorer, or K9's of the rapidfuzz.distance scorer)
    `scorer` stands for, or '' when it has no kernel."""
    from ._rapidfuzz import _DEVICE_SCORERS
    if scorer is None:
        return "ratio"                                     # the reference's default (_distance.py:32)
    if _jaro_scorer(scorer):
        return _jaro_scorer(scorer)
    if _lev_scorer(scorer):
        return _lev_scorer(scorer)
    if _indel_scorer(scorer):
        return _indel_scorer(scorer)
    name = scorer if isinstance(scorer, str) else getattr(scorer, "__name__", "")
    if not isinstance(scorer, str) and "rapidfuzz" not in (getattr(scorer, "__module__", "") or ""):
        return ""
    return name if name in _DEVICE_SCORERS else ""


# the scorers whose kernels have a top-n form here (K4 on one fixed string per list element, K9); Jaro (K8) and the per-pair scorers
# (K7) prune around a single best and keep their arg-max only -- their top-n forms are JaroWinkler.match(top_n=) (K21) and RapidFuzz.top_n (K19)
_TOP_N_SCORERS = ("ratio", "QRatio", "token_sort_ratio", "levenshtein", "osa", "indel")
_TOP_N_MAX = 64                 # one list entry per lane of a wave (csrc/topn_wave.h)
_JOIN_SCORERS = ("levenshtein", "osa", "indel")      # the scorers with a threshold kernel (K11; "indel": K13)


def _top_n_choices(ctx, name, from_list, names, skip, self_match, to_dev, ntop):
    """(index int32[n, ntop], score float64[n, ntop]) of every from-string's ntop best choices under scorer `name`, in the order
    (score descending, choice index ascending); the arguments are best_choice_async's"""
    from ._rapidfuzz import upload_for
    f_dev = upload_for(ctx, name, from_list)
    t_dev = f_dev if self_match else (to_dev if to_dev is not None else upload_for(ctx, name, names))
    if name in _lib.LEV_SCORERS:
        return _lib.lev_topn(ctx, f_dev, t_dev, name, ntop, skip)
    idx, score = _lib.indel_topn(ctx, f_dev, t_dev, ntop, skip)
    if name == "indel":
        # K4's order is this scorer's (indel_similarity and the ratio compare every two pairs alike, ties included:
        # tests/test_indel_join_cpu.py); the scores go from the 0..100 scale to the definition's 0..1, bit for bit
        from ._rapidfuzz import indel_scores
        return idx, indel_scores(from_list, names, idx, score)
    if name == "QRatio":
        # QRatio differs from ratio only when BOTH strings are empty (0 instead of 100): an empty from-string scores 0 against
        # every choice, so its columns are simply its first choices
        # (the skip code alone says which: 0 .. ntop - 1 without the one choice left out, or the ntop behind "everything up to")
        n_to = len(names)
        for i in [i for i, s in enumerate(from_list) if len(s) == 0]:
            sk = -1 if skip is None else int(skip[i])
            if sk <= -2:
                first = np.arange(-1 - sk, min(n_to, -1 - sk + ntop))
            else:
                first = np.arange(0, min(n_to, ntop + 1))
                first = first[first != sk][:ntop]
            idx[i], score[i] = -1, 0.0
            idx[i, :len(first)] = first
    return idx, score


class EditDistance(BaseMatcher):
    """
    Calculate the Edit Distance between lists of strings (Indel ratio, rapidfuzz.fuzz.ratio)

    Arguments (reference _distance.py:18-23):
        n_jobs: accepted for compatibility; the GPU kernel ignores it
        scorer: a rapidfuzz.fuzz scorer or its name; default "ratio" / rapidfuzz.fuzz.ratio.  Or
                jellyfish.jaro_similarity / jellyfish.jaro_winkler_similarity, or one of the names "jaro",
                "jaro_similarity", "jaro_winkler", "jaro_winkler_similarity".  Or
                rapidfuzz.distance.Levenshtein.normalized_similarity / rapidfuzz.distance.OSA.normalized_similarity, or
                one of the names "levenshtein", "levenshtein_normalized_similarity", "osa", "osa_normalized_similarity".
                Or rapidfuzz.distance.Indel.normalized_similarity, or one of the names "indel",
                "indel_normalized_similarity".
                Other callables -- a functools.partial of these included -- have no kernel (NotImplementedError).
        model_id: The name of the particular instance, used when comparing models
        normalize: Whether to min-max normalize the similarity scores (_distance.py:83-86)

    scorer "ratio" (K4): from-strings of up to 1024 characters run in the register-resident word classes (eight / four at
    a time up to 16 / 32 characters); longer ones, and alphabets whose match table (distinct code points of the to-list x
    words) exceeds 60 KiB of LDS, take a general -- slower -- kernel with its state in global memory.  The per-pair
    scorers (K7: WRatio, partial_ratio, the token_set family): from-strings of up to 256 characters and 32 distinct tokens
    in the LDS kernel, anything beyond (and to-strings beyond 32 distinct tokens) in K7's general kernel, which is slow.
    Any length and any alphabet is accepted.  There is no CPU fallback.

    The Jaro scorers (K8): Similarity is the scorer's own float64 value on jellyfish's 0..1 scale, unscaled, as the
    reference passes it through; jellyfish's default arguments (no long_tolerance), on code points.  From-strings of up to
    64 characters against to-strings of up to 256 run in registers; longer strings take a general -- slow -- kernel.  PARITY UNPINNED:
    jellyfish is not importable where this was built, the scorers are the restatement of its definition in
    include/polyfuzz_hip.h (tests/test_jaro_cpu.py compares with jellyfish itself wherever it is installed).

    Levenshtein and OSA (K9): Similarity is rapidfuzz's normalized_similarity, 1 - d / max(|from|, |to|) as float64 on the 0..1
    scale (1.0 for two empty strings), unscaled, as the reference passes a scorer's value through; d is the unit-cost edit
    distance, for "osa" with the transposition of two adjacent characters as one edit (optimal string alignment; unrestricted
    Damerau-Levenshtein, Hamming, custom weights and the distance callables have no kernel).  From-strings of up to 64
    characters run in registers against to-strings of any length, longer ones in a general -- slow -- kernel; a from-string's
    to-strings are walked from the nearest length outwards and left alone where the difference in length alone puts them below
    the best so far.  PARITY UNPINNED beyond the oracle; live pin armed: rapidfuzz is not importable where this was built,
    the scorers are the restatement of its definition in include/polyfuzz_hip.h (tests/test_levenshtein_cpu.py compares with
    rapidfuzz itself wherever it is installed).

    Indel ("indel"): Similarity is rapidfuzz.distance.Indel.normalized_similarity, 1 - (|from| + |to| - 2 lcs) / (|from| + |to|)
    as float64 on the 0..1 scale (1.0 for two empty strings), unscaled -- rapidfuzz.fuzz.ratio divided by 100, computed by its own
    formula.  `match` and `top_n` are K4's passes (the two scales order every two pairs alike, ties included); the host turns
    each score into the definition's float64 from the integer LCS it recovers from K4's ratio and the two lengths, verified bit
    for bit.  `join` and `components` run through K13.

    top_n (attribute, default 1; the constructor keeps the reference's signature: `m = EditDistance(scorer="osa"); m.top_n = 5`):
    the number of best choices per from-string.  The reference's facade has it for TFIDF and Embeddings only (polyfuzz.py:100),
    its edit-distance loop cannot afford more than the one np.argmax (_distance.py:89-102); here the columns To, Similarity,
    To_2, Similarity_2, ... (the layout of cosine_similarity's frame) are the choices in the order np.argsort(-scores,
    kind="stable") gives: score descending, equal scores in list order, exact, on the device -- for "ratio", "QRatio",
    "token_sort_ratio", "indel" (K4), "levenshtein" and "osa" (K9).  The scores are the scorer's own float64, unrounded; `normalize` takes
    ONE minimum and maximum over all Similarity columns.  top_n is clipped to the number of choices every row has (the
    reference's clip, _utils.py:55-56); more than 64 after clipping raises _lib.PfzUnsupported; the Jaro scorers and the
    per-pair scorers (K7) raise NotImplementedError from `match` -- their kernels keep a single best (for the per-pair scorers the
    top-n form is RapidFuzz.top_n, K19; for the Jaro scorers JaroWinkler.match(top_n=), K21).  An int >= 1, else
    ValueError; kept through pickling.

    join (method, "levenshtein", "osa" and "indel"): every pair at least `min_similarity` similar instead of each string's best --
    the threshold form (K11; "indel": K13), exact, with a self-join that reports each unordered pair once; see `join`.

    components (method, "levenshtein", "osa" and "indel"): the connected components of that self-join's graph as one int32 label
    per string -- near-duplicate clusters, computed on the device where the pairs are found (K12; "indel": K13); see `components`.
    """
    last_counts = None      # {"pairs", "components"} of the last `components` call


    def __init__(self,
                 n_jobs: int = 1,
                 scorer: Union[Callable, str, None] = "ratio",
                 model_id: str = None,
                 normalize: bool = True):
        super().__init__(model_id)
        self.type = "EditDistance"
        self._scorer_name = _device_scorer(scorer)
        if not self._scorer_name:
            raise NotImplementedError(
                "polyfuzz_amd.EditDistance runs the rapidfuzz.fuzz scorers, jellyfish's two Jaro scorers and rapidfuzz's Levenshtein / OSA / "
                "Indel normalized_similarity on the GPU; "
                f"scorer {scorer!r} has no HIP kernel and there is no CPU fallback")
        self.scorer = scorer
        self.normalize = normalize
        self.n_jobs = n_jobs
        self._to_dev = self._to_names = None     # device copy (+ cached K4 plan) of the last to-list
        self.last_timings = None
        self._top_n = 1

    @property
    def top_n(self) -> int:
        """best choices per from-string (class docstring); 1: the best match, the reference's frame"""
        return self.__dict__.get("_top_n", 1)          # (a matcher pickled before the attribute existed)

    @top_n.setter
    def top_n(self, value):
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 1:
            raise ValueError(f"top_n must be an int >= 1, not {value!r}")
        self._top_n = int(value)

    def match(self,
              from_list: List[str],
              to_list: List[str] = None,
              **kwargs) -> pd.DataFrame:
        """ Best match (first maximum of the ratio) of every from-string (reference _distance.py:46-87).

        The reference scores against the to_list it is handed, always (`PolyFuzz.transform` passes `self.to_list`,
        polyfuzz.py:234-240).  `re_train=False` only lets this matcher re-use what is resident: when the list it is handed
        IS the previous call's (the same object, or an equal list), its device copy and K4 plan (alphabet, length-sorted
        packed groups) are used again -- no upload, no preparation.  Any other list is uploaded. """
        if self.top_n > 1:
            return self._match_top_n(from_list, to_list, reuse_to=kwargs.get("re_train", True) is False)
        t0 = time.perf_counter()
        pending, names = self._best(from_list, to_list, reuse_to=kwargs.get("re_train", True) is False)
        blocks = pair_frame_blocks(from_list)        # (the From column: host work while the device scores)
        idx, score = pending.result()
        t1 = time.perf_counter()
        matches = pair_frame(from_list, names, idx, score, blocks=blocks)
        if self.normalize:      # global min-max over the best scores, _distance.py:83-86
            matches["Similarity"] = (matches["Similarity"] -
                                     matches["Similarity"].min()) / (matches["Similarity"].max() -
                                                                     matches["Similarity"].min())
        self.last_timings = {"device": (t1 - t0) * 1e3, "frame": (time.perf_counter() - t1) * 1e3}
        return matches

    def _match_top_n(self, from_list, to_list, reuse_to):
        """the frame From, To, Similarity, To_2, Similarity_2, ... of the top_n best choices (class docstring)"""
        if self._scorer_name not in _TOP_N_SCORERS:
            raise NotImplementedError(
                f"EditDistance.top_n > 1 runs on the GPU for the scorers {_TOP_N_SCORERS}; the kernels of scorer "
                f"{self._scorer_name!r} keep a single best per from-string -- set top_n = 1")
        t0 = time.perf_counter()
        # every row has len(to_list) choices, or one less in a self-match (reference _utils.py:55-56, applied to choices)
        ntop = max(1, min(self.top_n, (len(from_list) - 1) if to_list is None else len(to_list)))
        if ntop > _TOP_N_MAX:
            raise _lib.PfzUnsupported(-4, f"EditDistance.top_n = {ntop} exceeds the limit of {_TOP_N_MAX} best choices per from-string")
        (idx, score), names = self._best(from_list, to_list, reuse_to=reuse_to, top_n=ntop)
        t1 = time.perf_counter()
        data = {"From": object_column(from_list)}
        for r in range(ntop):
            data["To" if r == 0 else f"To_{r + 1}"] = gather_column(names, np.ascontiguousarray(idx[:, r]))
            data["Similarity" if r == 0 else f"Similarity_{r + 1}"] = score[:, r].copy()
        matches = pd.DataFrame(data, copy=False)
        if self.normalize and score.size:      # _distance.py:83-86 with one minimum and one maximum over all Similarity columns
            lo, hi = score.min(), score.max()
            for r in range(ntop):
                c = "Similarity" if r == 0 else f"Similarity_{r + 1}"
                matches[c] = (matches[c] - lo) / (hi - lo)
        self.last_timings = {"device": (t1 - t0) * 1e3, "frame": (time.perf_counter() - t1) * 1e3}
        return matches

    def join(self,
             from_list: List[str],
             to_list: List[str] = None,
             min_similarity: float = 0.8) -> pd.DataFrame:
        """ Every pair at least `min_similarity` similar (K11; scorer "indel": K13): the frame From, To, Similarity with one row per pair, ordered by
        from-index, then to-index.  A from-string without a partner has no row.  Similarity is the scorer's own float64,
        unrounded, and a pair is kept iff that float64 is >= min_similarity (rapidfuzz's score_cutoff: equal is kept).
        Exact: every such pair is found, whatever their number.

        `normalize` is NOT applied: a rescaled score no longer means the threshold.

        to_list None: the self-join of from_list -- every unordered pair of positions i < j once, as From = from_list[i],
        To = from_list[j]; never a string with itself, but equal strings at different positions are a pair.

        Scorers "levenshtein", "osa" and "indel" only (NotImplementedError otherwise; "ratio" under its own name lives on the
        0..100 scale and has no join: "indel" is the same metric on 0..1); min_similarity: a number in [0, 1]
        (ValueError otherwise).  The frame has the columns single_linkage reads; for the clusters of the self-join's graph
        (its connected components) see `components`, which never builds the frame. """
        if self._scorer_name not in _JOIN_SCORERS:
            raise NotImplementedError(
                f"EditDistance.join runs on the GPU for the scorers {_JOIN_SCORERS}; scorer {self._scorer_name!r} has no "
                "threshold kernel")
        if (isinstance(min_similarity, bool) or not isinstance(min_similarity, (int, float, np.integer, np.floating))
                or not 0.0 <= float(min_similarity) <= 1.0):      # (NaN compares false)
            raise ValueError(f"min_similarity must be a number in [0, 1], not {min_similarity!r}")
        from ._rapidfuzz import upload_for
        t0 = time.perf_counter()
        ctx = _lib.Context.default()
        names = from_list if to_list is None else to_list
        f_dev = upload_for(ctx, self._scorer_name, from_list)
        t_dev = None if to_list is None else upload_for(ctx, self._scorer_name, to_list)
        if self._scorer_name == "indel":
            row_ptr, idx, _, sim = _lib.indel_join(ctx, f_dev, t_dev, float(min_similarity))
        else:
            row_ptr, idx, _, sim = _lib.lev_join(ctx, f_dev, t_dev, self._scorer_name, float(min_similarity))
        t1 = time.perf_counter()
        frm = np.repeat(np.arange(len(from_list), dtype=np.int32), np.diff(row_ptr))
        matches = pd.DataFrame({"From": gather_column(from_list, frm), "To": gather_column(names, idx), "Similarity": sim}, copy=False)
        self.last_timings = {"device": (t1 - t0) * 1e3, "frame": (time.perf_counter() - t1) * 1e3}
        return matches

    def components(self,
                   from_list: List[str],
                   min_similarity: float = 0.8) -> np.ndarray:
        """ Near-duplicate clusters of from_list (K12; scorer "indel": K13): int32 labels, label[i] = the smallest position in i's connected
        component of the graph whose edges are the pairs `join(from_list, min_similarity=...)` reports -- "A ~ B and B ~ C put A,
        B and C together".  Equal strings share a component; a string with no partner is its own (label[i] == i).  Exact and
        deterministic.  The pairs are united on the device where they are found and never stored or downloaded: device memory
        is O(len(from_list)) whatever their number.  polyfuzz_amd.linkage.connected_components turns the labels into the three
        dicts single_linkage returns.

        `normalize` is NOT applied: there is no score to rescale.

        Scorers "levenshtein", "osa" and "indel" only (NotImplementedError otherwise); min_similarity: a number in [0, 1]
        (ValueError otherwise).  Sets last_timings and last_counts = {"pairs": hits, "components": components}. """
        if self._scorer_name not in _JOIN_SCORERS:
            raise NotImplementedError(
                f"EditDistance.components runs on the GPU for the scorers {_JOIN_SCORERS}; scorer {self._scorer_name!r} has no "
                "threshold kernel")
        if (isinstance(min_similarity, bool) or not isinstance(min_similarity, (int, float, np.integer, np.floating))
                or not 0.0 <= float(min_similarity) <= 1.0):      # (NaN compares false)
            raise ValueError(f"min_similarity must be a number in [0, 1], not {min_similarity!r}")
        from ._rapidfuzz import upload_for
        t0 = time.perf_counter()
        ctx = _lib.Context.default()
        f_dev = upload_for(ctx, self._scorer_name, from_list)
        if self._scorer_name == "indel":
            label, pairs, components = _lib.indel_components(ctx, f_dev, float(min_similarity))
        else:
            label, pairs, components = _lib.lev_components(ctx, f_dev, self._scorer_name, float(min_similarity))
        self.last_timings = {"device": (time.perf_counter() - t0) * 1e3, "frame": 0.0}
        self.last_counts = {"pairs": pairs, "components": components}
        return label

    def _best(self, from_list, to_list, reuse_to=False, top_n=None, choices=_top_n_choices):
        """the enqueued best-choice pass (top_n None) or `choices(...)`'s top_n best (its arguments: _top_n_choices's), and the
        names the indices stand for; the self-match's skip codes, the resident to-list and its reuse are decided here, once"""
        ctx = _lib.Context.default()
        self_match = to_list is None
        skip = None
        if self_match:
            names = from_list
            # list.remove(from_string) drops the FIRST equal element (_distance.py:93-96)
            first = {}
            for j, s in enumerate(names):
                first.setdefault(s, j)
            skip = np.fromiter((first[s] for s in from_list), np.int32, len(from_list))
        else:
            names = to_list
        # the resident copy stands for the list it was made from and for no other
        # -- compared by CONTENT against a snapshot taken when it was uploaded (the caller's list may have been changed
        # in place since; an ndarray / Series to-list has no list `==`)
        snap = None if self_match else tuple(to_list)
        reuse_to = reuse_to and not self_match and self._to_dev is not None and snap == self._to_names
        held = (self._to_dev, self._to_names)
        self._to_dev = self._to_names = None      # set again below, once this call's to-list is resident
        if len(names) - (1 if self_match else 0) <= 0 and len(from_list) > 0:
            raise ValueError("attempt to get argmax of an empty sequence")   # np.argmax([]) in the reference
        from ._rapidfuzz import best_choice_async, upload_for
        name = self._scorer_name              # "ratio": K4; the other rapidfuzz.fuzz scorers: K4 on transformed strings, or K7; Jaro: K8; Levenshtein / OSA: K9
        to_dev = None
        if not self_match:
            if reuse_to:
                to_dev = held[0]
            else:
                to_dev = upload_for(ctx, name, names)
            self._to_dev, self._to_names = to_dev, snap
        if top_n is not None:
            return choices(ctx, name, from_list, names, skip, self_match, to_dev, top_n), names
        return best_choice_async(ctx, name, from_list, names, skip, self_match, to_dev=to_dev), names

    # a matcher is pickled by joblib (reference _distance.py:77, polyfuzz.py:429-457): device handles stay behind
    def __getstate__(self):
        return {k: v for k, v in self.__dict__.items() if k not in ("_to_dev", "_to_names")}

    def __setstate__(self, state):
        self.__dict__.update(state)
        self._to_dev = self._to_names = None
