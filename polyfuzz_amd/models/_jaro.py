"""JaroWinkler -- jellyfish's Jaro / Jaro-Winkler similarity with all three questions answered on the device: the best match
(`match`: K8, through EditDistance), the n best choices (`match(top_n=, min_similarity=)`: K21), every pair at or above a score
(`join`: K20) and the clusters of that relation (`components`: K20).

"Jaro-Winkler >= 0.9" is the textbook rule of record linkage, and the scorer of the reference's custom-model tutorial
(docs/tutorial/models/models.md:46-58).  `EditDistance(scorer="jaro_winkler")` keeps refusing `join`, `components` and
`top_n > 1`; the threshold forms and the top-n live here, as RapidFuzz.top_n lives beside an EditDistance that refuses it.

Scores are K8's float64 on the scorer's own 0..1 scale, on code points, with jellyfish's default arguments (no
long_tolerance); `join` and the top-n report the very bits `match` would (csrc/k8_core.h jaro_score).
"""
import time
from typing import List

import numpy as np
import pandas as pd

from .. import _lib
from ._base import BaseMatcher
from ._distance import EditDistance
from ._distance import _TOP_N_MAX
from ._utils import gather_column, object_column


class JaroWinkler(BaseMatcher):
    """
    Jaro-Winkler (winkler=True, the default) or plain Jaro (winkler=False) similarity between lists of strings

    Arguments:
        winkler: True: jellyfish.jaro_winkler_similarity; False: jellyfish.jaro_similarity
        model_id: The name of the particular instance, used when comparing models
        normalize: `match` only, as EditDistance's (the reference's min-max rescaling of the Similarity column)

    match:      the best to-string of every from-string -- EditDistance(scorer="jaro_winkler" / "jaro").match, that matcher's
                frame and code path (K8); with the keywords top_n / min_similarity the n best choices at or above a score
                (K21), rapidfuzz.process.extract(..., limit=top_n, score_cutoff=min_similarity).  The count is a keyword of the
                call: the matcher has no attribute of that name.
    join:       every pair with score >= min_similarity, exact (K20).
    components: the connected components of the self-join's graph (K20); polyfuzz_amd.linkage.connected_components(strings,
                JaroWinkler(), 0.9) turns them into single_linkage's three dicts.
    """
    def __init__(self, winkler: bool = True, model_id: str = None, normalize: bool = True):
        super().__init__(model_id)
        self.type = "EditDistance"
        self.winkler = bool(winkler)
        self.normalize = normalize
        self._scorer_name = "jaro_winkler" if self.winkler else "jaro"
        self._best = EditDistance(scorer=self._scorer_name, model_id=model_id, normalize=normalize)

    def match(self, from_list: List[str], to_list: List[str] = None, top_n: int = 1, min_similarity: float = 0.0, **kwargs) -> pd.DataFrame:
        """ top_n == 1 and min_similarity == 0.0 (the defaults): the best match of every from-string,
        EditDistance(scorer=...).match, delegated with `kwargs` as they are.

        Otherwise (K21) the frame From, To, Similarity, To_2, Similarity_2, ... of EditDistance.top_n: per from-string its top_n
        best choices in the order np.argsort(-scores, kind="stable") gives -- float64 score descending, equal scores in list
        order --, exact, the scores K8's float64, unrounded.  top_n is clipped to the number of choices every row has (at least
        1); more than 64 after clipping raises _lib.PfzUnsupported.  A cell whose choice is missing, or scores below
        min_similarity (equal is kept), is None / 0.0.  At min_similarity == 0.0 the first pair of columns is the top_n = 1
        frame before normalisation.

        `normalize`: with min_similarity == 0.0 as EditDistance's top_n -- ONE minimum and maximum over all Similarity columns;
        with a cutoff it is NOT applied, by `join`'s rule: a rescaled score no longer means the threshold.

        to_list None: the self-match -- a from-string's own first occurrence is left out and nothing else, as EditDistance
        does.  re_train=False re-uses the resident to-list by EditDistance's rule; an empty set of choices raises what
        EditDistance raises.  top_n: an int >= 1, min_similarity: a number in [0, 1] (ValueError otherwise, before any device
        call). """
        if isinstance(top_n, bool) or not isinstance(top_n, (int, np.integer)) or top_n < 1:
            raise ValueError(f"top_n must be an int >= 1, not {top_n!r}")
        cutoff = _lib.check_min_similarity(min_similarity)
        self._best.normalize = self.normalize
        if top_n == 1 and cutoff == 0.0:
            matches = self._best.match(from_list, to_list, **kwargs)
            self.last_timings = getattr(self._best, "last_timings", None)
            return matches
        t0 = time.perf_counter()
        # every row has len(to_list) choices, or one less in a self-match (EditDistance._match_top_n's clip)
        ntop = max(1, min(int(top_n), (len(from_list) - 1) if to_list is None else len(to_list)))
        if ntop > _TOP_N_MAX:
            raise _lib.PfzUnsupported(-4, f"JaroWinkler.match: top_n = {ntop} exceeds the limit of {_TOP_N_MAX} best choices per from-string")

        def choices(ctx, name, from_list, names, skip, self_match, to_dev, ntop):
            f_dev = _lib.DeviceStrings.upload(ctx, from_list)
            return _lib.jaro_topn(ctx, f_dev, f_dev if self_match else to_dev, name, ntop, skip, score_cutoff=cutoff)
        (idx, score), names = self._best._best(from_list, to_list, reuse_to=kwargs.get("re_train", True) is False, top_n=ntop, choices=choices)
        t1 = time.perf_counter()
        data = {"From": object_column(from_list)}
        for r in range(ntop):      # (the kernel has applied the cutoff: a choice below it is no entry, index -1 -> None, score 0.0)
            data["To" if r == 0 else f"To_{r + 1}"] = gather_column(names, np.ascontiguousarray(idx[:, r]))
            data["Similarity" if r == 0 else f"Similarity_{r + 1}"] = score[:, r].copy()
        matches = pd.DataFrame(data, copy=False)
        if self.normalize and cutoff == 0.0 and score.size:      # EditDistance._match_top_n's: one minimum and one maximum
            lo, hi = score.min(), score.max()
            for r in range(ntop):
                c = "Similarity" if r == 0 else f"Similarity_{r + 1}"
                matches[c] = (matches[c] - lo) / (hi - lo)
        self.last_timings = {"device": (t1 - t0) * 1e3, "frame": (time.perf_counter() - t1) * 1e3}
        return matches

    def join(self,
             from_list: List[str],
             to_list: List[str] = None,
             min_similarity: float = 0.9) -> pd.DataFrame:
        """ Every pair at least `min_similarity` similar (K20): the frame From, To, Similarity with one row per pair, ordered by
        from-index, then to-index.  A from-string without a partner has no row.  Similarity is the scorer's own float64,
        unrounded, and a pair is kept iff that float64 is >= min_similarity (equal is kept).  Exact: every such pair is found,
        whatever their number.  An empty string scores 0.0 against everything, itself included.

        `normalize` is NOT applied: a rescaled score no longer means the threshold.

        to_list None: the self-join of from_list -- every unordered pair of positions i < j once, as From = from_list[i],
        To = from_list[j] (From is always the EARLIER position); never a string with itself, but equal strings at different
        positions are a pair.

        min_similarity: a number in [0, 1] (ValueError otherwise).  For the clusters of the self-join's graph see `components`,
        which never builds the frame. """
        t = _lib.check_min_similarity(min_similarity)
        t0 = time.perf_counter()
        ctx = _lib.Context.default()
        names = from_list if to_list is None else to_list
        f_dev = _lib.DeviceStrings.upload(ctx, from_list)
        t_dev = None if to_list is None else _lib.DeviceStrings.upload(ctx, to_list)
        row_ptr, idx, sim = _lib.jaro_join(ctx, f_dev, t_dev, self._scorer_name, t)
        t1 = time.perf_counter()
        frm = np.repeat(np.arange(len(from_list), dtype=np.int32), np.diff(row_ptr))
        matches = pd.DataFrame({"From": gather_column(from_list, frm), "To": gather_column(names, idx), "Similarity": sim}, copy=False)
        self.last_timings = {"device": (t1 - t0) * 1e3, "frame": (time.perf_counter() - t1) * 1e3}
        return matches

    def components(self,
                   from_list: List[str],
                   min_similarity: float = 0.9) -> np.ndarray:
        """ Near-duplicate clusters of from_list (K20): int32 labels, label[i] = the smallest position in i's connected component
        of the graph whose edges are the pairs `join(from_list, min_similarity=...)` reports -- "A ~ B and B ~ C put A, B and C
        together".  Equal non-empty strings share a component; a string with no partner is its own (label[i] == i).  Exact and
        deterministic.  The pairs are united on the device where they are found and never stored: device memory is
        O(len(from_list)) whatever their number.

        min_similarity: a number in [0, 1] (ValueError otherwise).  Sets last_timings and last_counts = {"pairs": hits,
        "components": components}. """
        t = _lib.check_min_similarity(min_similarity)
        t0 = time.perf_counter()
        if len(from_list) == 0:
            self.last_timings, self.last_counts = {"device": 0.0, "frame": 0.0}, {"pairs": 0, "components": 0}
            return np.empty(0, np.int32)
        ctx = _lib.Context.default()
        label, pairs, components = _lib.jaro_components(ctx, _lib.DeviceStrings.upload(ctx, from_list), self._scorer_name, t)
        self.last_timings = {"device": (time.perf_counter() - t0) * 1e3, "frame": 0.0}
        self.last_counts = {"pairs": pairs, "components": components}
        return label
