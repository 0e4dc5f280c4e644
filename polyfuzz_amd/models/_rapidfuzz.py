"""RapidFuzz -- the reference's `process.extractOne` matcher (polyfuzz/models/_rapidfuzz.py:10-113),
what `PolyFuzz("EditDistance")` dispatches to (polyfuzz.py:128-130), on the MI355X engine.

Same constructor and `.match()` contract: per from-string the best choice of the to-list under `scorer`
(first maximum, as rapidfuzz.process.extractOne keeps the first best), `None` / 0.0 when the best score is
below `score_cutoff`, Similarity = score / 100.

Scorers, all on the device (names or the rapidfuzz.fuzz functions of those names):
* `ratio`, `QRatio` (= ratio, but 0 when either string is empty), `token_sort_ratio` (= ratio of the strings'
  whitespace tokens sorted and joined by one space) -- one fixed string per list element: K4 (k4_indel.hip);
* `WRatio` (the reference's DEFAULT), `partial_ratio`, `token_set_ratio`, `token_ratio`, `partial_token_sort_ratio`,
  `partial_token_set_ratio`, `partial_token_ratio` -- a different string pair for every (from, to): K7
  (k7_fuzz.hip: windows by masked match tables and prefix bit counts, token-set differences by token masks).
rapidfuzz 3.x semantics: no default processor (strings are scored as given).  Any other callable raises
`NotImplementedError` (there is no CPU path in this package).
Strings of any length and token count are accepted; from-strings beyond 256 characters or 32 distinct tokens (and
to-strings beyond 32 distinct tokens) take K7's general kernel, which is slow.

Self-match.  The reference removes the from-string from ONE shared copy of the list (`to_list.remove(from_string)`,
_rapidfuzz.py:103-104), so with n_jobs=1 the list shrinks as rows are processed: row i is scored against the strings AFTER
it only, the last row against nothing.  By default a self-match here excludes only the first list element equal to the
from-string, for that from-string (the behaviour of EditDistance, _distance.py:93-96; SURVEY App. B calls the shrinking list
a bug).  `reference_self_match = True` (attribute, or keyword of `match`) reproduces the reference's frame instead -- on the
device: every choice up to and including the row itself is left out (skip codes, csrc/pfz_internal.h) -- held to frames of
the reference class itself (tests/golden/make_golden_rapidfuzz_self.py).

Threshold forms (K18, k18_fuzz_join.hip), under the seven K7 scorers: `join` -- every pair at least `min_similarity` similar, what
rapidfuzz.process.cdist(..., score_cutoff=c) keeps -- and `components` -- the clusters of that relation over one list.

Top-n (`top_n` attribute; K19, k19_fuzz_topn.hip): the n best choices of every from-string, rapidfuzz.process.extract(..., limit=n,
score_cutoff=c) -- K18's walk with the floor rising to the n-th best a wave holds; the K4 scorers through K4's own top-n.

PARITY UNPINNED: rapidfuzz is not installable in the build container; the scorer is the oracle's restatement
(oracle/indel.c), extractOne's tie / cut-off rules are restated from rapidfuzz's documentation.
"""
from typing import Callable, List, Union

import numpy as np
import pandas as pd

from .. import _lib
from ._base import BaseMatcher
from ._utils import gather_column, object_column, pair_frame, pair_frame_blocks

_K4_SCORERS = ("ratio", "QRatio", "token_sort_ratio")
_DEVICE_SCORERS = _K4_SCORERS + tuple(_lib.FUZZ_SCORERS)


def _scorer_name(scorer) -> str:
    """Name of the rapidfuzz.fuzz scorer `scorer` stands for; a callable from anywhere else (Levenshtein.ratio on
    its 0..1 scale, a user's own `ratio`) must not be mistaken for the rapidfuzz function of the same name."""
    if scorer is None:
        return "WRatio"                                   # the reference's default, fuzz.WRatio
    if isinstance(scorer, str):
        return scorer
    if "rapidfuzz" not in (getattr(scorer, "__module__", "") or ""):
        return repr(scorer)
    return getattr(scorer, "__name__", repr(scorer))


def _left_out(choice: int, skip: int) -> bool:
    """the skip codes of the best-choice kernels (csrc/pfz_internal.h: choice_left_out)"""
    return choice == skip or choice <= -2 - skip


def _transform(name, strings):
    """the string every list element is scored as: itself, or (token_sort_ratio) its whitespace tokens sorted and joined"""
    if name == "token_sort_ratio":           # rapidfuzz: ratio(" ".join(sorted(s1.split())), " ".join(sorted(s2.split())))
        return [" ".join(sorted(s.split())) for s in strings]
    return strings


def upload_for(ctx, name, strings):
    """A list resident on the device in the form scorer `name` reads (K4 scorers: one fixed string per element; K7 scorers:
    the strings themselves -- their token forms are built on the device and cached on the handle)."""
    return _lib.DeviceStrings.upload(ctx, _transform(name, strings))


class _PendingBest:
    """an enqueued best-choice pass: `result()` waits for the device and returns (index int32[n], score float64[n])"""

    def __init__(self, out, n, fix=None):
        self.out, self.n, self.fix = out, n, fix

    def result(self):
        idx, score = _lib.best_from_topn(*self.out.download())
        idx, score = idx[:self.n], score[:self.n]
        if self.fix is not None:
            self.fix(idx, score)
        return idx, score


def best_choice_async(ctx, name, from_list, names, skip, self_match, to_dev=None):
    """Enqueue the best-choice pass of every from-string under the rapidfuzz.fuzz (or K8 Jaro, K9 Levenshtein / OSA) scorer `name` and return at once (the
    caller builds its From column while the device works); `names` are the choices (the from-list itself in a
    self-match, where skip[i] is the choice left out for from-string i -- still the from-string's own first occurrence
    in the ORIGINAL list).  to_dev: the choices already resident (upload_for), e.g. from the previous call of a fitted
    matcher."""
    n = len(from_list)
    f_dev = upload_for(ctx, name, from_list)
    t_dev = f_dev if self_match else (to_dev if to_dev is not None else upload_for(ctx, name, names))
    out = _lib.DeviceTopN.alloc(ctx, max(n, 1), 2)
    fix = None
    if name in _lib.FUZZ_SCORERS:
        _lib.fuzz_extract_one_dev(ctx, f_dev, t_dev, name, out, skip)
    elif name in _lib.JARO_SCORERS:           # (EditDistance only: scores on jellyfish's 0..1 scale, not rapidfuzz's 0..100)
        _lib.jaro_argmax_dev(ctx, f_dev, t_dev, name, out, skip)
    elif name in _lib.LEV_SCORERS:            # (EditDistance only, K9: similarities on the 0..1 scale)
        _lib.lev_argmax_dev(ctx, f_dev, t_dev, name, out, skip)
    else:
        _lib.indel_argmax_dev(ctx, f_dev, t_dev, out, skip)
        if name == "QRatio":
            def fix(idx, score):
                # QRatio differs from ratio only when BOTH strings are empty (0 instead of 100): an empty from-string
                # scores 0 against every choice, so its first best is simply its first choice
                for i in [i for i, s in enumerate(from_list) if len(s) == 0]:
                    first_choice = next((j for j in range(len(names)) if not (skip is not None and _left_out(j, int(skip[i])))), -1)
                    idx[i], score[i] = first_choice, 0.0
        elif name == "indel":                 # (EditDistance only: K4's arg-max -- the order is the same --, its score on the 0..1 scale)
            def fix(idx, score):
                score[:] = indel_scores(from_list, names, idx, score)
    return _PendingBest(out, n, fix)


def indel_scores(from_list, names, idx, ratio):
    """K4's float64 ratios (0..100) of the pairs (from_list[i], names[idx[i, ...]]) as Indel.normalized_similarity (0..1): the
    integer LCS is recovered from each ratio and the two lengths (_lib.indel_lcs_of_ratio: verified bit for bit, ValueError
    otherwise) and put through the definition.  idx < 0 (no choice) keeps 0.0.  idx / ratio: [n] or [n, k]."""
    idx, ratio = np.asarray(idx), np.asarray(ratio, np.float64)
    la = np.fromiter(map(len, from_list), np.int64, len(from_list))
    lb = np.fromiter(map(len, names), np.int64, len(names))
    some = idx >= 0
    s = la.reshape((-1,) + (1,) * (idx.ndim - 1)) + lb[np.where(some, idx, 0)] if len(names) else np.zeros(idx.shape, np.int64)
    out = np.zeros(idx.shape, np.float64)
    out[some] = _lib.indel_similarity(_lib.indel_lcs_of_ratio(ratio[some], s[some]), s[some])
    return out


def best_choice(ctx, name, from_list, names, skip, self_match, to_dev=None):
    """(index of the first best choice int32[n], its score float64[n] on the 0..100 scale) of every from-string"""
    return best_choice_async(ctx, name, from_list, names, skip, self_match, to_dev).result()


class RapidFuzz(BaseMatcher):
    """
    Calculate the Edit Distance between lists of strings using RapidFuzz's process function

    Arguments (reference _rapidfuzz.py:17-38):
        n_jobs: accepted for compatibility; the GPU kernel ignores it
        score_cutoff: The minimum similarity for which to return a good match. Should be between 0 and 1.
        scorer: a rapidfuzz.fuzz scorer or its name; default (None) = fuzz.WRatio as in the reference.  Every
                rapidfuzz.fuzz scorer runs on the device; other callables raise NotImplementedError
        model_id: The name of the particular instance, used when comparing models

    Beyond the reference: `join` (every pair above a similarity) and `components` (the clusters of that relation), K18.

    top_n (attribute, default 1; the constructor keeps the reference's signature: `m = RapidFuzz(); m.top_n = 5`): the number of
    best choices per from-string -- rapidfuzz.process.extract(..., limit=top_n, score_cutoff=...) where the reference asks
    extractOne.  `match` then returns the columns To, Similarity, To_2, Similarity_2, ... in the order np.argsort(-scores,
    kind="stable") gives: score descending, equal scores in list order, exact, on the device, under all ten scorers (the seven
    per-pair scorers: K19; ratio / QRatio / token_sort_ratio: K4's top-n).  Similarity = score / 100; a cell whose choice is
    missing or scores below `score_cutoff` is None / 0.0.  top_n is clipped to the number of choices every row has (one less in
    a self-match); more than 64 after clipping raises _lib.PfzUnsupported before any device call.  An int >= 1, else
    ValueError; kept through pickling.  top_n = 1 is the frame and the code path it always was.
    """
    def __init__(self,
                 n_jobs: int = 1,
                 score_cutoff: float = 0,
                 scorer: Union[Callable, str, None] = None,
                 model_id: str = None):
        super().__init__(model_id)
        self.type = "EditDistance"
        self.score_cutoff = score_cutoff * 100
        name = _scorer_name(scorer)
        if name not in _DEVICE_SCORERS:
            raise NotImplementedError(
                f"polyfuzz_amd.RapidFuzz computes the rapidfuzz.fuzz scorers {_DEVICE_SCORERS} on the GPU; there is no "
                f"CPU path for an arbitrary scorer such as {name!r} -- use the reference's RapidFuzz matcher for it")
        self.scorer = scorer
        self._scorer_name = name
        self.n_jobs = n_jobs
        self.reference_self_match = False        # True: a self-match as the reference's shared, shrinking list gives it (n_jobs = 1)
        self._to_dev = self._to_names = None     # device copy (+ cached plan) of the last to-list
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
        """ Best choice of the to-list for every from-string (reference _rapidfuzz.py:61-113).

        The reference scores against the to_list it is handed, always (`PolyFuzz.transform` passes `self.to_list`,
        polyfuzz.py:234-240).  `re_train=False` only lets this matcher re-use what is resident: when the list it is handed IS
        the previous call's (the same object, or an equal list), its device copy, token forms and plan are used again -- no
        upload, no preparation.  Any other list is uploaded. """
        if self.top_n > 1:
            return self._match_top_n(from_list, to_list, **kwargs)
        ctx = _lib.Context.default()
        self_match = to_list is None
        # the resident copy stands for the list it was made from and for no other
        # -- compared by CONTENT against a snapshot taken when it was uploaded (the caller's list may have been changed
        # in place since; an ndarray / Series to-list has no list `==`)
        snap = None if self_match else tuple(to_list)
        reuse = kwargs.get("re_train", True) is False and not self_match and self._to_dev is not None and snap == self._to_names
        held = self._to_dev
        self._to_dev = self._to_names = None      # set again below, once this call's to-list is resident
        names = from_list if self_match else to_list
        n = len(from_list)
        skip = self._self_match_skip(from_list, kwargs) if self_match else None
        blocks = None
        if n == 0 or len(names) - (1 if self_match else 0) <= 0:
            idx, score = np.full(n, -1, np.int32), np.zeros(n)             # extractOne over no choices: None
            blocks = pair_frame_blocks(from_list)
        else:
            if not self_match:
                self._to_dev, self._to_names = (held if reuse else upload_for(ctx, self._scorer_name, names)), snap
            pending = best_choice_async(ctx, self._scorer_name, from_list, names, skip, self_match,
                                        to_dev=None if self_match else self._to_dev)
            blocks = pair_frame_blocks(from_list)                            # (the From column: host work while the device scores)
            idx, score = pending.result()
        hit = (idx >= 0) & (score >= self.score_cutoff)                       # extractOne: best score >= score_cutoff
        sim = np.where(hit, score / 100, 0.0)
        return pair_frame(from_list, names, idx, sim, keep=hit, blocks=blocks)

    def _self_match_skip(self, from_list, kwargs):
        """the skip codes of a self-match (csrc/pfz_internal.h), one per from-string"""
        n = len(from_list)
        if kwargs.get("reference_self_match", self.reference_self_match):
            # _rapidfuzz.py:86-104 with n_jobs = 1: when row i is scored, list.remove has taken the rows 0 .. i out of the shared
            # list (the first remaining element equal to from_list[i] is row i itself), and what is left keeps its order
            return (-2 - np.arange(n, dtype=np.int64)).astype(np.int32)
        first = {}
        for j, s in enumerate(from_list):
            first.setdefault(s, j)
        return np.fromiter((first[s] for s in from_list), np.int32, n)

    def _match_top_n(self, from_list, to_list=None, **kwargs):
        """the frame From, To, Similarity, To_2, Similarity_2, ... of the top_n best choices (class docstring); `match`'s rules for
        the self-match, reference_self_match and re_train=False"""
        from ._distance import _TOP_N_MAX, _top_n_choices
        self_match = to_list is None
        names = from_list if self_match else to_list
        n = len(from_list)
        # every row has len(to_list) choices, or one less in a self-match (reference _utils.py:55-56, applied to choices)
        ntop = max(1, min(self.top_n, len(names) - (1 if self_match else 0)))
        if ntop > _TOP_N_MAX:
            raise _lib.PfzUnsupported(-4, f"RapidFuzz.top_n = {ntop} exceeds the limit of {_TOP_N_MAX} best choices per from-string")
        snap = None if self_match else tuple(to_list)
        reuse = kwargs.get("re_train", True) is False and not self_match and self._to_dev is not None and snap == self._to_names
        held = self._to_dev
        self._to_dev = self._to_names = None      # set again below, once this call's to-list is resident
        skip = self._self_match_skip(from_list, kwargs) if self_match else None
        if n == 0 or len(names) - (1 if self_match else 0) <= 0:
            idx, score = np.full((n, ntop), -1, np.int32), np.zeros((n, ntop))             # extract over no choices: nothing
        else:
            ctx = _lib.Context.default()
            name = self._scorer_name
            if not self_match:
                self._to_dev, self._to_names = (held if reuse else upload_for(ctx, name, names)), snap
            if name in _lib.FUZZ_SCORERS:
                f_dev = upload_for(ctx, name, from_list)
                # the matcher's cut-off is the kernel's first floor (K19); the entry takes 0 .. 100 only, so one outside is clamped
                # for the kernel and `hit` below applies it as it is
                floor = min(max(float(self.score_cutoff), 0.0), 100.0) if self.score_cutoff == self.score_cutoff else 0.0
                idx, score = _lib.fuzz_topn(ctx, f_dev, f_dev if self_match else self._to_dev, name, ntop, skip, score_cutoff=floor)
            else:
                idx, score = _top_n_choices(ctx, name, from_list, names, skip, self_match, None if self_match else self._to_dev, ntop)
        hit = (idx >= 0) & (score >= self.score_cutoff)
        data = {"From": object_column(from_list)}
        for r in range(ntop):
            data["To" if r == 0 else f"To_{r + 1}"] = gather_column(names, np.ascontiguousarray(idx[:, r]), np.ascontiguousarray(hit[:, r]))
            data["Similarity" if r == 0 else f"Similarity_{r + 1}"] = np.where(hit[:, r], score[:, r] / 100, 0.0)
        return pd.DataFrame(data, copy=False)

    def _threshold_cutoff(self, what, min_similarity):
        """the checks of join / components, before any device call: the scorer has a threshold kernel, min_similarity is a number
        in [0, 1]; returns the cutoff on rapidfuzz's 0..100 scale -- the expression __init__ uses for score_cutoff"""
        if self._scorer_name not in _lib.FUZZ_SCORERS:
            raise NotImplementedError(
                f"RapidFuzz.{what} runs on the GPU for the scorers {tuple(_lib.FUZZ_SCORERS)}; scorer {self._scorer_name!r} is one "
                "fixed string per list element and has no threshold kernel here -- the same metric on the 0..1 scale is "
                'EditDistance(scorer="indel"), which has join and components')
        return _lib.check_min_similarity(min_similarity) * 100.0

    def join(self,
             from_list: List[str],
             to_list: List[str] = None,
             min_similarity: float = 0.8,
             **kwargs) -> pd.DataFrame:
        """ Every pair at least `min_similarity` similar under the matcher's scorer (K18): the frame From, To, Similarity with one
        row per pair, ordered by from-index, then to-index.  A from-string without a partner has no row.  A pair is kept iff its
        score -- the float64 `match` would report for it, on rapidfuzz's 0..100 scale -- is >= min_similarity * 100.0 (that
        product, in float64, is the cutoff; equal is kept: rapidfuzz's score_cutoff); Similarity = score / 100, unrounded.
        Exact: every such pair is found, whatever their number.  The constructor's `score_cutoff` plays no part.

        to_list None: the self-join of from_list -- every pair of positions i < j once, as From = from_list[i],
        To = from_list[j] (From is always the EARLIER position), scored as scorer(from_list[i], from_list[j]); never a string
        with itself, but equal strings at different positions are a pair like any other.  Equal strings do not always score
        100: WRatio("", "") is 0, and token_set_ratio, partial_token_set_ratio and partial_token_ratio of two strings without
        a token ("", "  ") are 0 -- such copies are no pair above min_similarity = 0.

        Under WRatio any two strings that share a token score at least 85.5 (100 * 0.95 * 0.9) when their lengths differ by a
        factor of 1.5 or more: min_similarity <= 0.855 joins everything that shares a word.

        `re_train=False` follows `match`'s rule: when to_list IS the previous call's (the same object, or an equal list), its
        device copy, token forms and plan are used again.

        The seven K7 scorers only (NotImplementedError under ratio / QRatio / token_sort_ratio); min_similarity: a number in
        [0, 1] (ValueError otherwise).  For the clusters of the self-join's graph see `components`, which never builds the
        frame. """
        cutoff = self._threshold_cutoff("join", min_similarity)
        self_join = to_list is None
        names = from_list if self_join else to_list
        snap = None if self_join else tuple(to_list)
        reuse = kwargs.get("re_train", True) is False and not self_join and self._to_dev is not None and snap == self._to_names
        held = self._to_dev
        self._to_dev = self._to_names = None      # set again below, once this call's to-list is resident
        if len(from_list) == 0 or len(names) == 0:
            return pd.DataFrame({"From": np.empty(0, object), "To": np.empty(0, object), "Similarity": np.empty(0, np.float64)})
        ctx = _lib.Context.default()
        f_dev = upload_for(ctx, self._scorer_name, from_list)
        if not self_join:
            self._to_dev, self._to_names = (held if reuse else upload_for(ctx, self._scorer_name, names)), snap
        row_ptr, idx, score = _lib.fuzz_join(ctx, f_dev, None if self_join else self._to_dev, self._scorer_name, cutoff)
        frm = np.repeat(np.arange(len(from_list), dtype=np.int32), np.diff(row_ptr))
        return pd.DataFrame({"From": gather_column(from_list, frm), "To": gather_column(names, idx), "Similarity": score / 100},
                            copy=False)

    def components(self,
                   strings: List[str],
                   min_similarity: float = 0.8) -> np.ndarray:
        """ Near-duplicate clusters of `strings` under the matcher's scorer (K18): int32 labels, label[i] = the smallest position
        in i's connected component of the graph whose edges are the pairs `join(strings, min_similarity=...)` reports (the
        self-join: From is the earlier position, To the later) -- "A ~ B and B ~ C put A, B and C together".  A string with no
        partner is its own component (label[i] == i).  Exact and deterministic.  The pairs are united on the device where they are
        found and never stored: device memory is O(len(strings)) whatever their number.
        polyfuzz_amd.linkage.connected_components turns the labels into the three dicts single_linkage returns.

        Equal strings share a component whenever they have a token (they score 100); empty or token-less copies score 0 under
        WRatio and the token-set scorers (see `join`) and stay apart above min_similarity = 0.  Under WRatio two strings that share a token score
        at least 85.5 (100 * 0.95 * 0.9) when their lengths differ by a factor of 1.5 or more: min_similarity <= 0.855 chains
        together everything that shares a word.

        The seven K7 scorers only (NotImplementedError otherwise); min_similarity: a number in [0, 1] (ValueError otherwise). """
        cutoff = self._threshold_cutoff("components", min_similarity)
        if len(strings) == 0:
            return np.empty(0, np.int32)
        ctx = _lib.Context.default()
        label, pairs, components = _lib.fuzz_components(ctx, upload_for(ctx, self._scorer_name, strings), self._scorer_name, cutoff)
        self.last_counts = {"pairs": pairs, "components": components}
        return label

    # a matcher is pickled by joblib (reference polyfuzz.py:429-457): device handles stay behind
    def __getstate__(self):
        return {k: v for k, v in self.__dict__.items() if k not in ("_to_dev", "_to_names")}

    def __setstate__(self, state):
        self.__dict__.update(state)
        self.__dict__.setdefault("reference_self_match", False)      # (a matcher pickled before the attribute existed)
        self._to_dev = self._to_names = None
