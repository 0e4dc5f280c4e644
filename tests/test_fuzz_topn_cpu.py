"""K19 -- the n best choices under K7's scorers (RapidFuzz.top_n, _lib.fuzz_topn) -- without a GPU:
  * a RISING floor loses no choice: k7_core.h's fz_score and fz_upper_bound (compiled for the host by tests/k7_core_host.cpp) with
    the floor the kernel hands them -- the score of the n-th best so far, the cutoff before -- in three orders of the walk,
    against oracle/fuzz_scorers.c stably sorted; and the same walk with its floor tests at <= loses ties;
  * the matcher's surface with the device unreachable;
  * the C entry's declaration and the ctypes wrapper."""
import bisect
import os
import pickle
import re
from types import SimpleNamespace

import numpy as np
import pytest

from polyfuzz_amd import _lib
from polyfuzz_amd._lib import fuzz_topn          # (K19's wrapper: this module is about nothing else)
from tests import k7_prep
from tests.test_k7_core_cpu import MODES, SLACK, _lists, host, run_pairs      # noqa: F401  (host: the fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
BATCH = 8             # pairs bounded and scored against one reading of the floor (the kernel: up to 64)


def _rows(L, lo, hi):
    """rows [lo, hi) of a prepared list (tests/k7_prep.py): the offsets are absolute, so views do"""
    return {"n": hi - lo, "sym": L["sym"], "off": [o[lo:hi + 1] for o in L["off"]], "tag": L["tag"], "tok_off": L["tok_off"][lo:hi + 1],
            "tok_id": L["tok_id"], "tok_len": L["tok_len"], "hist": L["hist"][lo:hi], "usum": L["usum"][lo:hi], "pres": L["pres"][lo:hi]}


def _walk(lib, alpha, A, i, B_in_order, order, mode, ntop, cutoff=0.0, broken=False):
    """k7_join_kernel's walk of row i with the top-n sink, on the host: the choices in `order` (B_in_order is the to-list prepared
    in that order), BATCH at a time -- the floor read once per batch, every pair bounded (fz_upper_bound, K7's slack, the float32
    compare of fuzz_join_go) and the survivors scored by fz_score AT THAT FLOOR, offered iff score >= cutoff and inserted by
    (score descending, index ascending).  broken: both floor tests at <= -- a pair that can only tie the n-th best is dropped."""
    best = []                                              # (-score, index), sorted: the list of topn_wave.h
    row = _rows(A, i, i + 1)
    for k in range(0, len(order), BATCH):
        full = len(best) >= ntop
        floor = max(cutoff, -best[ntop - 1][0]) if full else cutoff
        score, ub = run_pairs(lib, 1, alpha, row, _rows(B_in_order, k, min(k + BATCH, len(order))), mode, np.array([floor]))
        for t in range(score.shape[1]):
            bound = np.float32(ub[0, t]) + np.float32(SLACK)
            if bound <= np.float32(floor) if broken else bound < np.float32(floor):
                continue
            s = float(score[0, t])
            if s < cutoff or (broken and full and s <= floor):
                continue
            bisect.insort(best, (-s, int(order[k + t])))
            del best[ntop:]
    return [j for _, j in best], [-s for s, _ in best]


def _orders(tl, seed):
    n = len(tl)
    return {"index": np.arange(n), "length": np.argsort([len(s) for s in tl], kind="stable")[::-1],
            "shuffle": np.random.default_rng(seed).permutation(n)}


def _expect(truth_row, ntop, cutoff=0.0):
    cand = np.nonzero(truth_row >= cutoff)[0]
    order = cand[np.argsort(-truth_row[cand], kind="stable")][:ntop]
    return order.tolist(), truth_row[order].tolist()


@pytest.mark.parametrize("mode", MODES)
def test_a_rising_floor_loses_no_choice(host, oracle_mod, mode):     # noqa: F811
    """40 x 120 seeded strings, ntop 1 / 5 / 64, the pairs of a row in index order, longest first (ties of a length class met in
    DESCENDING index) and shuffled: the final list is the stable argsort of the oracle's row -- indices and score bits"""
    fl, tl = _lists(31, 40, 120)
    fl = [s for s in fl if len(s) <= 64 and len(set(s.split())) <= 32]
    alpha = k7_prep.Alphabet(tl)
    A = k7_prep.prepare(fl, alpha, False)
    truth = oracle_mod.fuzz_matrix(fl, tl, mode)
    for name, order in _orders(tl, 5).items():
        B = k7_prep.prepare([tl[j] for j in order], alpha, True)
        for ntop in (1, 5, 64):
            for i in range(len(fl)):
                assert _walk(host, alpha, A, i, B, order, mode, ntop) == _expect(truth[i], ntop), (mode, name, ntop, i)
    # the caller's cutoff as the first floor, an attained score (equal is kept)
    cutoff = float(np.unique(truth)[-3])
    order = _orders(tl, 5)["shuffle"]
    B = k7_prep.prepare([tl[j] for j in order], alpha, True)
    for i in range(len(fl)):
        assert _walk(host, alpha, A, i, B, order, mode, 5, cutoff) == _expect(truth[i], 5, cutoff), (mode, "cutoff", i)


def test_a_floor_test_at_le_loses_ties(host, oracle_mod):     # noqa: F811
    """200 to-strings drawn from 5 distinct ones, shuffled: equal scores are met out of index order.  The walk as it is gives the
    oracle's lists; with its floor tests at <= a copy of lower index that arrives once the list is full is dropped, and at least
    one row differs -- what holds the kernel's `<` and topn_insert's (score, index) compare in place."""
    base = ["a", "new york mets", "atlanta braves vs", "los angeles dodgers inc", "red sox vs yankees the boston"]
    rng = np.random.default_rng(19)
    tl = [base[k] for k in rng.integers(0, 5, 200)]
    fl = base + ["boston celtics", "zzz"]
    alpha = k7_prep.Alphabet(tl)
    A = k7_prep.prepare(fl, alpha, False)
    order = _orders(tl, 23)["shuffle"]
    B = k7_prep.prepare([tl[j] for j in order], alpha, True)
    for mode in ("WRatio", "token_set_ratio", "partial_ratio"):
        truth = oracle_mod.fuzz_matrix(fl, tl, mode)
        differ = 0
        for ntop in (3, 40, 64):
            for i in range(len(fl)):
                want = _expect(truth[i], ntop)
                assert _walk(host, alpha, A, i, B, order, mode, ntop) == want, (mode, ntop, i)
                differ += _walk(host, alpha, A, i, B, order, mode, ntop, broken=True) != want
        assert differ >= 1, mode


# ---- the matcher's surface, the device unreachable ----------------------------------------------------------------------------

@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a device call before the arguments were checked")
    monkeypatch.setattr(_lib.Context, "default", staticmethod(refuse))


@pytest.mark.parametrize("bad", [0, -1, 1.0, 2.5, "3", None, True, False, [2], float("nan")], ids=repr)
def test_top_n_must_be_a_positive_int(no_device, bad):
    from polyfuzz_amd.models import RapidFuzz
    m = RapidFuzz()
    assert m.top_n == 1
    with pytest.raises(ValueError, match="top_n"):
        m.top_n = bad
    assert m.top_n == 1
    m.top_n = np.int64(7)
    assert m.top_n == 7 and type(m.top_n) is int


def test_top_n_survives_pickling(no_device):
    from polyfuzz_amd.models import RapidFuzz
    m = RapidFuzz(scorer="partial_ratio", score_cutoff=0.4)
    m.top_n = 5
    m._to_dev, m._to_names = object(), ("a",)                     # (device handles stay behind)
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.top_n == 5 and m2._scorer_name == "partial_ratio" and m2.score_cutoff == 40 and m2._to_dev is None
    old = RapidFuzz.__new__(RapidFuzz)
    old.__setstate__({k: v for k, v in m.__getstate__().items() if k != "_top_n"})      # a matcher pickled before the attribute existed
    assert old.top_n == 1
    assert "top_n" in RapidFuzz.__doc__ and "process.extract" in RapidFuzz.__doc__


def test_more_than_64_columns_is_refused_before_any_device_call(no_device):
    from polyfuzz_amd.models import RapidFuzz
    names = [f"name {k}" for k in range(70)]
    for scorer in ("WRatio", "ratio"):
        m = RapidFuzz(scorer=scorer)
        m.top_n = 65
        for call in (lambda: m.match(["a"], names), lambda: m.match(names[:66])):                # 65 choices after clipping
            with pytest.raises(_lib.PfzUnsupported, match="64"):
                call()
        # clipped to the list's size -- 64 choices, a self-match has one fewer -- the check passes and the device is next
        for call in (lambda: m.match(["a"], names[:64]), lambda: m.match(names[:65])):
            with pytest.raises(AssertionError, match="a device call"):
                call()
        m.top_n = 1000
        with pytest.raises(AssertionError, match="a device call"):
            m.match(["a"], names[:10])


def test_empty_lists_need_no_device(no_device):
    from polyfuzz_amd.models import RapidFuzz
    m = RapidFuzz()
    m.top_n = 3
    df = m.match([], ["a", "b", "c"])
    assert list(df.columns) == ["From", "To", "Similarity", "To_2", "Similarity_2", "To_3", "Similarity_3"] and len(df) == 0
    df = m.match(["a", "b"], [])
    assert list(df.columns) == ["From", "To", "Similarity"] and df["To"].isna().all() and (df["Similarity"] == 0.0).all()
    df = m.match(["a"])                                             # a self-match of one string has no choice
    assert list(df.columns) == ["From", "To", "Similarity"] and df["To"].tolist() == [None]


# ---- the C entry and its wrapper ----------------------------------------------------------------------------------------------

def test_the_entry_is_declared_with_its_argument_checks():
    assert len(_lib.SIGNATURES["pfz_fuzz_topn"][1]) == 12
    header = open(os.path.join(REPO, "include", "polyfuzz_hip.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int pfz_fuzz_topn\(", header, flags=re.S)
    assert m, "pfz_fuzz_topn is not declared behind a comment of its own"
    doc = " ".join(m.group(1).split())
    for words in ("ntop < 1", "NaN score_cutoff", "outside [0, 100]", "PFZ_ERR_INVALID", "ntop > 64", "PFZ_ERR_UNSUPPORTED", "-1 / 0.0",
                  "Blocks", "equal is kept", "ascending to-index", "pfz_fuzz_extract_one"):
        assert words in doc, words


def test_the_wrapper_passes_its_arguments_in_the_entry_s_order():
    calls = []

    def entry(*args):
        calls.append(args)
        return 0
    ctx = SimpleNamespace(lib=SimpleNamespace(pfz_fuzz_topn=entry), h="ctx")
    f, t = SimpleNamespace(h="from", n=4), SimpleNamespace(h="to", n=9)
    idx, score = fuzz_topn(ctx, f, t, "partial_ratio", 5)
    assert idx.shape == score.shape == (4, 5) and idx.dtype == np.int32 and score.dtype == np.float64
    assert calls[0][:9] == ("ctx", "from", "to", _lib.FUZZ_SCORERS["partial_ratio"], None, 0, 4, 5, 0.0) and calls[0][11] is None
    out = fuzz_topn(ctx, f, t, "WRatio", 2, np.array([0, 1, 2, 3]), score_cutoff=85.5, begin=1, end=3, counters=True)
    assert out[0].shape == (2, 2) and out[2] == {"bounded": 0, "scored": 0, "steps": 0} and list(out[2]) == list(_lib.FUZZ_JOIN_COUNTERS)
    assert calls[1][3] == 0 and calls[1][4] is not None and calls[1][5:9] == (1, 3, 2, 85.5) and calls[1][11] is not None
    with pytest.raises(ValueError):
        fuzz_topn(ctx, f, t, "WRatio", 2, np.array([0, 1]))
