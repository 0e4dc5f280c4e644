"""GPU parity of K10 (pfz_pairs_rescore_topn) and of BlockedEditDistance: a device-resident candidate table scored under ratio /
Levenshtein / OSA / Jaro / Jaro-Winkler and re-ranked per row == np.argsort(-scores, kind="stable")[:ntop] over the row's valid
candidates taken in ascending index order, on the CPU oracles' scores (tests/lev_oracle.py; oracle/jaro.c; oracle/indel.c).  Every
comparison is == on int32 indices and on float64 scores; there is no tolerance."""
import contextlib

import numpy as np
import pandas as pd
import pytest

from tests import lev_oracle
from tests.test_levenshtein_gpu import _rand, _swapped

pytestmark = pytest.mark.gpu

FIVE = ("ratio", "levenshtein", "osa", "jaro", "jaro_winkler")


def all_scores(oracle_mod, fl, tl):
    """{scorer: float64 [len(fl), len(tl)]} of the five scorers, from the oracles"""
    out = {name: lev_oracle.sim_matrix(fl, tl, lev_oracle.matrix(fl, tl, name, workers=4)) for name in lev_oracle.SCORERS}
    out["ratio"] = oracle_mod.indel_argmax(fl, tl, want_matrix=True)[2]
    for name in ("jaro", "jaro_winkler"):
        out[name] = oracle_mod.jaro_matrix(fl, tl, name)
    return out


def expected(sim, cand, ntop):
    """(idx int32[n, ntop], score float64[n, ntop]) of candidate table `cand` (int [n, m], anything outside [0, n_to) skipped)"""
    n, n_to = cand.shape[0], sim.shape[1]
    idx, val = np.full((n, ntop), -1, np.int32), np.zeros((n, ntop))
    for i in range(n):
        js = np.unique(cand[i][(cand[i] >= 0) & (cand[i] < n_to)])          # ascending (and distinct: the table's contract)
        order = js[np.argsort(-sim[i, js], kind="stable")[:ntop]]
        idx[i, :len(order)], val[i, :len(order)] = order, sim[i, order]
    return idx, val


def random_table(rng, n, n_to, m):
    """int32 [n, m]: per row a random number (0 .. min(m, n_to); the first rows none, the next ones as many as fit) of distinct
    to-indices at random places, -1 / n_to / -7 everywhere else"""
    tab = rng.choice(np.array([-1, -1, n_to, -7], np.int32), size=(n, m))
    for i in range(n):
        k = 0 if i < 3 else (min(m, n_to) if i < 8 else int(rng.integers(0, min(m, n_to) + 1)))
        tab[i, rng.choice(m, k, replace=False)] = rng.choice(n_to, k, replace=False)
    return tab


def device_table(ctx, tab):
    from polyfuzz_amd import _lib
    return _lib.DeviceTopN.from_host(ctx, tab, np.zeros(tab.shape, np.float32))


def _assert_topn(got, want, what):
    idx, score = got
    assert idx.dtype == np.int32 and score.dtype == np.float64 and idx.shape == want[0].shape == score.shape, what
    np.testing.assert_array_equal(idx, want[0], err_msg=str(what))
    np.testing.assert_array_equal(score, want[1], err_msg=str(what))


@contextlib.contextmanager
def _k10_counters(ctx):
    """box["launches"] = timed K10 scopes (one per call with a register launch or a general one), box["general"] = launches of the
    general kernel"""
    box = {}
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        yield box
        ctx.sync()
        box["launches"] = ctx.prof_get("k10_pairs")[1]
        box["general"] = ctx.prof_get("k10_pairs_general")[1]
    finally:
        ctx.prof_enable(False)


# ---- 1. mixed shapes, all five scorers; 2. order independence ----------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed(golden, oracle_mod):
    """~120 x 250 on the recipe of test_edit_topn_gpu.py's `mixed`, every to-string present twice (the index decides)"""
    rng = np.random.default_rng(1001)
    t = golden["titles_lists"]
    edge = [31, 32, 33, 63, 64, 65]
    base = "the quick brown fox jumps over the lazy dog and runs far away from home again"
    cut = lambda: base[:int(rng.integers(24, 65))]
    fl = (t["from_list"][:16] + ["", "a", "ab", "CA", "the matrix", "Z"] + [base[:n] for n in edge] + [base[::-1][:n] for n in edge] +
          ["ab" * 100, "naïve café Ωmega \U0001f600 smile", "qqq中文", "####", "\U0001f600\U0001f601"] + _rand(rng, "ab", 1, 70, 30) +
          ["ab" * k for k in (1, 16, 17, 32, 33)] + ["abba" * 6, "baab" * 9] + _rand(rng, "abcdefgh ", 60, 66, 4) + _rand(rng, "abcdefgh ", 100, 200, 3) +
          [_swapped(rng, cut(), int(rng.integers(1, 6))) for _ in range(37)])
    uniq = (t["to_list"][:20] + ["", "a", "ba", "ABC", "the matrix", "The Matrix"] + [base[:n] for n in edge] + [base[3:3 + n] for n in edge] +
            ["ba" * 75, "naïve cafe Ωmega \U0001f601 smile \U0001f600", "中文qqq"] + [(base * 4)[:n] for n in (255, 256, 257)] + [(base * 14)[:1000]] +
            _rand(rng, "ab", 1, 70, 24) + ["ba" * k for k in range(1, 8)] + ["ab" * k + "ba" * k for k in range(1, 6)] +
            _rand(rng, "abcdefgh ", 60, 66, 5) + _rand(rng, "abc", 1, 9, 8) + [_swapped(rng, cut(), int(rng.integers(1, 6))) for _ in range(36)])
    tl = uniq + uniq[::-1]
    n, n_to = len(fl), len(tl)
    assert 110 <= n <= 130 and 230 <= n_to <= 270
    assert {0, 1, 31, 32, 33, 63, 64, 65, 200} <= set(map(len, fl)) and any(100 <= len(s) < 200 for s in fl)
    assert {0, 1, 255, 256, 257, 1000} <= set(map(len, tl))
    assert max(map(ord, "".join(tl))) > 0xFFFF and any(255 < ord(c) <= 0xFFFF for c in "".join(tl))
    tables = {m: random_table(rng, n, n_to, m) for m in (1, 5, 64, 65, 130)}
    return fl, tl, all_scores(oracle_mod, fl, tl), tables


@pytest.mark.parametrize("name", FIVE)
def test_mixed_shapes(ctx, mixed, name):
    """both word widths, Jaro's 256-character border (rows with and without a longer candidate), the general kernel, a second and
    a third chunk of 64 candidates, a full 64-entry list, ntop beyond the valid candidates of a row, rows without any"""
    from polyfuzz_amd import _lib
    fl, tl, sims, tables = mixed
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    lt = np.array([len(s) for s in tl])
    for m, tab in tables.items():
        valid = (tab >= 0) & (tab < len(tl))
        assert (valid[:3].sum(axis=1) == 0).all() and (valid[3:8].sum(axis=1) == m).all() and not valid.all()
        if m >= 64:      # Jaro: short from-rows with a candidate beyond 256 characters, and without one
            has_long = np.array([(lt[r[v]] > 256).any() for r, v in zip(tab, valid)])
            short = np.array([len(s) <= 64 for s in fl])
            assert (has_long & short).any() and (~has_long & short & (valid.sum(axis=1) > 0)).any()
        c = device_table(ctx, tab)
        for ntop in (1, 5, 64):
            with _k10_counters(ctx) as box:
                got = _lib.pairs_rescore_topn(ctx, f, t, c, name, ntop)
            _assert_topn(got, expected(sims[name], tab, ntop), (name, m, ntop))
            assert box["launches"] == 1 and box["general"] == 1          # (from-strings beyond 64 characters are in every call)
    full = expected(sims[name], tables[130], 64)[0]
    assert (full[3:8] >= 0).all() and (full[:3] == -1).all()               # a full 64-entry list; rows that are all -1
    assert (expected(sims[name], tables[5], 64)[0][:, 5:] == -1).all()     # ntop beyond what a row has


@pytest.mark.parametrize("name", FIVE)
def test_order_independence(ctx, mixed, name):
    from polyfuzz_amd import _lib
    fl, tl, sims, tables = mixed
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    rng = np.random.default_rng(1002)
    for m in (5, 65, 130):
        tab = tables[m]
        first = _lib.pairs_rescore_topn(ctx, f, t, device_table(ctx, tab), name, 5)
        for _ in range(2):
            perm = np.stack([row[rng.permutation(m)] for row in tab])
            assert (perm != tab).any()
            _assert_topn(_lib.pairs_rescore_topn(ctx, f, t, device_table(ctx, perm), name, 5), first, (name, m))


# ---- 3. agreement with the all-pairs kernels ---------------------------------------------------------------------------------

def test_agreement_with_the_all_pairs_kernels(ctx, mixed):
    """every row gets all n_to indices (in a shuffled order) as candidates: the result is the all-pairs kernels' own"""
    from polyfuzz_amd import _lib
    fl, tl, _, _ = mixed
    n, n_to = len(fl), len(tl)
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    rng = np.random.default_rng(1003)
    c = device_table(ctx, np.stack([rng.permutation(n_to).astype(np.int32) for _ in range(n)]))
    for ntop in (1, 5, 64):
        for name in ("levenshtein", "osa"):
            _assert_topn(_lib.pairs_rescore_topn(ctx, f, t, c, name, ntop), _lib.lev_topn(ctx, f, t, name, ntop), (name, ntop))
        _assert_topn(_lib.pairs_rescore_topn(ctx, f, t, c, "ratio", ntop), _lib.indel_topn(ctx, f, t, ntop), ("ratio", ntop))
    for name in ("jaro", "jaro_winkler"):
        idx, score = _lib.pairs_rescore_topn(ctx, f, t, c, name, 3)
        a_idx, a_score = _lib.jaro_argmax(ctx, f, t, name)
        np.testing.assert_array_equal(idx[:, 0], a_idx, err_msg=name)
        np.testing.assert_array_equal(score[:, 0], a_score, err_msg=name)


# ---- 4. an alphabet whose match table does not fit LDS ------------------------------------------------------------------------

def test_wide_alphabet_takes_the_general_kernel(ctx, oracle_mod):
    """8 000 distinct code points in the to-list: 64 KB of 64-bit table entries, beyond the 60 KiB budget -- every row is the general
    kernel's, short ones included"""
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(1004)
    wide = [chr(c) for c in range(0x4E00, 0x4E00 + 8000)]
    mk = lambda n, a: "".join(a[i] for i in rng.integers(0, len(a), n))
    uniq = ["".join(wide[k:k + 100]) for k in range(0, 8000, 100)] + [mk(int(n), wide[:12]) for n in rng.integers(0, 40, 20)]
    tl = uniq + uniq[::-1]
    fl = [mk(int(n), wide[:12]) for n in (0, 1, 20, 32, 33, 64, 65, 130)] + [s[::2] for s in uniq[:6]] + [uniq[3], uniq[85]]
    assert len(set("".join(tl))) == 8000 and (8000 + 1) * 8 > 60 * 1024
    sims = all_scores(oracle_mod, fl, tl)
    tab = random_table(rng, len(fl), len(tl), 70)
    f, t, c = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl), device_table(ctx, tab)
    for name in FIVE:
        with _k10_counters(ctx) as box:
            got = _lib.pairs_rescore_topn(ctx, f, t, c, name, 5)
        _assert_topn(got, expected(sims[name], tab, 5), name)
        assert box["launches"] == 1 and box["general"] == 1


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------

def test_entry_point_refuses_what_it_cannot_do(ctx):
    from polyfuzz_amd import _lib
    f = _lib.DeviceStrings.upload(ctx, ["ab", "b", "abc"])
    t = _lib.DeviceStrings.upload(ctx, ["a", "b"])
    c = device_table(ctx, np.array([[0, 1], [1, -1], [5, 0]], np.int32))
    idx, score = _lib.pairs_rescore_topn(ctx, f, t, c, "levenshtein", 3)
    assert idx.tolist() == [[0, 1, -1], [1, -1, -1], [0, -1, -1]] and score.tolist() == [[0.5, 0.5, 0.0], [1.0, 0.0, 0.0], [1 - 2 / 3, 0.0, 0.0]]
    for scorer, ntop in ((5, 1), (-1, 1), ("osa", 0), ("osa", -2)):
        with pytest.raises(_lib.PfzError) as e:
            _lib.pairs_rescore_topn(ctx, f, t, c, scorer, ntop)
        assert e.value.code == -1                                      # PFZ_ERR_INVALID
    with pytest.raises(_lib.PfzUnsupported, match="64"):
        _lib.pairs_rescore_topn(ctx, f, t, c, "jaro", 65)
    with pytest.raises(_lib.PfzUnsupported, match="1024"):
        _lib.pairs_rescore_topn(ctx, f, t, device_table(ctx, np.full((3, 1025), -1, np.int32)), "ratio", 1)
    idx, _ = _lib.pairs_rescore_topn(ctx, f, t, device_table(ctx, np.full((3, 1024), -1, np.int32)), "ratio", 2)
    assert (idx == -1).all()
    with pytest.raises(_lib.PfzError) as e:
        _lib.pairs_rescore_topn(ctx, f, t, device_table(ctx, np.zeros((2, 2), np.int32)), "ratio", 1)      # fewer rows than from-strings
    assert e.value.code == -1
    idx, score = _lib.pairs_rescore_topn(ctx, _lib.DeviceStrings.upload(ctx, []), t, c, "ratio", 3)       # n_from = 0
    assert idx.shape == (0, 3) and score.shape == (0, 3)


# ---- 6. the matcher -------------------------------------------------------------------------------------------------------------

def _want_frame(fl, names, idx, val, normalize):
    data = {"From": fl}
    for r in range(idx.shape[1]):
        data["To" if r == 0 else f"To_{r + 1}"] = [names[j] if j >= 0 else None for j in idx[:, r]]
        data["Similarity" if r == 0 else f"Similarity_{r + 1}"] = val[:, r]
    df = pd.DataFrame(data)
    if normalize:          # one minimum and one maximum over the cells that hold a choice; the empty ones stay 0.0
        held = idx >= 0
        lo, hi = val[held].min(), val[held].max()
        for r in range(idx.shape[1]):
            c = "Similarity" if r == 0 else f"Similarity_{r + 1}"
            df[c] = np.where(held[:, r], (val[:, r] - lo) / (hi - lo), 0.0)
    return df


def _assert_frame(df, want):
    assert list(df.columns) == list(want.columns) and len(df) == len(want)
    for c in want.columns:
        if c.startswith("Similarity"):
            assert df[c].dtype == np.float64
            np.testing.assert_array_equal(df[c].to_numpy(), want[c].to_numpy(), err_msg=c)
        else:
            assert df[c].tolist() == want[c].tolist(), c


@pytest.fixture(scope="module")
def titles(ctx, golden, oracle_mod):
    """303 from-strings x 500 to-titles, a second from-list, a self-match list of 400 -- with the oracles' scores and the candidate
    indices of an identically configured TFIDF.  (golden["titles_lists"] holds 300 from- and 291 to-titles: the lists of 500 and of
    400 are filled up from the other file of titles, golden["titles_self_list"], and from the from-titles.)"""
    from polyfuzz_amd.models import TFIDF
    t, s = golden["titles_lists"], golden["titles_self_list"]["from_list"]
    fl = t["from_list"][:300] + ["", "ab", "zzzqqqxxx"]
    tl = (t["to_list"] + s + t["from_list"][::-1])[:500]
    fl2 = t["from_list"][40:100] + s[:30] + ["q", "the"]
    dup = (t["to_list"] + s)[:400]
    assert len(fl) == 303 and len(tl) == 500 and len(dup) == 400
    tf = TFIDF(min_similarity=0.0, top_n=16)
    cand = tf.match_device(fl, tl).download()[0]
    cand2 = tf.match_device(fl2, tl, re_train=False).download()[0]
    cand_self = TFIDF(min_similarity=0.0, top_n=16).match_device(dup).download()[0]
    assert cand.shape == (303, 16) and cand_self.shape == (400, 16)
    assert (cand[300:302] == -1).all()                                     # "" and "ab" have no 3-gram: no candidate
    assert ((cand >= 0).sum(axis=1) == 0).any() and ((cand >= 0).sum(axis=1) == 16).any()
    assert (cand_self != np.arange(400)[:, None]).all()                      # a row's own index is never a candidate
    return {"fl": fl, "tl": tl, "fl2": fl2, "dup": dup, "cand": cand, "cand2": cand2, "cand_self": cand_self,
            "sims": all_scores(oracle_mod, fl, tl), "sims2": all_scores(oracle_mod, fl2, tl), "sims_self": all_scores(oracle_mod, dup, dup)}


@pytest.mark.parametrize("name", FIVE)
def test_matcher(ctx, titles, name):
    from polyfuzz_amd.models import BlockedEditDistance
    d = titles
    fl, tl, fl2, dup = d["fl"], d["tl"], d["fl2"], d["dup"]
    cols = ["From", "To", "Similarity", "To_2", "Similarity_2", "To_3", "Similarity_3"]
    for normalize in (False, True):
        m = BlockedEditDistance(scorer=name, candidates=16, top_n=3, normalize=normalize)
        df = m.match(fl, tl)
        assert list(df.columns) == cols
        _assert_frame(df, _want_frame(fl, tl, *expected(d["sims"][name], d["cand"], 3), normalize))
        assert df["To"][300] is None and df["Similarity"][300] == 0.0 and set(m.last_timings) == {"tfidf", "k10", "frame"}
        # re_train=False on a second from-list: the fitted TF-IDF side and the resident raw to-list serve again
        held = m._to_dev
        df = m.match(fl2, list(tl), re_train=False)
        assert m._to_dev is held
        _assert_frame(df, _want_frame(fl2, tl, *expected(d["sims2"][name], d["cand2"], 3), normalize))
        # a self-match
        df = BlockedEditDistance(scorer=name, candidates=16, top_n=3, normalize=normalize).match(dup)
        _assert_frame(df, _want_frame(dup, dup, *expected(d["sims_self"][name], d["cand_self"], 3), normalize))
