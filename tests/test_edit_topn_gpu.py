"""GPU parity of the top-n forms of K9 (Levenshtein / OSA) and K4 (ratio) and of EditDistance.top_n: the ntop best choices of every
from-string == np.argsort(-sim, kind="stable")[:ntop] on the CPU oracles' scores (tests/lev_oracle.py; oracle/indel.c) after the
left-out choices are masked.  Every comparison is == on int32 indices and on float64 scores; there is no tolerance."""
import numpy as np
import pandas as pd
import pytest

from tests import lev_oracle
from tests.test_levenshtein_gpu import _first_occurrence, _k9_counters, _rand, _skip_forms, _swapped, pruning_lists

pytestmark = pytest.mark.gpu

SCORERS = lev_oracle.SCORERS


def expected_topn(sim, ntop, skip=None):
    """(idx int32[n, ntop], score float64[n, ntop]): the stable descending sort of every row of `sim` over the choices `skip` leaves
    in (the skip codes of the best-choice kernels); -1 / 0.0 beyond them"""
    n, n_to = sim.shape
    idx, val = np.full((n, ntop), -1, np.int32), np.zeros((n, ntop))
    if n_to == 0:
        return idx, val
    out = np.zeros(sim.shape, bool) if skip is None else lev_oracle.left_out(n_to, skip)
    masked = np.where(out, -1.0, sim)                                    # (scores are >= 0: the left-out ones sort last)
    order = np.argsort(-masked, axis=1, kind="stable")[:, :ntop]
    ok = ~np.take_along_axis(out, order, axis=1)
    k = order.shape[1]
    idx[:, :k] = np.where(ok, order, -1)
    val[:, :k] = np.where(ok, np.take_along_axis(sim, order, axis=1), 0.0)
    return idx, val


def _assert_topn(got, want, what):
    idx, score = got
    assert idx.dtype == np.int32 and score.dtype == np.float64 and idx.shape == want[0].shape == score.shape, what
    np.testing.assert_array_equal(idx, want[0], err_msg=str(what))
    np.testing.assert_array_equal(score, want[1], err_msg=str(what))


def _three_skips(rng, plain_idx, n, n_to, up_to_range):
    one, up_to = _skip_forms(rng, plain_idx, n, n_to, up_to_range)
    return (("no skip", None), ("one choice", one), ("up to", up_to))


# ---- 1. mixed, K9 --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed(golden):
    """~120 x 250 on the recipe of test_levenshtein_gpu.py's `mixed`, every to-string present twice (the index decides)"""
    rng = np.random.default_rng(193)
    t = golden["titles_lists"]
    edge = [31, 32, 33, 63, 64, 65]
    base = "the quick brown fox jumps over the lazy dog and runs far away from home again"
    cut = lambda: base[:int(rng.integers(24, 65))]
    fl = (t["from_list"][:16] + ["", "a", "ab", "CA", "the matrix", "Z"] + [base[:n] for n in edge] + [base[::-1][:n] for n in edge] +
          ["ab" * 100, "naïve café Ωmega \U0001f600 smile", "qqq中文", "####", "\U0001f600\U0001f601"] + _rand(rng, "ab", 1, 70, 30) +
          ["ab" * k for k in (1, 16, 17, 32, 33)] + ["abba" * 6, "baab" * 9] + _rand(rng, "abcdefgh ", 60, 66, 4) +
          [_swapped(rng, cut(), int(rng.integers(1, 6))) for _ in range(40)])
    uniq = (t["to_list"][:20] + ["", "a", "ba", "ABC", "the matrix", "The Matrix"] + [base[:n] for n in edge] + [base[3:3 + n] for n in edge] +
            ["ba" * 75, "naïve cafe Ωmega \U0001f601 smile \U0001f600", "中文qqq"] + [(base * 4)[:n] for n in (255, 256, 257)] + [(base * 14)[:1000]] +
            _rand(rng, "ab", 1, 70, 24) + ["ba" * k for k in range(1, 8)] + ["ab" * k + "ba" * k for k in range(1, 6)] +
            _rand(rng, "abcdefgh ", 60, 66, 5) + _rand(rng, "abc", 1, 9, 8) + [_swapped(rng, cut(), int(rng.integers(1, 6))) for _ in range(36)])
    tl = uniq + uniq[::-1]
    return fl, tl, {name: lev_oracle.sim_matrix(fl, tl, lev_oracle.matrix(fl, tl, name)) for name in SCORERS}


def test_lev_topn_mixed(ctx, mixed):
    from polyfuzz_amd import _lib
    fl, tl, sims = mixed
    n, n_to = len(fl), len(tl)
    assert 110 <= n <= 130 and 230 <= n_to <= 270
    assert {0, 1, 31, 32, 33, 63, 64, 65, 200} <= set(map(len, fl)) and {0, 1, 255, 256, 257, 1000} <= set(map(len, tl))
    assert max(map(ord, "".join(tl))) > 0xFFFF and any(255 < ord(c) <= 0xFFFF for c in "".join(tl))
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    rng = np.random.default_rng(194)
    for name in SCORERS:
        sim = sims[name]
        plain = lev_oracle.argmax(sim)
        assert (plain[0] < n_to // 2).all()                           # (every best has a later twin: ties did occur)
        skips = _three_skips(rng, plain[0], n, n_to, n_to - 1)
        assert (expected_topn(sim, 5, skips[2][1])[0][-3:] == -1).all()      # the last rows keep no choice at all
        for what, skip in skips:
            a_idx, a_score = _lib.lev_argmax(ctx, f, t, name, skip)
            for ntop in (1, 2, 5, 64):
                got = _lib.lev_topn(ctx, f, t, name, ntop, skip)
                _assert_topn(got, expected_topn(sim, ntop, skip), (name, what, ntop))
                np.testing.assert_array_equal(got[0][:, 0], a_idx)
                np.testing.assert_array_equal(got[1][:, 0], a_score)
        _assert_topn(_lib.lev_topn(ctx, f, t, name, 5, None, 30, 61), [a[30:61] for a in expected_topn(sim, 5)], (name, "row shard"))


# ---- 2. fewer choices than ntop; the entry points' refusals -----------------------------------------------------------------

def test_fewer_choices_than_ntop(ctx, oracle_mod):
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(195)
    fl = _rand(rng, "abc", 0, 12, 9) + ["", "abc" * 30]
    for tl, ntop, skip in ((["abc", "", "abcb"], 5, None),
                           (_rand(rng, "abc", 0, 12, 70), 64, np.full(len(fl), -2 - 59, np.int32))):      # up to 59: ten choices left
        f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
        left = len(tl) if skip is None else 10
        for name in SCORERS:
            want = expected_topn(lev_oracle.sim_matrix(fl, tl, lev_oracle.matrix(fl, tl, name)), ntop, skip)
            assert (want[0][:, :left] >= 0).all() and (want[0][:, left:] == -1).all() and (want[1][:, left:] == 0.0).all()
            _assert_topn(_lib.lev_topn(ctx, f, t, name, ntop, skip), want, (name, len(tl), ntop))
        mat = oracle_mod.indel_argmax(fl, tl, want_matrix=True)[2]
        _assert_topn(_lib.indel_topn(ctx, f, t, ntop, skip), expected_topn(mat, ntop, skip), ("ratio", len(tl), ntop))


def test_entry_points_refuse_what_they_cannot_do(ctx):
    from polyfuzz_amd import _lib
    f = _lib.DeviceStrings.upload(ctx, ["a", "b"])
    for call in (lambda k: _lib.lev_topn(ctx, f, f, "osa", k), lambda k: _lib.indel_topn(ctx, f, f, k)):
        for bad in (0, -3):
            with pytest.raises(_lib.PfzError) as e:
                call(bad)
            assert e.value.code == -1                                      # PFZ_ERR_INVALID
        with pytest.raises(_lib.PfzUnsupported, match="64"):
            call(65)
    idx, score = _lib.lev_topn(ctx, f, f, "levenshtein", 3, None, 1, 1)         # an empty row range
    assert idx.shape == (0, 3) and score.shape == (0, 3)
    idx, score = _lib.indel_topn(ctx, f, f, 3, None, 2, 2)
    assert idx.shape == (0, 3)
    with pytest.raises(_lib.PfzError):
        _lib.lev_topn(ctx, f, f, "osa", 2, np.array([1, -5], np.int32))         # both skip forms in one call


# ---- 3. pruning, K9 ------------------------------------------------------------------------------------------------------

def test_lev_topn_pruning_by_the_length_bound(ctx):
    """100 x 2 048, lengths 1 .. 120, every to-string twice: the threshold is the ntop-th best, so ntop = 1 and 5 must leave pairs
    unwalked and ntop = 64 may.  The expected distances of this shape come from _lib.lev_matrix, the entry that walks every pair
    (test_levenshtein_gpu.py holds it to the oracle).  Then to-strings of ONE length: no bound is strictly below a score, every
    pair is walked."""
    from polyfuzz_amd import _lib
    fl, tl = pruning_lists()
    # (every string is there an even number of times: every other one of the sorted list is the list of originals; and of those,
    # sorted by length, every other one keeps every length)
    uniq = sorted(sorted(tl)[::2], key=len)[::2]
    rng = np.random.default_rng(196)
    tl = uniq + uniq
    tl = [tl[k] for k in rng.permutation(len(tl))]
    fl = fl[:100]
    n, n_to = len(fl), len(tl)
    lt = np.array([len(s) for s in tl])
    assert n == 100 and n_to == 2048 and set(lt) == set(range(1, 121)) and all(tl.count(s) >= 2 for s in tl[:50])
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    sim = lev_oracle.sim_matrix(fl, tl, _lib.lev_matrix(ctx, f, t, "levenshtein"))
    for what, skip in _three_skips(rng, lev_oracle.argmax(sim)[0], n, n_to, 512):
        for ntop in (1, 5, 64):
            with _k9_counters(ctx) as box:
                got = _lib.lev_topn(ctx, f, t, "levenshtein", ntop, skip)
            print(f"K9 top-n pruning levenshtein {what} ntop {ntop}: {box['walked']} of {n * n_to} pairs walked, share {box['walked'] / (n * n_to):.4f}")
            _assert_topn(got, expected_topn(sim, ntop, skip), (what, ntop))
            assert box["launches"] == 1
            if ntop in (1, 5):
                assert box["walked"] < n * n_to, (what, ntop)
    same = ([s for s in tl if len(s) == 40] * 40)[:256]
    from_40 = [s[:40] for s in fl]
    assert len(same) == 256
    f, t = _lib.DeviceStrings.upload(ctx, from_40), _lib.DeviceStrings.upload(ctx, same)
    for name in SCORERS:
        sim1 = lev_oracle.sim_matrix(from_40, same, lev_oracle.matrix(from_40, same, name))
        with _k9_counters(ctx) as box:
            got = _lib.lev_topn(ctx, f, t, name, 5)
        _assert_topn(got, expected_topn(sim1, 5), name)
        assert box["walked"] == n * 256, name


# ---- 4. parts ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def few_rows():
    """3 from-strings (one per K9 class: <= 32, <= 64, beyond) x 4 096 to-strings, every one of them twice"""
    _, tl = pruning_lists()
    big = "".join(tl[:40])
    fl = [big[:20], big[30:80], big[100:200]]
    assert [len(s) for s in fl] == [20, 50, 100] and len(tl) == 4096
    return fl, tl


def test_lev_topn_few_rows_split_over_workgroups(ctx, few_rows):
    from polyfuzz_amd import _lib
    fl, tl = few_rows
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for name in SCORERS:
        sim = lev_oracle.sim_matrix(fl, tl, lev_oracle.matrix(fl, tl, name))
        for ntop in (5, 64):
            _assert_topn(_lib.lev_topn(ctx, f, t, name, ntop), expected_topn(sim, ntop), (name, ntop))


@pytest.mark.parametrize("parts", [None, "5"])
def test_indel_topn_few_rows_split_over_workgroups(ctx, oracle_mod, few_rows, monkeypatch, parts):
    from polyfuzz_amd import _lib
    fl, tl = few_rows
    if parts:
        monkeypatch.setenv("PFZ_K4_PARTS", parts)
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    mat = oracle_mod.indel_argmax(fl, tl, want_matrix=True)[2]
    for ntop in (5, 64):
        _assert_topn(_lib.indel_topn(ctx, f, t, ntop), expected_topn(mat, ntop), (parts, ntop))


# ---- 5. mixed, ratio -----------------------------------------------------------------------------------------------------

RATIO_FROM_LENGTHS = [0, 1, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025]


@pytest.fixture(scope="module")
def ratio_lists(oracle_mod):
    rng = np.random.default_rng(197)
    alpha = "abcdefgh "
    mk = lambda n, a=alpha: "".join(a[i] for i in rng.integers(0, len(a), n))
    fl = [mk(n) for n in RATIO_FROM_LENGTHS] + [mk(int(n)) for n in rng.integers(2, 40, 14)]
    uniq = [mk(int(n)) for n in [0, 1, 3, 17, 32, 64, 100, 130, 300, 600, 1500] + list(rng.integers(1, 40, 89))]
    tl = uniq + uniq[::-1]
    wide = "".join(chr(c) for c in list(range(0x4E00, 0x4E00 + 400)) + list(range(0x41, 0x5B)))
    uniq16 = [mk(int(n), wide) for n in rng.integers(0, 50, 75)] + [mk(n, wide) for n in (33, 70, 130)]
    fl16 = [mk(n, wide) for n in (0, 1, 16, 17, 32, 33, 64, 65, 128, 129)] + uniq16[:6]
    tl16 = uniq16 + uniq16[::-1]
    assert len(set("".join(tl16))) > 255
    return {"narrow": (fl, tl, oracle_mod.indel_argmax(fl, tl, want_matrix=True)[2]),
            "wide": (fl16, tl16, oracle_mod.indel_argmax(fl16, tl16, want_matrix=True)[2])}


@pytest.mark.parametrize("which,general", [("narrow", False), ("narrow", True), ("wide", False), ("wide", True)])
def test_indel_topn_mixed(ctx, ratio_lists, monkeypatch, which, general):
    """from-lengths on both sides of every word class's border -- with ntop > 1 the short ones run in the one-string kernel -- against
    ~200 to-strings, every one twice; 16-bit symbols; everything through the general kernel.  Column 0 == pfz_indel_argmax, which
    runs the quad / octo kernels on the short rows: the two paths are tied together"""
    from polyfuzz_amd import _lib
    fl, tl, mat = ratio_lists[which]
    n, n_to = len(fl), len(tl)
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    rng = np.random.default_rng(198)
    plain = lev_oracle.argmax(mat)
    skips = [(what, skip, _lib.indel_argmax(ctx, f, t, skip)) for what, skip in _three_skips(rng, plain[0], n, n_to, n_to - 1)]
    if general:
        monkeypatch.setenv("PFZ_K4_FORCE_GENERAL", "1")
    for what, skip, (a_idx, a_score) in skips:
        for ntop in (1, 3, 64):
            got = _lib.indel_topn(ctx, f, t, ntop, skip)
            _assert_topn(got, expected_topn(mat, ntop, skip), (which, general, what, ntop))
            np.testing.assert_array_equal(got[0][:, 0], a_idx)
            np.testing.assert_array_equal(got[1][:, 0], a_score)
    assert mat[0, tl.index("")] == 100.0 and len(fl[0]) == 0                     # both empty


# ---- 6. the matcher ------------------------------------------------------------------------------------------------------

def _want_frame(fl, names, idx, val, normalize):
    data = {"From": fl}
    for r in range(idx.shape[1]):
        data["To" if r == 0 else f"To_{r + 1}"] = [names[j] if j >= 0 else None for j in idx[:, r]]
        data["Similarity" if r == 0 else f"Similarity_{r + 1}"] = val[:, r]
    df = pd.DataFrame(data)
    if normalize:
        lo, hi = val.min(), val.max()
        for c in df.columns:
            if c.startswith("Similarity"):
                df[c] = (df[c] - lo) / (hi - lo)
    return df


def _assert_frame(df, want):
    assert list(df.columns) == list(want.columns) and len(df) == len(want)
    for c in want.columns:
        if c.startswith("Similarity"):
            assert df[c].dtype == np.float64
            np.testing.assert_array_equal(df[c].to_numpy(), want[c].to_numpy(), err_msg=c)
        else:
            assert df[c].tolist() == want[c].tolist(), c


def _scores(oracle_mod, name, fl, tl):
    if name in SCORERS:
        return lev_oracle.sim_matrix(fl, tl, lev_oracle.matrix(fl, tl, name))
    srt = (lambda l: [" ".join(sorted(s.split())) for s in l]) if name == "token_sort_ratio" else (lambda l: l)
    mat = oracle_mod.indel_argmax(srt(fl), srt(tl), want_matrix=True)[2]
    if name == "QRatio":
        mat[[i for i, s in enumerate(fl) if not s]] = 0.0          # QRatio: 0 when either string is empty
        assert (mat[:, [j for j, s in enumerate(tl) if not s]] == 0.0).all()
    return mat


@pytest.mark.parametrize("name", ["ratio", "levenshtein", "osa", "token_sort_ratio", "QRatio"])
def test_matcher_top_n(ctx, oracle_mod, golden, name):
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import EditDistance
    t = golden["titles_lists"]
    fl = t["from_list"][:50] + ["", "new york mets", "mets  york new", ""]
    tl = t["to_list"][:90] + ["york new mets", "", "new york yankees"] + t["to_list"][:20]
    sim = _scores(oracle_mod, name, fl, tl)
    e_idx, e_val = expected_topn(sim, 3)
    for normalize in (False, True):
        m = EditDistance(scorer=name, normalize=normalize)
        m.top_n = 3
        df = m.match(fl, tl)
        assert list(df.columns) == ["From", "To", "Similarity", "To_2", "Similarity_2", "To_3", "Similarity_3"]
        _assert_frame(df, _want_frame(fl, tl, e_idx, e_val, normalize))
        assert (df["Similarity"] >= df["Similarity_2"]).all() and (df["Similarity_2"] >= df["Similarity_3"]).all()
    if name == "QRatio":
        assert (e_val[fl.index("")] == 0.0).all() and e_idx[fl.index("")].tolist() == [0, 1, 2]
    # re_train=False: the resident to-list and its plan serve again
    m = EditDistance(scorer=name, normalize=False)
    m.top_n = 3
    m.match(fl[:5], tl)
    held = m._to_dev
    df = m.match(fl, list(tl), re_train=False)
    assert m._to_dev is held
    _assert_frame(df, _want_frame(fl, tl, e_idx, e_val, False))
    # the clip at a to-list of 2
    df = m.match(fl, tl[:2])
    assert list(df.columns) == ["From", "To", "Similarity", "To_2", "Similarity_2"]
    _assert_frame(df, _want_frame(fl, tl[:2], *expected_topn(sim[:, :2], 2), False))
    # a self-match with repeats: the from-string's own first occurrence is left out and nothing else
    dup = golden["titles_self_list"]["from_list"][:60] + golden["titles_self_list"]["from_list"][:15] + ["", ""]
    s_idx, s_val = expected_topn(_scores(oracle_mod, name, dup, dup), 3, _first_occurrence(dup))
    for normalize in (False, True):
        m = EditDistance(scorer=name, normalize=normalize)
        m.top_n = 3
        _assert_frame(m.match(dup), _want_frame(dup, dup, s_idx, s_val, normalize))
    if name != "QRatio":
        assert (s_val[:15, 0] == s_val.max()).all() and (s_idx[:15, 0] >= 60).all()      # (the repeated strings find their twins)
    # top_n = 1 is the frame of an instance that never touched the attribute
    m = EditDistance(scorer=name)
    m.top_n = 1
    assert m.match(fl, tl).equals(EditDistance(scorer=name).match(fl, tl))
    m.top_n = 70
    with pytest.raises(_lib.PfzUnsupported, match="64"):
        m.match(fl, tl)                                                      # 70 after clipping: beyond the 64 of a wave
