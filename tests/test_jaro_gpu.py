"""GPU parity of K8 (all-pairs Jaro / Jaro-Winkler + first arg-max) against the definition (tests/jaro_oracle.py): every
comparison is exact, == on float64 scores and on indices.  PARITY UNPINNED beyond the oracle (tests/test_jaro_cpu.py holds
the oracle to jellyfish wherever it is installed)."""
import pickle

import numpy as np
import pandas as pd
import pytest

from tests import jaro_oracle

pytestmark = pytest.mark.gpu

SCORERS = ("jaro", "jaro_winkler")


def _rand(rng, alpha, lo, hi, n):
    return ["".join(rng.choice(list(alpha), size=int(rng.integers(lo, hi + 1)))) for _ in range(n)]


def _first_occurrence(strings):
    first = {}
    for j, s in enumerate(strings):
        first.setdefault(s, j)
    return np.array([first[s] for s in strings], np.int32)


@pytest.fixture(scope="module")
def mixed(golden):
    """~120 x 250: real titles, the edge lengths of the register kernel's word classes (31 .. 65 on either side and on both;
    to-strings of 255 .. 257, where its four flag words end), strings far beyond them, characters the to-list never uses,
    code points above 255 and above 0xFFFF, dense strings over two letters, prefixes of 0..6 common characters around
    w = 0.7"""
    rng = np.random.default_rng(81)
    t = golden["titles_lists"]
    edge = [31, 32, 33, 63, 64, 65]
    base = "the quick brown fox jumps over the lazy dog and runs far away from home again"
    prefixes = ["abcdef"[:k] + "uvwxyz"[k:] + tail for k in range(7) for tail in ("", "mnopq", "qponm")]
    fl = (t["from_list"][:35] + ["", "a", "ab", "the matrix", "Z"] + [base[:n] for n in edge] + [base[::-1][:n] for n in edge] +
          ["ab" * 100, "naïve café Ωmega \U0001f600 smile", "qqq中文", "####", "\U0001f600\U0001f601"] + _rand(rng, "ab", 1, 70, 30) +
          prefixes[:14] + _rand(rng, "abcdefgh ", 60, 66, 10))
    tl = (t["to_list"][:100] + ["", "a", "ba", "the matrix", "The Matrix"] + [base[:n] for n in edge] + [base[3:3 + n] for n in edge] +
          ["ba" * 75, "naïve cafe Ωmega \U0001f601 smile \U0001f600", "中文qqq"] + [(base * 4)[:n] for n in (255, 256, 257)] + ["ab" * 150] + _rand(rng, "ab", 1, 70, 30) + prefixes +
          _rand(rng, "abcdefgh ", 60, 66, 20) + _rand(rng, "abc", 1, 9, 50))
    return fl, tl, {name: jaro_oracle.matrix(fl, tl, name) for name in SCORERS}


def test_matrix_bit_exact(ctx, mixed):
    from polyfuzz_amd import _lib
    fl, tl, want = mixed
    assert 110 <= len(fl) <= 130 and 230 <= len(tl) <= 270
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for name in SCORERS:
        got = _lib.jaro_matrix(ctx, f, t, name)
        np.testing.assert_array_equal(got, want[name], err_msg=name)
        idx, score = _lib.jaro_argmax(ctx, f, t, name)
        e_idx, e_score = jaro_oracle.argmax(want[name])
        np.testing.assert_array_equal(idx, e_idx)
        np.testing.assert_array_equal(score, e_score)
    part = _lib.jaro_matrix(ctx, f, t, "jaro_winkler", 30, 61)           # a row shard
    np.testing.assert_array_equal(part, want["jaro_winkler"][30:61])
    assert want["jaro_winkler"][fl.index("the matrix"), tl.index("the matrix")] == 1.0
    assert (want["jaro"][fl.index("")] == 0.0).all() and (want["jaro"][:, tl.index("")] == 0.0).all()


def test_invalid_scorer_is_refused(ctx):
    from polyfuzz_amd import _lib
    f = _lib.DeviceStrings.upload(ctx, ["a"])
    out = np.zeros(1)
    for scorer in (2, -1):
        assert ctx.lib.pfz_jaro_matrix_host(ctx.h, f.h, f.h, scorer, 0, 1, out.ctypes.data_as(_lib.c_vp)) == -1      # PFZ_ERR_INVALID
    with pytest.raises(KeyError):
        _lib.jaro_matrix(ctx, f, f, "ratio")


@pytest.fixture(scope="module")
def tied(golden):
    """~150 x 400 with every to-string present two or three times: ties in every row, the first index must win"""
    rng = np.random.default_rng(82)
    t = golden["titles_lists"]
    uniq = t["to_list"][:110] + _rand(rng, "ab", 1, 40, 30) + ["", "x" * 70, "the"]
    tl = uniq + uniq[::-1] + uniq[:114]
    fl = t["from_list"][:100] + _rand(rng, "ab", 1, 40, 40) + ["", "x" * 70, "y" * 66] + uniq[:7]
    return fl, tl, {name: jaro_oracle.matrix(fl, tl, name) for name in SCORERS}


def test_argmax_ties_and_skip_codes(ctx, tied):
    from polyfuzz_amd import _lib
    fl, tl, want = tied
    assert len(fl) == 150 and len(tl) == 400
    n = len(fl)
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    rng = np.random.default_rng(83)
    for name in SCORERS:
        plain = jaro_oracle.argmax(want[name])
        # a left-out index: the row's own best (the next equal string must win), -1 (nothing) for every fifth row
        one = plain[0].copy()
        one[::5] = -1
        # "everything up to": -2 - k leaves choices 0..k out; the last rows keep no candidate at all
        up_to = (-2 - rng.integers(0, len(tl) - 1, n)).astype(np.int32)
        up_to[::7] = -1
        up_to[-3:] = -2 - (len(tl) - 1)
        for skip in (None, one, up_to):
            e_idx, e_score = plain if skip is None else jaro_oracle.argmax(want[name], skip)
            idx, score = _lib.jaro_argmax(ctx, f, t, name, skip)
            np.testing.assert_array_equal(idx, e_idx, err_msg=name)
            np.testing.assert_array_equal(score, e_score, err_msg=name)
            out = _lib.DeviceTopN.alloc(ctx, n, 2)
            _lib.jaro_argmax_dev(ctx, f, t, name, out, skip)
            d_idx, d_score = _lib.best_from_topn(*out.download())
            np.testing.assert_array_equal(d_idx[:n], e_idx)
            np.testing.assert_array_equal(d_score[:n], e_score)
        assert (jaro_oracle.argmax(want[name], up_to)[0][-3:] == -1).all()
        assert (plain[0] < len(tl) - 114).all()                        # (every best has a later twin: ties did occur)
    idx2, _ = _lib.jaro_argmax(ctx, f, t, "jaro", None, 40, 90)        # a row shard
    np.testing.assert_array_equal(idx2, jaro_oracle.argmax(want["jaro"])[0][40:90])
    with pytest.raises(_lib.PfzError):
        _lib.jaro_argmax(ctx, f, t, "jaro", np.where(np.arange(n) % 2 == 0, 3, -5).astype(np.int32))     # both forms in one call


def test_few_rows_many_choices(ctx):
    """3 x 5 000: 79 groups of to-strings, split over many workgroups per from-string; the host and the device entry agree"""
    from polyfuzz_amd import _lib, datasets
    _, titles = datasets.c3_lists(5000)
    tl = titles[:5000]
    fl = [tl[1234], "the lord of the rings the return of the king", "ab"]
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for name in SCORERS:
        e_idx, e_score = jaro_oracle.argmax(jaro_oracle.matrix(fl, tl, name))
        idx, score = _lib.jaro_argmax(ctx, f, t, name)
        np.testing.assert_array_equal(idx, e_idx)
        np.testing.assert_array_equal(score, e_score)
        out = _lib.DeviceTopN.alloc(ctx, 3, 2)
        _lib.jaro_argmax_dev(ctx, f, t, name, out)
        d_idx, d_score = _lib.best_from_topn(*out.download())
        np.testing.assert_array_equal(d_idx[:3], e_idx)
        np.testing.assert_array_equal(d_score[:3], e_score)
    assert e_score[0] == 1.0 and tl[e_idx[0]] == tl[1234]


def _frame(fl, names, idx, score, normalize):
    df = pd.DataFrame({"From": fl, "To": [names[j] for j in idx], "Similarity": score})
    if normalize:           # reference _distance.py:83-86
        df["Similarity"] = (df["Similarity"] - df["Similarity"].min()) / (df["Similarity"].max() - df["Similarity"].min())
    return df


def test_matcher(ctx, golden):
    from polyfuzz_amd.models import EditDistance
    t = golden["titles_lists"]
    fl, tl = t["from_list"][:100], t["to_list"][:200]
    e_idx, e_score = jaro_oracle.argmax(jaro_oracle.matrix(fl, tl, "jaro_winkler"))
    for normalize in (False, True):
        model = EditDistance(scorer="jaro_winkler", normalize=normalize)
        df = model.match(fl, tl)
        want = _frame(fl, tl, e_idx, e_score, normalize)
        assert list(df.columns) == ["From", "To", "Similarity"]
        assert df["From"].tolist() == fl and df["To"].tolist() == want["To"].tolist()
        np.testing.assert_array_equal(df["Similarity"].to_numpy(), want["Similarity"].to_numpy())
    # re_train=False on the same list: the resident copy and its plan serve again
    model = EditDistance(scorer="jaro_winkler", normalize=False)
    model.match(fl[:10], tl)
    held = model._to_dev
    df = model.match(fl, list(tl), re_train=False)
    assert model._to_dev is held
    np.testing.assert_array_equal(df["Similarity"].to_numpy(), e_score)
    # a pickled matcher leaves its device handles behind and works after loading
    clone = pickle.loads(pickle.dumps(model))
    assert clone._to_dev is None and clone._scorer_name == "jaro_winkler"
    df = clone.match(fl, tl)
    assert df["To"].tolist() == [tl[j] for j in e_idx]
    np.testing.assert_array_equal(df["Similarity"].to_numpy(), e_score)
    # Jaro by name, and a self-match with repeats: the from-string's own first occurrence is left out
    dup = golden["titles_self_list"]["from_list"][:120] + golden["titles_self_list"]["from_list"][:30]
    s_idx, s_score = jaro_oracle.argmax(jaro_oracle.matrix(dup, dup, "jaro"), _first_occurrence(dup))
    df = EditDistance(scorer="jaro_similarity", normalize=False).match(dup)
    assert df["To"].tolist() == [dup[j] for j in s_idx]
    np.testing.assert_array_equal(df["Similarity"].to_numpy(), s_score)
    assert (s_score[:30] == 1.0).all()                  # (the repeats find their twins)
