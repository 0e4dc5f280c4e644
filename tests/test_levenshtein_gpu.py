"""GPU parity of K9 (all-pairs Levenshtein / OSA similarity + first arg-max) against the definition (tests/lev_oracle.py: the
Wagner-Fischer table): every comparison is exact, == on int32 distances, on float64 scores and on indices.  PARITY UNPINNED beyond
the oracle (tests/test_levenshtein_cpu.py holds it to rapidfuzz wherever that is installed)."""
import contextlib
import pickle

import numpy as np
import pandas as pd
import pytest

from tests import lev_oracle

pytestmark = pytest.mark.gpu

SCORERS = lev_oracle.SCORERS


def _rand(rng, alpha, lo, hi, n):
    return ["".join(rng.choice(list(alpha), size=int(rng.integers(lo, hi + 1)))) for _ in range(n)]


def _swapped(rng, s, k):
    """`s` with k transpositions of two adjacent, different characters at places that do not touch: 2 k edits for Levenshtein, k
    for OSA -- and between two such variants of one string, every swap of either counts half under OSA"""
    s, free = list(s), set(range(len(s) - 1))
    for _ in range(k):
        ok = [i for i in sorted(free) if s[i] != s[i + 1]]
        if not ok:
            break
        i = ok[int(rng.integers(len(ok)))]
        s[i], s[i + 1] = s[i + 1], s[i]
        free -= {i - 1, i, i + 1}
    return "".join(s)


def _first_occurrence(strings):
    first = {}
    for j, s in enumerate(strings):
        first.setdefault(s, j)
    return np.array([first[s] for s in strings], np.int32)


def _dev_argmax(ctx, f, t, name, n, skip=None):
    from polyfuzz_amd import _lib
    out = _lib.DeviceTopN.alloc(ctx, n, 2)
    _lib.lev_argmax_dev(ctx, f, t, name, out, skip)
    idx, score = _lib.best_from_topn(*out.download())
    return idx[:n], score[:n]


@contextlib.contextmanager
def _k9_counters(ctx):
    """with _k9_counters(ctx) as box: ...K9 calls...  ->  box["walked"] = pairs whose recurrence was walked, box["general"] = launches
    of the general kernel, box["launches"] = timed K9 scopes (one per call)"""
    box = {}
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        yield box
        ctx.sync()
        box["walked"] = ctx.prof_get("k9_pairs_walked")[1]
        box["general"] = ctx.prof_get("k9_lev_general")[1]
        box["launches"] = ctx.prof_get("k9_lev")[1]
    finally:
        ctx.prof_enable(False)


def _skip_forms(rng, plain_idx, n, n_to, up_to_range):
    """the row's own best left out (the next equal string must win), nothing for every fifth row; and "everything up to k" codes,
    the last three rows keeping no candidate at all"""
    one = plain_idx.copy()
    one[::5] = -1
    up_to = (-2 - rng.integers(0, up_to_range, n)).astype(np.int32)
    up_to[::7] = -1
    up_to[-3:] = -2 - (n_to - 1)
    return one, up_to


def _assert_argmax(ctx, f, t, name, n, sim, skip, what):
    from polyfuzz_amd import _lib
    e_idx, e_score = lev_oracle.argmax(sim, skip)
    idx, score = _lib.lev_argmax(ctx, f, t, name, skip)
    assert idx.dtype == np.int32 and score.dtype == np.float64
    np.testing.assert_array_equal(idx, e_idx, err_msg=f"{name} {what}")
    np.testing.assert_array_equal(score, e_score, err_msg=f"{name} {what}")
    d_idx, d_score = _dev_argmax(ctx, f, t, name, n, skip)
    np.testing.assert_array_equal(d_idx, e_idx, err_msg=f"{name} {what} (device entry)")
    np.testing.assert_array_equal(d_score, e_score, err_msg=f"{name} {what} (device entry)")
    return e_idx, e_score


@pytest.fixture(scope="module")
def mixed(golden):
    """~120 x 250 on the recipe of test_jaro_gpu.py's `mixed`: real titles, the edge lengths of the word classes (0, 1, 31 .. 65 on
    the from-side; 0, 1, 255 .. 257 and 1 000 on the to-side), characters the to-list never uses, code points above 255 and above
    0xFFFF, 30 dense strings over two letters, and transposition-heavy pairs ("ab" * k against "ba" * k, CA / ABC, and a sentence
    with a few adjacent characters swapped, on both sides: that is where OSA and Levenshtein part)"""
    rng = np.random.default_rng(93)
    t = golden["titles_lists"]
    edge = [31, 32, 33, 63, 64, 65]
    base = "the quick brown fox jumps over the lazy dog and runs far away from home again"
    swaps = ["ab" * k for k in (1, 16, 17, 32, 33)]
    cut = lambda: base[:int(rng.integers(24, 65))]
    fl = (t["from_list"][:16] + ["", "a", "ab", "CA", "the matrix", "Z"] + [base[:n] for n in edge] + [base[::-1][:n] for n in edge] +
          ["ab" * 100, "naïve café Ωmega \U0001f600 smile", "qqq中文", "####", "\U0001f600\U0001f601"] + _rand(rng, "ab", 1, 70, 30) +
          swaps + ["abba" * 6, "baab" * 9] + _rand(rng, "abcdefgh ", 60, 66, 4) + [_swapped(rng, cut(), int(rng.integers(1, 6))) for _ in range(40)])
    tl = (t["to_list"][:40] + ["", "a", "ba", "ABC", "the matrix", "The Matrix"] + [base[:n] for n in edge] + [base[3:3 + n] for n in edge] +
          ["ba" * 75, "naïve cafe Ωmega \U0001f601 smile \U0001f600", "中文qqq"] + [(base * 4)[:n] for n in (255, 256, 257)] + [(base * 14)[:1000]] +
          _rand(rng, "ab", 1, 70, 30) + ["ba" * k for k in range(1, 16)] + ["ab" * k + "ba" * k for k in range(1, 11)] +
          _rand(rng, "abcdefgh ", 60, 66, 10) + _rand(rng, "abc", 1, 9, 20) + [_swapped(rng, cut(), int(rng.integers(1, 6))) for _ in range(95)])
    return fl, tl, {name: lev_oracle.matrix(fl, tl, name) for name in SCORERS}


def test_matrix_and_argmax_mixed(ctx, mixed):
    from polyfuzz_amd import _lib
    fl, tl, want = mixed
    assert 110 <= len(fl) <= 130 and 230 <= len(tl) <= 270
    lf, lt = set(map(len, fl)), set(map(len, tl))
    assert {0, 1, 31, 32, 33, 63, 64, 65} <= lf and {0, 1, 255, 256, 257, 1000} <= lt
    differ = (want["osa"] != want["levenshtein"]).mean()
    print(f"K9 mixed: OSA differs from Levenshtein in {differ:.3f} of the cells")
    assert differ >= 0.1 and (want["osa"] <= want["levenshtein"]).all()
    assert want["levenshtein"][fl.index("CA"), tl.index("ABC")] == 3 == want["osa"][fl.index("CA"), tl.index("ABC")]
    assert want["levenshtein"][fl.index("ab"), tl.index("ba")] == 2 and want["osa"][fl.index("ab"), tl.index("ba")] == 1
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for name in SCORERS:
        got = _lib.lev_matrix(ctx, f, t, name)
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, want[name], err_msg=name)
        sim = lev_oracle.sim_matrix(fl, tl, want[name])
        _assert_argmax(ctx, f, t, name, len(fl), sim, None, "mixed")
        np.testing.assert_array_equal(_lib.lev_matrix(ctx, f, t, name, 30, 61), want[name][30:61])           # a row shard
        idx, score = _lib.lev_argmax(ctx, f, t, name, None, 30, 61)
        e_idx, e_score = lev_oracle.argmax(sim)
        np.testing.assert_array_equal(idx, e_idx[30:61])
        np.testing.assert_array_equal(score, e_score[30:61])
        assert sim[fl.index("the matrix"), tl.index("the matrix")] == 1.0 and sim[fl.index(""), tl.index("")] == 1.0
        assert e_idx[fl.index("")] == tl.index("") and e_score[fl.index("")] == 1.0
        assert (sim[fl.index("####")] == 0.0).sum() > 0          # (from-characters the to-list never uses match nothing)


def test_invalid_scorer_is_refused(ctx):
    from polyfuzz_amd import _lib
    f = _lib.DeviceStrings.upload(ctx, ["a"])
    out = np.zeros(1, np.int32)
    for scorer in (2, -1):
        assert ctx.lib.pfz_lev_matrix_host(ctx.h, f.h, f.h, scorer, 0, 1, out.ctypes.data_as(_lib.c_vp)) == -1      # PFZ_ERR_INVALID
    with pytest.raises(KeyError):
        _lib.lev_matrix(ctx, f, f, "jaro")


@pytest.fixture(scope="module")
def tied(golden):
    """150 x 400 with every to-string present two or three times: ties in every row, the first index must win"""
    rng = np.random.default_rng(94)
    t = golden["titles_lists"]
    uniq = t["to_list"][:110] + _rand(rng, "ab", 1, 40, 30) + ["", "x" * 70, "the"]
    tl = uniq + uniq[::-1] + uniq[:114]
    fl = t["from_list"][:100] + _rand(rng, "ab", 1, 40, 40) + ["", "x" * 70, "y" * 66] + uniq[:7]
    return fl, tl, {name: lev_oracle.matrix(fl, tl, name) for name in SCORERS}


def test_argmax_ties_and_skip_codes(ctx, tied):
    from polyfuzz_amd import _lib
    fl, tl, want = tied
    assert len(fl) == 150 and len(tl) == 400
    n = len(fl)
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    rng = np.random.default_rng(95)
    for name in SCORERS:
        sim = lev_oracle.sim_matrix(fl, tl, want[name])
        plain = lev_oracle.argmax(sim)
        one, up_to = _skip_forms(rng, plain[0], n, len(tl), len(tl) - 1)
        for what, skip in (("no skip", None), ("one choice", one), ("up to", up_to)):
            _assert_argmax(ctx, f, t, name, n, sim, skip, what)
        assert (lev_oracle.argmax(sim, up_to)[0][-3:] == -1).all()
        assert (plain[0] < len(tl) - 114).all()                        # (every best has a later twin: ties did occur)
        s_idx, s_score = lev_oracle.argmax(sim, one)
        assert (s_score[one >= 0] == plain[1][one >= 0]).all() and (s_idx[one >= 0] > one[one >= 0]).all()
    with pytest.raises(_lib.PfzError):
        _lib.lev_argmax(ctx, f, t, "osa", np.where(np.arange(n) % 2 == 0, 3, -5).astype(np.int32))     # both forms in one call


def border_lists():
    """~40 x 300 over about 300 code points (Latin, Greek, a slice of CJK: 16-bit symbols), a dozen of them frequent: from-strings of
    65, 128, 129, 256, 257 and 600 characters beside the register classes' own borders, to-strings up to 2 000"""
    rng = np.random.default_rng(96)
    alpha = [chr(c) for c in list(range(0x61, 0x7b)) + [0x20] + list(range(0x3b1, 0x3ca)) + list(range(0x4e00, 0x4e00 + 250))]
    hot = alpha[:12]

    def mk(n, pool=None):
        pool = pool or hot * 30 + alpha
        return "".join(pool[int(k)] for k in rng.integers(0, len(pool), n))
    tl = [mk(int(n)) for n in rng.integers(0, 90, 270)] + [mk(n) for n in (64, 65, 128, 129, 256, 257, 600, 1999, 2000)] + \
        ["ab" * 64, "ba" * 64 + "b", "ab" * 300] + ["".join(alpha[k:k + 20]) for k in range(0, len(alpha), 20)]
    longs = [mk(n) for n in (65, 128, 129, 256, 257, 600)]
    fl = longs + ["ba" * 64, "ab" * 64 + "a", "ba" * 300, tl[270], tl[273][3:], tl[276][:590] + "zz\U0001f600", mk(64), mk(32), mk(33), mk(1), ""] + \
        [mk(int(n)) for n in rng.integers(2, 64, 19)] + [mk(70, hot[:2]), mk(130, hot[:2]), tl[5], tl[100][::-1]]
    return fl, tl


def test_general_kernel_and_word_class_borders(ctx):
    """~40 x 300: from-strings of 65, 128, 129, 256, 257 and 600 characters (the general kernel: two to ten 64-bit words in global
    memory) beside the register classes' own borders, to-strings up to 2 000, and a to-list of more than 256 distinct code points
    (16-bit symbols) -- one launch of the general kernel per call; then an alphabet of one symbol more than K4's 60 KiB table limit
    holds (the count is test_jaro_gpu.py's), where every from-string, however short, is the general kernel's"""
    from polyfuzz_amd import _lib
    from tests.test_jaro_gpu import LDS_LIMIT_SYMBOLS, lds_limit_lists
    fl, tl = border_lists()
    longs = fl[:6]
    distinct = len({c for s in tl for c in s})
    assert 256 < distinct < LDS_LIMIT_SYMBOLS and 35 <= len(fl) <= 45 and 290 <= len(tl) <= 310 and max(map(len, tl)) == 2000
    assert {65, 128, 129, 256, 257, 600} <= set(map(len, fl))
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for name in SCORERS:
        want = lev_oracle.matrix(fl, tl, name)
        with _k9_counters(ctx) as box:
            got = _lib.lev_matrix(ctx, f, t, name)
        assert box["general"] == 1 and box["launches"] == 1 and box["walked"] == len(fl) * len(tl)
        np.testing.assert_array_equal(got, want, err_msg=name)
        sim = lev_oracle.sim_matrix(fl, tl, want)
        with _k9_counters(ctx) as box:
            _assert_argmax(ctx, f, t, name, len(fl), sim, None, "borders")
        assert box["general"] == 2 and box["launches"] == 2
        assert sim[fl.index(tl[270]), 270] == 1.0 and (want[:6] < np.array([len(s) for s in longs])[:, None]).sum() > 100
    # one symbol beyond the table limit: nothing fits the LDS
    fl, tl = lds_limit_lists(LDS_LIMIT_SYMBOLS + 1, 100)
    assert len({c for s in tl for c in s}) == LDS_LIMIT_SYMBOLS + 1 and min(map(len, fl)) <= 32
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for name in SCORERS:
        want = lev_oracle.matrix(fl, tl, name)
        sim = lev_oracle.sim_matrix(fl, tl, want)
        with _k9_counters(ctx) as box:
            got = _lib.lev_matrix(ctx, f, t, name)
            _assert_argmax(ctx, f, t, name, len(fl), sim, None, "beyond the LDS limit")
        assert box["general"] == 3 and box["launches"] == 3 and box["walked"] == 3 * len(fl) * len(tl)
        np.testing.assert_array_equal(got, want, err_msg=name)
        assert (sim > 0.5).sum() >= 20


def pruning_lists():
    """4 096 to-strings over nine letters, lengths spread evenly over 1 .. 120, every other one a copy of an earlier one (ties), in
    scattered order; 300 from-strings: to-strings with 0 .. 3 random edits"""
    rng = np.random.default_rng(97)
    alpha = list("abcdefghi")
    uniq = ["".join(rng.choice(alpha, size=1 + (k * 120) // 2048)) for k in range(2048)]
    tl = uniq + uniq
    tl = [tl[k] for k in rng.permutation(4096)]
    fl = []
    for k in rng.choice(4096, 300, replace=False):
        s = list(tl[int(k)])
        for _ in range(int(rng.integers(0, 4))):
            kind, at = int(rng.integers(3)), int(rng.integers(0, len(s) + 1))
            if kind == 0:
                s.insert(at, str(rng.choice(alpha)))
            elif kind == 1 and len(s) > 1:
                del s[min(at, len(s) - 1)]
            elif s:
                s[min(at, len(s) - 1)] = str(rng.choice(alpha))
        fl.append("".join(s))
    return fl, tl


def test_pruning_by_the_length_bound(ctx):
    """300 x 4 096, lengths 1 .. 120: a workgroup walks from the groups nearest |a| outwards and stops a direction where the length
    bound falls strictly below its best.  Arg-max == the oracle's under the three skip forms (ties: every to-string is there twice;
    with the row's own best left out its later twin must win), host and device entry, and fewer than 300 x 4 096 pairs walked.
    Then to-strings of ONE length: nothing can be pruned, every pair is walked, both scorers.
    The 300 x 4 096 call is held to the oracle under Levenshtein only -- the table of 1.2 million pairs takes the numpy oracle ten
    seconds per scorer, and the walk order and the bound do not depend on the scorer; OSA's walked count is asserted all the same.
    Measured on an MI355X, share of the pairs walked without skip / one choice / up to: 0.7110 / 0.7127 / 0.7085 (OSA without skip:
    0.7104); 136 of the 300 from-strings are beyond 64 characters and the general kernel's, which walks everything -- the register
    kernel's rows walk 47 %."""
    from polyfuzz_amd import _lib
    fl, tl = pruning_lists()
    n, n_to = len(fl), len(tl)
    lt = np.array([len(s) for s in tl])
    assert n == 300 and n_to == 4096 and lt.min() == 1 and lt.max() == 120 and np.bincount(lt)[1:].min() >= 30
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    sim = lev_oracle.sim_matrix(fl, tl, lev_oracle.matrix(fl, tl, "levenshtein", workers=2))
    plain = lev_oracle.argmax(sim)
    rng = np.random.default_rng(98)
    one, up_to = _skip_forms(rng, plain[0], n, n_to, 512)
    for what, skip in (("no skip", None), ("one choice", one), ("up to", up_to)):
        with _k9_counters(ctx) as box:
            _assert_argmax(ctx, f, t, "levenshtein", n, sim, skip, what)
        share = box["walked"] / (2 * n * n_to)
        print(f"K9 pruning levenshtein {what}: {box['walked'] // 2} of {n * n_to} pairs walked per call, share {share:.4f}")
        assert box["launches"] == 2 and box["walked"] < 2 * n * n_to
    s_idx, s_score = lev_oracle.argmax(sim, one)
    assert (s_score[one >= 0] == plain[1][one >= 0]).all() and (s_idx[one >= 0] > one[one >= 0]).all()      # ties did occur
    assert (lev_oracle.argmax(sim, up_to)[0][-3:] == -1).all() and (plain[1] == 1.0).sum() >= 20
    with _k9_counters(ctx) as box:
        _lib.lev_argmax(ctx, f, t, "osa")
    print(f"K9 pruning osa no skip: {box['walked']} of {n * n_to} pairs walked, share {box['walked'] / (n * n_to):.4f}")
    assert box["walked"] < n * n_to
    # one length: every bound is the same, and none is strictly below a score
    same = [s for s in tl if len(s) == 40] * 16
    same = same[:512]
    from_40 = [s[:40] if len(s) >= 40 else s for s in fl]
    assert len(same) == 512 and {len(s) for s in same} == {40}
    f, t = _lib.DeviceStrings.upload(ctx, from_40), _lib.DeviceStrings.upload(ctx, same)
    for name in SCORERS:
        sim1 = lev_oracle.sim_matrix(from_40, same, lev_oracle.matrix(from_40, same, name))
        with _k9_counters(ctx) as box:
            idx, score = _lib.lev_argmax(ctx, f, t, name)
        e_idx, e_score = lev_oracle.argmax(sim1)
        np.testing.assert_array_equal(idx, e_idx, err_msg=name)
        np.testing.assert_array_equal(score, e_score, err_msg=name)
        assert box["walked"] == n * 512, name


def test_fixture_rows_at_full_width(ctx):
    """the 2 000 rows of tests/golden/c3_lev_oracle.npz against all 20 000 titles: index and score == the fixture's, the score
    recomputed from its distance and M"""
    import os
    from polyfuzz_amd import _lib, datasets
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c3_lev_oracle.npz"))
    fl, tl = datasets.c3_lists()
    assert len(fl) == len(tl) == 20_000 and str(g["source"]) == "oracle"
    rows = g["rows"]
    f, t = _lib.DeviceStrings.upload(ctx, [fl[i] for i in rows]), _lib.DeviceStrings.upload(ctx, tl)
    for name in SCORERS:
        m = g[f"M_{name}"]
        want = lev_oracle.similarity(g[f"distance_{name}"], m, m)
        with _k9_counters(ctx) as box:
            idx, score = _lib.lev_argmax(ctx, f, t, name)
        print(f"K9 fixture rows {name}: {box['walked']} of {len(rows) * len(tl)} pairs walked, share {box['walked'] / (len(rows) * len(tl)):.4f}")
        np.testing.assert_array_equal(idx, g[f"idx_{name}"], err_msg=name)
        np.testing.assert_array_equal(score, want, err_msg=name)
        d_idx, d_score = _dev_argmax(ctx, f, t, name, len(rows))
        np.testing.assert_array_equal(d_idx, g[f"idx_{name}"])
        np.testing.assert_array_equal(d_score, want)


def _frame(fl, names, idx, score, normalize):
    df = pd.DataFrame({"From": fl, "To": [names[j] for j in idx], "Similarity": score})
    if normalize:           # reference _distance.py:83-86
        df["Similarity"] = (df["Similarity"] - df["Similarity"].min()) / (df["Similarity"].max() - df["Similarity"].min())
    return df


def test_matcher(ctx, golden):
    from polyfuzz_amd.models import EditDistance
    t = golden["titles_lists"]
    fl, tl = t["from_list"][:100], t["to_list"][:200]
    best = {name: lev_oracle.argmax(lev_oracle.sim_matrix(fl, tl, lev_oracle.matrix(fl, tl, name))) for name in SCORERS}
    for name in SCORERS:
        e_idx, e_score = best[name]
        for normalize in (False, True):
            model = EditDistance(scorer=name, normalize=normalize)
            df = model.match(fl, tl)
            want = _frame(fl, tl, e_idx, e_score, normalize)
            assert list(df.columns) == ["From", "To", "Similarity"]
            assert df["From"].tolist() == fl and df["To"].tolist() == want["To"].tolist()
            np.testing.assert_array_equal(df["Similarity"].to_numpy(), want["Similarity"].to_numpy())
    e_idx, e_score = best["osa"]
    # re_train=False on the same list: the resident copy and its plan serve again; on a changed list: uploaded anew
    model = EditDistance(scorer="osa_normalized_similarity", normalize=False)
    model.match(fl[:10], tl)
    held = model._to_dev
    df = model.match(fl, list(tl), re_train=False)
    assert model._to_dev is held
    np.testing.assert_array_equal(df["Similarity"].to_numpy(), e_score)
    changed = tl[::-1]
    df = model.match(fl, changed, re_train=False)
    assert model._to_dev is not held
    c_idx, c_score = lev_oracle.argmax(lev_oracle.sim_matrix(fl, tl, lev_oracle.matrix(fl, tl, "osa"))[:, ::-1])
    assert df["To"].tolist() == [changed[j] for j in c_idx]
    np.testing.assert_array_equal(df["Similarity"].to_numpy(), c_score)
    # a pickled matcher leaves its device handles behind and works after loading
    clone = pickle.loads(pickle.dumps(model))
    assert clone._to_dev is None and clone._scorer_name == "osa"
    df = clone.match(fl, tl)
    assert df["To"].tolist() == [tl[j] for j in e_idx]
    np.testing.assert_array_equal(df["Similarity"].to_numpy(), e_score)
    # a self-match with repeats: the from-string's own first occurrence is left out (_distance.py:93-96)
    dup = golden["titles_self_list"]["from_list"][:120] + golden["titles_self_list"]["from_list"][:30]
    for name in SCORERS:
        sim = lev_oracle.sim_matrix(dup, dup, lev_oracle.matrix(dup, dup, name))
        s_idx, s_score = lev_oracle.argmax(sim, _first_occurrence(dup))
        df = EditDistance(scorer=name, normalize=False).match(dup)
        assert df["To"].tolist() == [dup[j] for j in s_idx]
        np.testing.assert_array_equal(df["Similarity"].to_numpy(), s_score)
        assert (s_score[:30] == 1.0).all()                  # (the repeats find their twins)


FAMILY_LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 128, 129)


def _family_list(rng, wide):
    """130 strings -- two full plan groups and a padded one -- 13 of each length of FAMILY_LENGTHS: prefixes of one sentence with
    a few characters replaced and a few adjacent ones swapped, so that many pairs are near each other.  wide: the replacements
    come from 400 code points of their own (more than 256 symbols: the plan packs 16 bits per symbol), else from eight letters"""
    base = "the quick brown fox jumps over the lazy dog and runs far away from home again, and then it sleeps " * 2
    pool = [chr(0x100 + k) for k in range(400)] if wide else list("abcdefgh")
    out = []
    for k in range(13):
        for n in FAMILY_LENGTHS:
            s = list(base[k % 3:k % 3 + n])
            places = rng.choice(n, min(n, int(rng.integers(0, 5)) + (n // 8 if wide else 0)), replace=False) if n else []
            for p in places:
                s[p] = pool[int(rng.integers(len(pool)))]
            out.append(_swapped(rng, "".join(s), int(rng.integers(0, 3))))
    if wide:      # every code point of the pool is in the list: the alphabet is wider than 8 bits whatever the draws were
        out[-1] = "".join(pool[:129])
        out[-2] = "".join(pool[129:257])
    return out


@pytest.mark.parametrize("wide", (False, True), ids=("symbols8", "symbols16"))
def test_the_four_entries_agree_on_one_list(ctx, wide):
    """K9's matrix, K11's join (two lists at t = 0, self at t = 0.5), K12's components and K10's rescoring on ONE list of 130
    strings against the oracle and each other: from-strings of all three row classes (<= 32, 33 .. 64, the general kernel's at two
    and three words), the general kernels at 256 lanes (K9, K11, K12) and at 64 (K10), 8- and 16-bit symbols, both scorers"""
    from polyfuzz_amd import _lib
    sl = _family_list(np.random.default_rng(97 + wide), wide)
    n = len(sl)
    assert n == 130 and sorted(set(map(len, sl))) == list(FAMILY_LENGTHS)
    assert (len({c for s in sl for c in s}) > 256) == wide
    f, t = _lib.DeviceStrings.upload(ctx, sl), _lib.DeviceStrings.upload(ctx, sl)
    every = _lib.DeviceTopN.from_host(ctx, np.tile(np.arange(n, dtype=np.int32), (n, 1)), np.zeros((n, n), np.float32))
    assert n <= _lib.PAIR_MAX_CANDIDATES
    upper = np.triu(np.ones((n, n), bool), 1)
    for name in SCORERS:
        want = lev_oracle.matrix(sl, sl, name)
        sim = lev_oracle.sim_matrix(sl, sl, want)
        np.testing.assert_array_equal(_lib.lev_matrix(ctx, f, t, name), want, err_msg=name)
        # t = 0 over two lists: every pair, with exactly those distances
        row_ptr, idx, dist, got_sim = _lib.lev_join(ctx, f, t, name, 0.0, capacity=n * n)
        np.testing.assert_array_equal(row_ptr, np.arange(n + 1, dtype=np.int64) * n, err_msg=name)
        np.testing.assert_array_equal(idx.reshape(n, n), np.tile(np.arange(n, dtype=np.int32), (n, 1)), err_msg=name)
        np.testing.assert_array_equal(dist.reshape(n, n), want, err_msg=name)
        np.testing.assert_array_equal(got_sim.reshape(n, n), sim, err_msg=name)
        # t = 0.5 over the list itself: the unordered pairs, and K12 walks what K11 walks
        hits = int((upper & (sim >= 0.5)).sum())
        assert 100 < hits < upper.sum()
        row_ptr, idx, dist, _, work = _lib.lev_join(ctx, f, None, name, 0.5, counters=True)
        assert row_ptr[-1] == hits == len(idx), name
        rows = np.repeat(np.arange(n), np.diff(row_ptr))
        assert (rows < idx).all() and (sim[rows, idx] >= 0.5).all()
        np.testing.assert_array_equal(dist, want[rows, idx], err_msg=name)
        label, pairs, components, comp_work = _lib.lev_components(ctx, f, name, 0.5, counters=True)
        assert pairs == hits and comp_work == work, (name, pairs, hits, comp_work, work)
        assert 1 <= components <= n and (label <= np.arange(n)).all() and (label[rows] == label[idx]).all()
        # K10 over every to-index as a candidate: the row's eight best, (score descending, index ascending)
        order = np.argsort(-sim, axis=1, kind="stable")[:, :8]
        got_idx, got_score = _lib.pairs_rescore_topn(ctx, f, t, every, name, 8)
        np.testing.assert_array_equal(got_idx, order.astype(np.int32), err_msg=name)
        np.testing.assert_array_equal(got_score, np.take_along_axis(sim, order, axis=1), err_msg=name)
