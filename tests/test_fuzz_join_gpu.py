"""GPU parity of K18 -- RapidFuzz.join / _lib.fuzz_join, every pair whose K7 score reaches a cutoff -- against
oracle.native.fuzz_matrix thresholded by the same `t * 100.0`: row pointers, to-indices and score bits, compared with ==.
PARITY UNPINNED beyond the oracle (rapidfuzz is not installable)."""
import ctypes
import functools

import numpy as np
import pytest

from tests import helpers
from tests.test_fuzz_gpu import MODES, _lists

pytestmark = pytest.mark.gpu


def expect_join(truth, cutoff, self_join=False):
    """(row_ptr int64, idx int32, score float64) of the pairs truth >= cutoff; a self-join: the strict upper triangle"""
    hit = truth >= cutoff
    if self_join:
        hit &= np.triu(np.ones_like(hit), 1)
    rows, cols = np.nonzero(hit)                         # (row-major: to-indices ascending within a row)
    row_ptr = np.zeros(truth.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=truth.shape[0]), out=row_ptr[1:])
    return row_ptr, cols.astype(np.int32), truth[rows, cols]


def assert_join_equals(got, want, msg=""):
    for g, w, what in zip(got, want, ("row_ptr", "idx", "score")):
        assert g.dtype == w.dtype and g.shape == w.shape, (msg, what, g.shape, w.shape)
        np.testing.assert_array_equal(g.view(np.int64) if what == "score" else g, w.view(np.int64) if what == "score" else w,
                                      err_msg=f"{msg} {what}")


@functools.lru_cache(maxsize=None)
def case_1_lists():
    fl, tl = _lists(3, 70, 150)
    fl += ["this is a test", "this is a word", "fuzzy was a bear", "", "a", "mets mets mets new"]
    tl += ["this is a new test!!!", "THIS IS A WORD", "fuzzy fuzzy was a bear", "", "this is a test!", "new mets"]
    return tuple(fl), tuple(tl)


@functools.lru_cache(maxsize=None)
def case_1_truth(mode):
    import oracle
    oracle.build_native()
    fl, tl = case_1_lists()
    return oracle.native.fuzz_matrix(list(fl), list(tl), mode)


@functools.lru_cache(maxsize=None)
def self_list():
    sl = _lists(9, 130, 1, long_words=True)[0]
    return tuple(sl + [sl[3], sl[10], "", "", "  ", "  "])


@functools.lru_cache(maxsize=None)
def self_truth(mode):
    import oracle
    oracle.build_native()
    return oracle.native.fuzz_matrix(list(self_list()), list(self_list()), mode)


def thresholds(truth):
    """the fixed similarities of the cases and two attained scores / 100 (a cutoff that IS a score: equality must be kept)"""
    attained = np.unique(truth)
    return [0, 0.29, 0.6, 0.855, 0.9, 1.0] + [float(attained[len(attained) // 3]) / 100, float(attained[-2]) / 100]


@pytest.mark.parametrize("parts", ["1", "3"])
@pytest.mark.parametrize("mode", MODES)
def test_every_scorer_two_lists(ctx, monkeypatch, mode, parts):
    """76 x 156 strings, every scorer, every threshold, a from-row as one unit and as three.  At t = 0 with one part a unit queues
    156 survivors: the 128-entry ring wraps."""
    from polyfuzz_amd import _lib
    fl, tl = map(list, case_1_lists())
    truth = case_1_truth(mode)
    assert truth.shape == (76, 156)
    counts = [int((truth >= t * 100.0).sum()) for t in (0, 0.6, 0.855, 0.9, 1.0)]
    if mode == "WRatio":
        assert counts == [11856, 2640, 1758, 163, 5]
    else:
        assert counts[0] == 11856 and counts[-1] >= 361                      # no threshold is vacuous
    monkeypatch.setenv("PFZ_K7_PARTS", parts)
    f_dev, t_dev = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for t in thresholds(truth):
        got = _lib.fuzz_join(ctx, f_dev, t_dev, mode, t * 100.0)
        assert_join_equals(got, expect_join(truth, t * 100.0), f"{mode} t={t!r} parts={parts}")


@pytest.mark.parametrize("n_to", [1, 63, 64, 65, 129, 300])
def test_group_borders_and_empty_lists(ctx, oracle_mod, monkeypatch, n_to):
    """3 from-strings against to-lists that end on, before and behind a group of 64; 300 choices as ONE unit at t = 0: more
    survivors than the queue holds twice over, the ring wraps; and the empty lists"""
    from polyfuzz_amd import _lib
    fl = ["new york mets", "atlanta braves vs", ""]
    tl = _lists(21, 1, n_to)[1]
    monkeypatch.setenv("PFZ_K7_PARTS", "1")
    f_dev, t_dev = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for mode in ("WRatio", "token_set_ratio"):
        truth = oracle_mod.native.fuzz_matrix(fl, tl, mode)
        for t in (0, 0.6, 1.0):
            assert_join_equals(_lib.fuzz_join(ctx, f_dev, t_dev, mode, t * 100.0), expect_join(truth, t * 100.0), f"{mode} {n_to} {t}")
    if n_to == 1:
        none = _lib.DeviceStrings.upload(ctx, [])
        row_ptr, idx, score = _lib.fuzz_join(ctx, none, t_dev, "WRatio", 0.0)
        assert row_ptr.tolist() == [0] and len(idx) == len(score) == 0
        row_ptr, idx, score = _lib.fuzz_join(ctx, f_dev, none, "WRatio", 0.0)
        assert row_ptr.tolist() == [0, 0, 0, 0] and len(idx) == len(score) == 0
        row_ptr, idx, score = _lib.fuzz_join(ctx, none, None, "WRatio", 0.0)
        assert row_ptr.tolist() == [0] and len(idx) == 0
        assert _lib.fuzz_join(ctx, _lib.DeviceStrings.upload(ctx, ["a"]), None, "WRatio", 0.0)[0].tolist() == [0, 0]      # never (i, i)


@pytest.mark.parametrize("mode", ["WRatio", "token_ratio", "partial_ratio", "partial_token_set_ratio"])
def test_self_join_is_the_strict_upper_triangle(ctx, mode):
    """136 strings with repeats, "" twice and "  " twice: every i < j once as row i, to-index j; the from-handle as to-handle gives
    the bytes NULL gives; token-less copies are pairs only where the scorer gives them a score above the cutoff"""
    from polyfuzz_amd import _lib
    names = list(self_list())
    truth = self_truth(mode)
    if mode == "WRatio":
        head = truth[:130, :130]
        assert [int(((head >= t * 100.0) & np.triu(np.ones_like(head, bool), 1)).sum()) for t in (0.6, 0.9, 1.0)] == [1825, 136, 3]
    dev = _lib.DeviceStrings.upload(ctx, names)
    for t in (0, 0.6, 0.9, 1.0):
        want = expect_join(truth, t * 100.0, self_join=True)
        got = _lib.fuzz_join(ctx, dev, None, mode, t * 100.0)
        assert_join_equals(got, want, f"{mode} self t={t}")
        assert_join_equals(_lib.fuzz_join(ctx, dev, dev, mode, t * 100.0), got, f"{mode} self, own handle, t={t}")
    # positions 132 / 133 are "", 134 / 135 "  ": WRatio("", "") is 0 (two blanks are equal non-empty strings: 100); without a token
    # partial_token_set_ratio gives both pairs of copies 0; token_ratio and partial_ratio give them 100
    row_ptr, idx, _ = _lib.fuzz_join(ctx, dev, None, mode, 60.0)
    partners = lambda i: idx[row_ptr[i]:row_ptr[i + 1]].tolist()
    assert (133 in partners(132), 135 in partners(134)) == {"WRatio": (False, True), "partial_token_set_ratio": (False, False)}.get(mode, (True, True))
    assert 130 in partners(3) and 131 in partners(10)                        # the repeated strings have a token: 100 with their copies


@functools.lru_cache(maxsize=None)
def beyond_lists():
    """the lists of tests/test_fuzz_gpu.py::test_strings_beyond_the_fast_kernel, plus a from-string of 65 .. 128 and one of
    129 .. 256 characters: all three regions of the call and all three word classes"""
    fl, tl = _lists(11, 12, 60, long_words=True)
    rng = np.random.default_rng(5)
    words = ["alpha", "beta", "gamma", "delta", "of", "the", "inc", "llc", "new", "york", "mets", "braves"]
    long_from = " ".join(rng.choice(words, size=70))
    many_tok = " ".join(f"t{i}" for i in range(40))
    fl += [long_from[:400], many_tok, "new york mets", "", long_from[:100], long_from[3:203]]
    tl += [" ".join(f"t{i}" for i in range(3, 38)), long_from[5:300], "york new mets", "t1 t2 t3", ""]
    assert max(map(len, fl)) > 256 and max(len(set(s.split())) for s in tl) > 32
    assert any(64 < len(s) <= 128 for s in fl) and any(128 < len(s) <= 256 for s in fl)
    return tuple(fl), tuple(tl)


@pytest.mark.parametrize("mode", MODES)
def test_long_strings_and_the_general_path(ctx, oracle_mod, monkeypatch, mode):
    """a 400-character from-string, one of 40 distinct tokens, a to-string of 35: the three regions of a call -- fast rows x ordinary
    to-strings, general rows x all, fast rows x big slots -- each pair in exactly one; then ordinary strings through the general
    kernel, two lists and self-join.  (The scorers that sweep windows take several seconds here: the general kernel scores the
    400 x 295 character pair window by window in global memory, once per threshold -- K7's own test of these lists pays the same.)"""
    from polyfuzz_amd import _lib
    fl, tl = map(list, beyond_lists())
    truth = oracle_mod.native.fuzz_matrix(fl, tl, mode)
    f_dev, t_dev = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for t in (0, 0.6, 0.9):
        assert_join_equals(_lib.fuzz_join(ctx, f_dev, t_dev, mode, t * 100.0), expect_join(truth, t * 100.0), f"{mode} t={t}")
    monkeypatch.setenv("PFZ_K7_FORCE_GENERAL", "1")
    fl2, tl2 = _lists(12, 25, 40)
    truth2 = oracle_mod.native.fuzz_matrix(fl2, tl2, mode)
    f2, t2 = _lib.DeviceStrings.upload(ctx, fl2), _lib.DeviceStrings.upload(ctx, tl2)
    for t in (0, 0.6, 0.9):
        assert_join_equals(_lib.fuzz_join(ctx, f2, t2, mode, t * 100.0), expect_join(truth2, t * 100.0), f"{mode} general t={t}")
    truth2s = oracle_mod.native.fuzz_matrix(fl2, fl2, mode)
    assert_join_equals(_lib.fuzz_join(ctx, f2, None, mode, 60.0), expect_join(truth2s, 60.0, True), f"{mode} general self")


def test_wide_alphabet(ctx, oracle_mod):
    """more than 256 symbols (tests/test_fuzz_gpu.py::test_alphabet_size_and_the_scratch_columns at n_chars = 600, smaller lists):
    the scratch columns hold 16-bit ranks; both families of windows run"""
    from polyfuzz_amd import _lib
    n_chars = 600
    rng = np.random.default_rng(n_chars)
    glyphs = [chr(0x4E00 + k) for k in range(n_chars)]

    def mk(n, lo, hi):
        return [" ".join("".join(rng.choice(glyphs, size=int(rng.integers(lo, hi)))) for _ in range(int(rng.integers(1, 5)))) for _ in range(n)]
    tl = mk(400, 2, 9) + mk(60, 1, 3)
    fl = []
    for _ in range(60):
        t = tl[int(rng.integers(0, len(tl)))]
        a, b = sorted(int(x) for x in rng.integers(0, len(t) + 1, size=2))
        piece = t[a:b] or t[:3]
        fl.append(piece if rng.random() < 0.5 else piece + " " + tl[int(rng.integers(0, len(tl)))] + " " + "".join(rng.choice(glyphs, size=6)))
    fl += mk(20, 2, 9) + ["", glyphs[0]]
    assert len(set("".join(tl))) > 256
    f_dev, t_dev = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for mode in ("WRatio", "partial_ratio"):
        truth = oracle_mod.native.fuzz_matrix(fl, tl, mode)
        want = expect_join(truth, 0.6 * 100.0)
        assert len(want[1]) > 0
        assert_join_equals(_lib.fuzz_join(ctx, f_dev, t_dev, mode, 0.6 * 100.0), want, mode)


def test_capacity_on_the_device(ctx):
    """the C entry itself, its arrays pre-filled with a sentinel: below the total nothing is written and *out_total is exact; at the
    total and above the answer is exact; the same call twice gives the same bytes"""
    from polyfuzz_amd import _lib
    fl, tl = map(list, case_1_lists())
    want = expect_join(case_1_truth("WRatio"), 85.5)
    T = len(want[1])
    assert T == 1758
    f_dev, t_dev = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)

    def call(cap):
        row_ptr = np.full(len(fl) + 1, -7, np.int64)
        idx = np.full(max(cap, 1) + 3, -7, np.int32)
        score = np.full(max(cap, 1) + 3, -7.0, np.float64)
        total = ctypes.c_int64(-1)
        _lib.check(ctx.lib.pfz_fuzz_join(ctx.h, f_dev.h, t_dev.h, 0, 85.5, cap, _lib._ptr(row_ptr), _lib._ptr(idx), _lib._ptr(score),
                                         ctypes.byref(total), None))
        return row_ptr, idx, score, total.value
    for cap in (0, T - 1):
        row_ptr, idx, score, total = call(cap)
        assert total == T and (row_ptr == -7).all() and (idx == -7).all() and (score == -7.0).all()
    for cap in (T, T + 1):
        row_ptr, idx, score, total = call(cap)
        assert total == T and (idx[T:] == -7).all() and (score[T:] == -7.0).all()
        assert_join_equals((row_ptr, idx[:T], score[:T]), want, f"capacity {cap}")
        again = call(cap)
        assert all(a.tobytes() == b.tobytes() for a, b in zip((row_ptr, idx, score), again[:3]))
    for bad in ((7, 90.0, 8), (-1, 90.0, 8), (0, float("nan"), 8), (0, -0.5, 8), (0, 100.5, 8), (0, 90.0, -1)):
        total = ctypes.c_int64(0)
        rc = ctx.lib.pfz_fuzz_join(ctx.h, f_dev.h, t_dev.h, bad[0], bad[1], bad[2], _lib._ptr(np.zeros(len(fl) + 1, np.int64)),
                                   _lib._ptr(np.zeros(8, np.int32)), _lib._ptr(np.zeros(8, np.float64)), ctypes.byref(total), None)
        assert rc != 0, bad
        with pytest.raises(_lib.PfzError):
            _lib.check(rc)


def test_counters(ctx):
    """150 x 3 000 titles, WRatio.  At t = 0 every pair is bounded and every pair is scored; at t = 0.9 the bound leaves at most a
    tenth of the pairs to score (the CPU bound alone keeps 0.47 %; coarse entries and the slack have a factor of 20).
    Measured on an MI355X at t = 0.9: 450 000 bounded, 416 scored (0.092 %), 13 hits (the figures are printed)."""
    from polyfuzz_amd import _lib, datasets
    fl, tl = datasets.c3_lists(3000)
    fl = fl[:150]
    f_dev, t_dev = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    row_ptr, idx, score, work = _lib.fuzz_join(ctx, f_dev, t_dev, "WRatio", 0.0, counters=True)
    assert row_ptr[-1] == 150 * 3000 and work["bounded"] == 150 * 3000 and work["scored"] == work["bounded"] and work["steps"] > 0
    row_ptr, idx, score, work = _lib.fuzz_join(ctx, f_dev, t_dev, "WRatio", 0.9 * 100.0, counters=True)
    hits = int(row_ptr[-1])
    print(f"t = 0.9: bounded {work['bounded']}, scored {work['scored']} ({work['scored'] / work['bounded']:.4%}), hits {hits}")
    assert work["bounded"] == 150 * 3000 and hits <= work["scored"] and 10 * work["scored"] <= work["bounded"]


def test_full_size_against_the_committed_fixture(ctx):
    """All 20 000 x 20 000 titles, WRatio, t = 0.9, against tests/golden/c3_fuzz_oracle_WRatio.npz: a row has a hit iff the fixture's
    best score is >= 90 (5 903 rows); the row's maximum is the fixture's score, bit for bit; the smallest to-index among its maxima
    is the fixture's index; and the same per-row maxima are fuzz_extract_one's on the device."""
    from polyfuzz_amd import _lib
    fl, tl = helpers.c3_fuzz_lists()
    rows, e_idx, e_score = helpers.load_c3_fuzz_golden("WRatio")
    assert len(rows) == 20_000
    f_dev, t_dev = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    cutoff = 0.9 * 100.0
    row_ptr, idx, score = _lib.fuzz_join(ctx, f_dev, t_dev, "WRatio", cutoff)
    n_hits = np.diff(row_ptr)
    has = e_score >= cutoff
    assert int(has.sum()) == 5903
    np.testing.assert_array_equal(n_hits > 0, has)
    assert (score >= cutoff).all() and all((np.diff(idx[a:b]) > 0).all() for a, b in zip(row_ptr[:-1], row_ptr[1:]) if b - a > 1)
    starts = row_ptr[:-1][has]
    row_max = np.maximum.reduceat(score, starts)
    np.testing.assert_array_equal(row_max.view(np.int64), e_score[has].view(np.int64))
    row_of = np.repeat(np.arange(20_000), n_hits)
    is_max = score == np.repeat(row_max, n_hits[has])
    first_max = np.full(20_000, np.iinfo(np.int32).max, np.int64)
    np.minimum.at(first_max, row_of[is_max], idx[is_max])
    np.testing.assert_array_equal(first_max[has], e_idx[has])
    d_idx, d_score = _lib.fuzz_extract_one(ctx, f_dev, t_dev, "WRatio")
    np.testing.assert_array_equal(row_max.view(np.int64), d_score[has].view(np.int64))
    np.testing.assert_array_equal(first_max[has], d_idx[has])
    assert (d_score[~has] < cutoff).all()


def test_frame(ctx):
    """RapidFuzz().join: columns, order, Similarity * 100 the oracle's bits, the self-join form, re_train=False, a K4 scorer"""
    from polyfuzz_amd.models import RapidFuzz
    fl, tl = map(list, case_1_lists())
    truth = case_1_truth("WRatio")
    row_ptr, idx, score = expect_join(truth, 0.855 * 100.0)
    m = RapidFuzz(score_cutoff=0.99)                      # (the constructor's cut-off plays no part)
    df = m.join(fl, tl, 0.855)
    frm = np.repeat(np.arange(len(fl)), np.diff(row_ptr))
    assert list(df.columns) == ["From", "To", "Similarity"] and len(df) == 1758
    assert df["From"].tolist() == [fl[i] for i in frm] and df["To"].tolist() == [tl[j] for j in idx]
    sim = df["Similarity"].to_numpy()
    np.testing.assert_array_equal(sim, score / 100)
    assert (sim * 100 == score).mean() > 0.9 and np.abs(sim * 100 - score).max() < 1e-13      # (the division's inverse, where it is exact)
    held = m._to_dev
    assert held is not None and m.join(fl, list(tl), 0.855, re_train=False).equals(df) and m._to_dev is held
    assert m.join(fl, tl[:-1], 0.855, re_train=False)["To"].tolist() == [tl[j] for j in idx if j < len(tl) - 1] and m._to_dev is not held
    names = list(self_list())
    rp, ix, sc = expect_join(self_truth("WRatio"), 0.9 * 100.0, self_join=True)
    ds = RapidFuzz().join(names, min_similarity=0.9)
    fr = np.repeat(np.arange(len(names)), np.diff(rp))
    assert ds["From"].tolist() == [names[i] for i in fr] and ds["To"].tolist() == [names[j] for j in ix]
    np.testing.assert_array_equal(ds["Similarity"].to_numpy(), sc / 100)
    assert (fr < ix).all()
    with pytest.raises(NotImplementedError):
        RapidFuzz(scorer="ratio").join(fl, tl, 0.9)


def test_pool_fill(ctx):
    """the join and the self-join under every fill mode of the allocator: the output bytes do not depend on what a fresh device
    block holds"""
    from polyfuzz_amd import _lib
    fl, tl = map(list, case_1_lists())
    names = list(self_list())
    want = expect_join(case_1_truth("WRatio"), 0.855 * 100.0)
    want_s = {mode: expect_join(self_truth(mode), 60.0, True) for mode in ("WRatio", "partial_ratio")}
    try:
        for fill in (1, 2, 3, 0):
            ctx.pool_fill(fill)
            f_dev, t_dev, dev = (_lib.DeviceStrings.upload(ctx, x) for x in (fl, tl, names))
            assert_join_equals(_lib.fuzz_join(ctx, f_dev, t_dev, "WRatio", 0.855 * 100.0), want, f"fill {fill}")
            for mode in want_s:
                assert_join_equals(_lib.fuzz_join(ctx, dev, None, mode, 60.0), want_s[mode], f"fill {fill} self {mode}")
    finally:
        ctx.pool_fill(0)
