"""GPU parity of K19 -- RapidFuzz.top_n / _lib.fuzz_topn, the n best choices of every from-string under K7's scorers -- against
oracle.native.fuzz_matrix, stably sorted: int32 indices and the float64 scores' bits, compared with ==.
PARITY UNPINNED beyond the oracle (rapidfuzz is not installable)."""
import numpy as np
import pytest

from tests.test_fuzz_gpu import MODES, _lists
from tests.test_fuzz_join_gpu import beyond_lists, case_1_lists, case_1_truth, self_list, self_truth

pytestmark = pytest.mark.gpu


def expect_topn(truth, ntop, cutoff=0.0, skip=None):
    """(idx int32[n, ntop], score float64[n, ntop]): per row np.argsort(-scores, kind="stable")[:ntop] over the choices not left out
    (skip: K7's codes -- >= 0 that one choice, <= -2 every choice up to -2 - code) whose score is >= cutoff; -1 / 0.0 beyond"""
    n = truth.shape[0]
    idx, score = np.full((n, ntop), -1, np.int32), np.zeros((n, ntop), np.float64)
    for i in range(n):
        keep = truth[i] >= cutoff
        if skip is not None and skip[i] >= 0:
            keep[skip[i]] = False
        elif skip is not None and skip[i] <= -2:
            keep[:-1 - int(skip[i])] = False
        cand = np.nonzero(keep)[0]
        order = cand[np.argsort(-truth[i, cand], kind="stable")][:ntop]
        idx[i, :len(order)], score[i, :len(order)] = order, truth[i, order]
    return idx, score


def assert_topn_equals(got, want, msg=""):
    for g, w, what in zip(got, want, ("idx", "score")):
        assert g.dtype == w.dtype and g.shape == w.shape, (msg, what, g.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g.view(np.int64) if what == "score" else g, w.view(np.int64) if what == "score" else w,
                                      err_msg=f"{msg} {what}")


def first_equal(names):
    first = {}
    for j, s in enumerate(names):
        first.setdefault(s, j)
    return np.array([first[s] for s in names], np.int32)


@pytest.mark.parametrize("parts", ["1", "3"])
@pytest.mark.parametrize("mode", MODES)
def test_every_scorer_two_lists(ctx, monkeypatch, mode, parts):
    """76 x 156 strings, every scorer, a from-row as one unit and as three, ntop 1 / 2 / 5 / 64; column 0 is the arg-max kernel's
    answer.  With one part a unit meets 156 choices: the ring wraps while the floor moves."""
    from polyfuzz_amd import _lib
    fl, tl = map(list, case_1_lists())
    truth = case_1_truth(mode)
    assert truth.shape == (76, 156)
    monkeypatch.setenv("PFZ_K7_PARTS", parts)
    f_dev, t_dev = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    b_idx, b_score = _lib.fuzz_extract_one(ctx, f_dev, t_dev, mode)
    for ntop in (1, 2, 5, 64):
        got = _lib.fuzz_topn(ctx, f_dev, t_dev, mode, ntop)
        assert_topn_equals(got, expect_topn(truth, ntop), f"{mode} ntop={ntop} parts={parts}")
        np.testing.assert_array_equal(got[0][:, 0], b_idx)
        np.testing.assert_array_equal(got[1][:, 0].view(np.int64), b_score.view(np.int64))


@pytest.mark.parametrize("n_to", [1, 63, 64, 65, 129, 300])
def test_group_borders_and_empty_lists(ctx, oracle_mod, monkeypatch, n_to):
    """3 from-strings against to-lists that end on, before and behind a group of 64; ntop beyond the list pads with -1 / 0.0;
    and the empty lists"""
    from polyfuzz_amd import _lib
    fl = ["new york mets", "atlanta braves vs", ""]
    tl = _lists(21, 1, n_to)[1]
    monkeypatch.setenv("PFZ_K7_PARTS", "1")
    f_dev, t_dev = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for mode in ("WRatio", "token_set_ratio"):
        truth = oracle_mod.native.fuzz_matrix(fl, tl, mode)
        for ntop in (1, 64):
            got = _lib.fuzz_topn(ctx, f_dev, t_dev, mode, ntop)
            assert_topn_equals(got, expect_topn(truth, ntop), f"{mode} n_to={n_to} ntop={ntop}")
            if ntop > n_to:
                assert (got[0][:, n_to:] == -1).all() and (got[1][:, n_to:] == 0.0).all()
            part = _lib.fuzz_topn(ctx, f_dev, t_dev, mode, ntop, begin=1, end=3)          # a row range: the rows it names
            assert_topn_equals(part, (got[0][1:3], got[1][1:3]), f"{mode} n_to={n_to} ntop={ntop} rows 1..2")
    if n_to == 1:
        none = _lib.DeviceStrings.upload(ctx, [])
        idx, score = _lib.fuzz_topn(ctx, none, t_dev, "WRatio", 3)
        assert idx.shape == score.shape == (0, 3)
        idx, score = _lib.fuzz_topn(ctx, f_dev, none, "WRatio", 3)
        assert idx.shape == (3, 3) and (idx == -1).all() and (score == 0.0).all()
        for bad in ((0, 0.0), (-1, 0.0), (3, float("nan")), (3, -0.5), (3, 100.5)):
            with pytest.raises(_lib.PfzError) as e:
                _lib.fuzz_topn(ctx, f_dev, t_dev, "WRatio", bad[0], score_cutoff=bad[1])
            assert not isinstance(e.value, _lib.PfzUnsupported)
        with pytest.raises(_lib.PfzUnsupported):
            _lib.fuzz_topn(ctx, f_dev, t_dev, "WRatio", 65)


@pytest.mark.parametrize("mode", MODES)
def test_ties_against_the_order_of_the_walk(ctx, oracle_mod, monkeypatch, mode):
    """200 to-strings drawn from 5 distinct strings of different lengths, shuffled: the plan is sorted by length, so equal scores
    are met out of index order, and the result must still list them by ascending index (a floor test at <= loses them)"""
    from polyfuzz_amd import _lib
    base = ["a", "new york mets", "atlanta braves vs", "los angeles dodgers inc", "red sox vs yankees the boston"]
    assert len(set(map(len, base))) == 5
    rng = np.random.default_rng(19)
    tl = [base[k] for k in rng.integers(0, 5, 200)]
    fl = base + ["boston celtics", "zzz"]
    truth = oracle_mod.native.fuzz_matrix(fl, tl, mode)
    monkeypatch.setenv("PFZ_K7_PARTS", "1")
    f_dev, t_dev = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for ntop in (3, 40, 64):
        want = expect_topn(truth, ntop)
        assert all((np.diff(want[1][i]) == 0).any() for i in range(len(fl)))          # every row's list has a tie inside
        assert_topn_equals(_lib.fuzz_topn(ctx, f_dev, t_dev, mode, ntop), want, f"{mode} ntop={ntop}")


@pytest.mark.parametrize("mode", ["WRatio", "token_ratio", "partial_ratio", "partial_token_set_ratio"])
def test_choices_left_out(ctx, mode):
    """136 strings with repeats, "" twice and "  " twice against themselves: the default self-match (the first element equal to the
    from-string is left out) and reference_self_match (every choice up to the row: the last row has none)"""
    from polyfuzz_amd import _lib
    names = list(self_list())
    truth = self_truth(mode)
    n = len(names)
    dev = _lib.DeviceStrings.upload(ctx, names)
    for what, skip in (("equal", first_equal(names)), ("up to", (-2 - np.arange(n)).astype(np.int32))):
        for ntop in (1, 5, 64):
            got = _lib.fuzz_topn(ctx, dev, dev, mode, ntop, skip)
            assert_topn_equals(got, expect_topn(truth, ntop, skip=skip), f"{mode} {what} ntop={ntop}")
            if what == "up to":
                assert (got[0][-1] == -1).all() and (got[1][-1] == 0.0).all()
                assert (got[0][got[0] >= 0] > np.repeat(np.arange(n), (got[0] >= 0).sum(axis=1))).all()


@pytest.mark.parametrize("mode", ["WRatio", "partial_ratio", "token_set_ratio"])
def test_cutoff(ctx, mode):
    """score_cutoff 0 / 60 / 85.5 / 100 and one attained score (equality is kept): the cells below are -1 / 0.0, a row whose best is
    below has none"""
    from polyfuzz_amd import _lib
    fl, tl = map(list, case_1_lists())
    truth = case_1_truth(mode)
    mid = float(np.sort(truth[7])[-3])                  # an attained score: row 7's third best, so the cutoff itself is in its list
    f_dev, t_dev = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for cutoff in (0.0, 60.0, 85.5, 100.0, mid):
        for ntop in (5, 64):
            want = expect_topn(truth, ntop, cutoff)
            got = _lib.fuzz_topn(ctx, f_dev, t_dev, mode, ntop, score_cutoff=cutoff)
            assert_topn_equals(got, want, f"{mode} cutoff={cutoff!r} ntop={ntop}")
            assert (got[1][got[0] >= 0] >= cutoff).all()
    assert (expect_topn(truth, 5, mid)[1] == mid).any()                         # the attained cutoff is in a list: equal is kept
    assert (expect_topn(truth, 5, 100.0)[0][:, 0] == -1).any()                  # a row whose best is below the cutoff


@pytest.mark.parametrize("mode", MODES)
def test_beyond_the_fast_kernel(ctx, oracle_mod, mode):
    """a 400-character from-string, one of 40 distinct tokens, a to-string of 35: every pair lies in exactly one of the three
    regions of a call, a row's list is the merge of all three.  (The scorers that sweep windows take several seconds: the general
    kernel scores the 400 x 295 character pair window by window in global memory, as in K7's and K18's tests of these lists.)"""
    from polyfuzz_amd import _lib
    fl, tl = map(list, beyond_lists())
    truth = oracle_mod.native.fuzz_matrix(fl, tl, mode)
    got = _lib.fuzz_topn(ctx, _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl), mode, 5)
    assert_topn_equals(got, expect_topn(truth, 5), f"{mode} beyond")


@pytest.mark.parametrize("mode", MODES)
def test_the_general_kernel_alone(ctx, monkeypatch, mode):
    """PFZ_K7_FORCE_GENERAL: the lists of case 1 through the general kernel's third sink, four lists per row; and a self-match of
    48 strings there, both skip codes"""
    from polyfuzz_amd import _lib
    monkeypatch.setenv("PFZ_K7_FORCE_GENERAL", "1")
    fl, tl = map(list, case_1_lists())
    got = _lib.fuzz_topn(ctx, _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl), mode, 5)
    assert_topn_equals(got, expect_topn(case_1_truth(mode), 5), f"{mode} general")
    names = list(self_list())[88:]                      # (the tail: "" twice and "  " twice are in it)
    truth = self_truth(mode)[88:, 88:]
    dev = _lib.DeviceStrings.upload(ctx, names)
    for what, skip in (("equal", first_equal(names)), ("up to", (-2 - np.arange(len(names))).astype(np.int32))):
        assert_topn_equals(_lib.fuzz_topn(ctx, dev, dev, mode, 5, skip), expect_topn(truth, 5, skip=skip), f"{mode} general self {what}")


def test_counters(ctx, monkeypatch):
    """150 x 3 000 titles, WRatio: every pair is bounded once, whatever ntop; the rising floor leaves most pairs unscored at
    ntop = 1 and scores more as ntop grows; the counters change nothing in the result (the figures are printed).  A unit scores at
    least the ntop pairs its list holds.  With a row as ONE unit (PFZ_K7_PARTS = 1, as the full-size lists run) at most half of
    all pairs are scored at ntop = 1: among 3 000 titles a title's best shares a word with it (85.5 or more under WRatio), the
    bound of a choice that shares none is below that, and far fewer than half of the titles share a word with a given one.
    Split rows are not held to that: every part scores its first batches against the cutoff, a floor of its own each -- on an
    MI355X the default split of these lists (11 parts) scored about 253 000 of the 450 000 pairs at ntop = 1, one part 73 000."""
    from polyfuzz_amd import _lib, datasets
    fl, tl = datasets.c3_lists(3000)
    fl = fl[:150]
    f_dev, t_dev = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    want = {ntop: _lib.fuzz_topn(ctx, f_dev, t_dev, "WRatio", ntop) for ntop in (1, 64)}
    for parts in (None, "1"):
        if parts:
            monkeypatch.setenv("PFZ_K7_PARTS", parts)
        scored = []
        for ntop in (1, 64):
            idx, score, work = _lib.fuzz_topn(ctx, f_dev, t_dev, "WRatio", ntop, counters=True)
            assert_topn_equals((idx, score), want[ntop], f"ntop={ntop} parts={parts}")
            print(f"parts {parts or 'default'}, ntop = {ntop}: bounded {work['bounded']}, scored {work['scored']} "
                  f"({work['scored'] / work['bounded']:.4%})")
            assert work["bounded"] == 150 * 3000 and 150 * ntop <= work["scored"] <= work["bounded"] and work["steps"] > 0
            scored.append(work["scored"])
        assert scored[0] < scored[1]
    assert 2 * scored[0] <= 150 * 3000                       # (the last round: a row as one unit)


def test_stale_memory(ctx):
    """a two-list call and a self-match under the allocator's fill words 0x0, 0x1 and 0x0000000100000001: the same bytes"""
    from polyfuzz_amd import _lib
    fl, tl = map(list, case_1_lists())
    names = list(self_list())
    skip = first_equal(names)
    want = expect_topn(case_1_truth("WRatio"), 5), expect_topn(self_truth("partial_ratio"), 64, 60.0, skip)
    seen = []
    try:
        for fill in (_lib.Context.POOL_FILL_ZERO, _lib.Context.POOL_FILL_ONE64, _lib.Context.POOL_FILL_ONE32):
            ctx.pool_fill(fill)
            f_dev, t_dev, dev = (_lib.DeviceStrings.upload(ctx, x) for x in (fl, tl, names))
            got = _lib.fuzz_topn(ctx, f_dev, t_dev, "WRatio", 5), _lib.fuzz_topn(ctx, dev, dev, "partial_ratio", 64, skip, score_cutoff=60.0)
            for g, w in zip(got, want):
                assert_topn_equals(g, w, f"fill {fill}")
            seen.append(b"".join(a.tobytes() for g in got for a in g))
    finally:
        ctx.pool_fill(0)
    assert seen[0] == seen[1] == seen[2]


def test_the_matcher(ctx, oracle_mod):
    """RapidFuzz().top_n = 3 on the README lists and on a self-match: columns, dtypes, the first pair of columns the top_n = 1
    frame's, Similarity_k = oracle / 100, the cut-off, re_train=False, and the K4 scorers through indel_topn"""
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import RapidFuzz
    from_list = ["apple", "apples", "appl", "recal", "house", "similarity"]
    to_list = ["apple", "apples", "mouse"]
    cols = ["From", "To", "Similarity", "To_2", "Similarity_2", "To_3", "Similarity_3"]
    sim_cols = ("Similarity", "Similarity_2", "Similarity_3")

    def check_frame(df, names, idx, score, n_cols=3):
        assert list(df.columns) == cols[:1 + 2 * n_cols]
        for r in range(n_cols):
            to, sim = df[cols[1 + 2 * r]], df[cols[2 + 2 * r]]
            assert to.dtype == object and sim.dtype == np.float64
            assert to.tolist() == [names[j] if j >= 0 else None for j in idx[:, r]]
            np.testing.assert_array_equal(sim.to_numpy().view(np.int64), np.where(idx[:, r] >= 0, score[:, r] / 100, 0.0).view(np.int64))

    m = RapidFuzz()
    one = m.match(from_list, to_list)
    m.top_n = 3
    df = m.match(from_list, to_list)
    truth = oracle_mod.native.fuzz_matrix(from_list, to_list, "WRatio")
    check_frame(df, to_list, *expect_topn(truth, 3))
    assert df["From"].tolist() == from_list and df[["From", "To", "Similarity"]].equals(one)
    held = m._to_dev
    assert held is not None and m.match(from_list, list(to_list), re_train=False).equals(df) and m._to_dev is held
    assert m.match(from_list, to_list[:2], re_train=False).shape == (6, 5) and m._to_dev is not held          # clipped to two choices
    # the cut-off blanks cells (the reference's own scenario: a mean below 0.5)
    mc = RapidFuzz(score_cutoff=0.95)
    mc.top_n = 3
    dc = mc.match(from_list, to_list)
    check_frame(dc, to_list, *expect_topn(truth, 3, 0.95 * 100))
    assert dc["To_3"].isna().all() and dc["Similarity"].mean() < 0.5 and dc[["From", "To", "Similarity"]].equals(
        RapidFuzz(score_cutoff=0.95).match(from_list, to_list))
    # self-match: the default (the first equal element left out) and the reference's shrinking list
    names = list(self_list())
    st = self_truth("WRatio")
    ms = RapidFuzz()
    one = ms.match(names)
    ms.top_n = 3
    ds = ms.match(names)
    check_frame(ds, names, *expect_topn(st, 3, skip=first_equal(names)))
    assert ds[["From", "To", "Similarity"]].equals(one)
    dr = ms.match(names, reference_self_match=True)
    check_frame(dr, names, *expect_topn(st, 3, skip=(-2 - np.arange(len(names))).astype(np.int32)))
    assert dr.iloc[-1][["To", "To_2", "To_3"]].isna().all()
    # ratio and QRatio: K4's top-n on the strings themselves, QRatio's empty from-string scoring 0 against everything
    fl2, tl2 = ["apple", "", "appl"], ["apple", "", "apples", "mouse"]
    f_dev, t_dev = _lib.DeviceStrings.upload(ctx, fl2), _lib.DeviceStrings.upload(ctx, tl2)
    k4 = _lib.indel_topn(ctx, f_dev, t_dev, 3)
    for scorer in ("ratio", "QRatio"):
        mk = RapidFuzz(scorer=scorer)
        mk.top_n = 3
        idx, score = k4[0].copy(), k4[1].copy()
        if scorer == "QRatio":
            idx[1], score[1] = [0, 1, 2], 0.0
        check_frame(mk.match(fl2, tl2), tl2, idx, score)
    assert k4[0][1, 0] == 1 and k4[1][1, 0] == 100.0          # ratio("", "") is 100: the row QRatio changes
