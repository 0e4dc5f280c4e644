"""A workgroup's SECOND row, on a match table it cleared itself.  The general form of every edit-distance kernel keeps the
from-string's match table in global memory -- zero on entry, zero again after every row -- and runs a grid capped at a multiple of
the compute-unit count; a bit the clearing leaves behind gives the workgroup's next row a wrong LCS or distance and raises no
fault.  Every list here has more general rows than the grid of its kernel (K4 and K7: 2 per compute unit, K11 / K12 / K13: 8; K10
deals two general rows to every other workgroup by its own rule), sized by the device's compute-unit count, and every result is
held to the CPU oracles with ==.  tests/second_row_cases.py makes the lists; tests/test_second_row_cpu.py checks them."""
import contextlib

import numpy as np
import pytest

from tests import lev_oracle
from tests import second_row_cases as sc
from tests.test_components_cpu import union_find_labels
from tests.test_edit_topn_gpu import _assert_topn, _three_skips, expected_topn
from tests.test_join_gpu import _assert_join

pytestmark = pytest.mark.gpu

SCORERS = lev_oracle.SCORERS


@contextlib.contextmanager
def _profile(ctx, *names):
    """with _profile(ctx, name, ...) as box: ...calls...  ->  box[name] = the launches / the count of that profile name"""
    box = {}
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        yield box
        ctx.sync()
        for name in names:
            box[name] = ctx.prof_get(name)[1]
    finally:
        ctx.prof_enable(False)


# ---- K4 ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=(False, True), ids=("symbols8", "symbols16"))
def k4_case(request, ctx, oracle_mod):
    """2 x CUs + 96 from-strings of 0 .. 130 characters (W = 3 words) against 256 to-strings, every one twice; the C oracle's matrix"""
    n_cu = ctx.info()["n_cu"]
    fl, tl = sc.k4_lists(n_cu, wide=request.param)
    e_idx, e_score, mat = oracle_mod.indel_argmax(fl, tl, want_matrix=True)
    assert len(fl) == 2 * n_cu + 96 and len(tl) == 256 and (len(set("".join(tl))) > 255) == request.param
    return n_cu, fl, tl, e_idx, e_score, mat


def _k4_dev_argmax(ctx, f, t, n, skip):
    from polyfuzz_amd import _lib
    out = _lib.DeviceTopN.alloc(ctx, n, 2)
    _lib.indel_argmax_dev(ctx, f, t, out, skip)
    idx, score = _lib.best_from_topn(*out.download())
    return idx[:n], score[:n]


def test_k4_argmax(ctx, k4_case, monkeypatch):
    """PFZ_K4_FORCE_GENERAL: all 2 x CUs + 96 rows in one general launch of 2 x CUs workgroups (the rows go in word-class order, so
    the second rows are the list's longest strings, on tables the shorter ones used).  Arg-max, host and device entry, under the
    three skip forms: with the row's own best left out its later twin must win"""
    from polyfuzz_amd import _lib
    n_cu, fl, tl, e_idx, e_score, mat = k4_case
    n, n_to = len(fl), len(tl)
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    monkeypatch.setenv("PFZ_K4_FORCE_GENERAL", "1")
    rng = np.random.default_rng(721)
    for what, skip in _three_skips(rng, e_idx, n, n_to, n_to - 1):
        w_idx, w_score = lev_oracle.argmax(mat, skip)
        if skip is None:
            np.testing.assert_array_equal(w_idx, e_idx)
            np.testing.assert_array_equal(w_score, e_score)
        with _profile(ctx, "k4_indel_general", "k4_general_rows", "k4_quad_launches") as box:
            idx, score = _lib.indel_argmax(ctx, f, t, skip)
            d_idx, d_score = _k4_dev_argmax(ctx, f, t, n, skip)
        assert box == {"k4_indel_general": 2, "k4_general_rows": 2 * n, "k4_quad_launches": 0} and n > 2 * n_cu, box
        np.testing.assert_array_equal(idx, w_idx, err_msg=what)
        np.testing.assert_array_equal(score, w_score, err_msg=what)
        np.testing.assert_array_equal(d_idx, w_idx, err_msg=f"{what} (device entry)")
        np.testing.assert_array_equal(d_score, w_score, err_msg=f"{what} (device entry)")
        if what == "one choice":
            moved = skip >= 0
            assert (w_score[moved] == e_score[moved]).all() and (w_idx[moved] > skip[moved]).all()      # ties did occur
    assert (e_score > 50).sum() > n // 3                                          # (rows with near matches to lose)


def test_k4_matrix(ctx, k4_case, monkeypatch):
    """the whole matrix -- a call of 128 rows has 128 workgroups and no second row -- and, as a call of its own, the 64 rows either
    side of row 2 x CUs"""
    from polyfuzz_amd import _lib
    n_cu, fl, tl, e_idx, e_score, mat = k4_case
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    monkeypatch.setenv("PFZ_K4_FORCE_GENERAL", "1")
    with _profile(ctx, "k4_general_rows") as box:
        got = _lib.indel_matrix(ctx, f, t)
    assert box["k4_general_rows"] == len(fl) > 2 * n_cu
    np.testing.assert_array_equal(got, mat)
    lo, hi = max(0, 2 * n_cu - 64), 2 * n_cu + 64
    np.testing.assert_array_equal(_lib.indel_matrix(ctx, f, t, lo, hi), mat[lo:hi])
    assert mat[fl.index(""), tl.index("")] == 100.0


def test_k4_topn(ctx, k4_case, monkeypatch):
    from polyfuzz_amd import _lib
    n_cu, fl, tl, e_idx, e_score, mat = k4_case
    n, n_to = len(fl), len(tl)
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    monkeypatch.setenv("PFZ_K4_FORCE_GENERAL", "1")
    rng = np.random.default_rng(722)
    for what, skip in _three_skips(rng, e_idx, n, n_to, n_to - 1):
        for ntop in (1, 3, 64):
            with _profile(ctx, "k4_general_rows") as box:
                got = _lib.indel_topn(ctx, f, t, ntop, skip)
            assert box["k4_general_rows"] == n > 2 * n_cu
            _assert_topn(got, expected_topn(mat, ntop, skip), (what, ntop))


# ---- K11, K12, K13 -------------------------------------------------------------------------------------------------------------------

class _Joins:
    """the family list of this device, its bounds and the distances walked so far; want(metric, thr, two_lists) -> the oracle's CSR"""

    def __init__(self, n_cu):
        self.n_cu = n_cu
        self.sl, self.family = sc.family_list(n_cu)
        self.second = self.sl[:256]
        self.bounds = {False: sc.distance_bounds(self.sl, self.sl), True: sc.distance_bounds(self.sl, self.second)}
        self.cache, self.made = {}, {}

    def want(self, metric, thr, two_lists):
        key = (metric, thr, two_lists)
        if key not in self.made:
            self.made[key] = sc.join_oracle(self.sl, self.second if two_lists else self.sl, thr, metric, not two_lists, self.cache,
                                            self.bounds[two_lists])
        return self.made[key]

    def components(self, metric, thr):
        row_ptr, idx, _, _ = self.want(metric, thr, False)
        n = len(self.sl)
        labels = union_find_labels(n, zip(np.repeat(np.arange(n), np.diff(row_ptr)).tolist(), idx.tolist()))
        return labels, len(idx), int((labels == np.arange(n)).sum())


@pytest.fixture(scope="module")
def joins(ctx):
    j = _Joins(ctx.info()["n_cu"])
    lens = lev_oracle.lengths(j.sl)
    assert len(j.sl) == 8 * j.n_cu + 256 and lens.min() > 64 and lens.max() <= 93      # every row is the general kernel's
    return j


def _assert_components(got, want, what):
    label, pairs, components = got[:3]
    assert label.dtype == np.int32 and label.shape == want[0].shape, what
    np.testing.assert_array_equal(label, want[0], err_msg=f"{what}: labels")
    assert (pairs, components) == want[1:], (what, pairs, components, want[1:])


@pytest.mark.parametrize("name", SCORERS)
def test_k11_join(ctx, joins, name):
    """8 x CUs + 256 rows in a general launch of 8 x CUs workgroups: the list with itself and against its first 256 strings, pairs,
    distances and score bits == the oracle's on the pairs the two bounds leave, and no other pair in the output"""
    from polyfuzz_amd import _lib
    f, t = _lib.DeviceStrings.upload(ctx, joins.sl), _lib.DeviceStrings.upload(ctx, joins.second)
    for thr in sc.JOIN_THRESHOLDS:
        for two_lists in (False, True):
            want = joins.want(name, thr, two_lists)
            with _profile(ctx, "k11_join", "k11_join_general") as box:
                got = _lib.lev_join(ctx, f, t if two_lists else None, name, thr, capacity=len(want[1]) + 64)
            _assert_join(got, want, f"{name} t={thr} two_lists={two_lists}")
            assert box == {"k11_join": 1, "k11_join_general": 1}, box
            assert len(want[1]) > len(joins.second)                              # (hits in both rounds of the grid)
    assert (np.diff(joins.want(name, 0.9, False)[0])[8 * joins.n_cu:] > 0).any()   # (second rows with hits of their own)


@pytest.mark.parametrize("name", SCORERS)
def test_k12_components(ctx, joins, name):
    from polyfuzz_amd import _lib
    f = _lib.DeviceStrings.upload(ctx, joins.sl)
    for thr in sc.JOIN_THRESHOLDS:
        want = joins.components(name, thr)
        with _profile(ctx, "k12_walk", "k12_walk_general") as box:
            *got, work = _lib.lev_components(ctx, f, name, thr, counters=True)
        assert box == {"k12_walk": 1, "k12_walk_general": 1}, box
        _assert_components(got, want, f"{name} t={thr}")
        *join, join_work = _lib.lev_join(ctx, f, None, name, thr, counters=True)
        assert got[1] == len(join[1]) and work == join_work, (name, thr, work, join_work)
        assert 1 < want[2] < len(joins.sl) - 100


def test_k13_join(ctx, joins):
    from polyfuzz_amd import _lib
    f, t = _lib.DeviceStrings.upload(ctx, joins.sl), _lib.DeviceStrings.upload(ctx, joins.second)
    for thr in sc.JOIN_THRESHOLDS:
        for two_lists in (False, True):
            want = joins.want("indel", thr, two_lists)
            with _profile(ctx, "k13_join", "k13_join_general") as box:
                got = _lib.indel_join(ctx, f, t if two_lists else None, thr, capacity=len(want[1]) + 64)
            _assert_join(got, want, f"indel t={thr} two_lists={two_lists}")
            assert box == {"k13_join": 1, "k13_join_general": 1}, box
            assert len(want[1]) > len(joins.second)
    assert (np.diff(joins.want("indel", 0.9, False)[0])[8 * joins.n_cu:] > 0).any()


def test_k13_components(ctx, joins):
    from polyfuzz_amd import _lib
    f = _lib.DeviceStrings.upload(ctx, joins.sl)
    for thr in sc.JOIN_THRESHOLDS:
        want = joins.components("indel", thr)
        with _profile(ctx, "k13_comp", "k13_comp_general") as box:
            *got, work = _lib.indel_components(ctx, f, thr, counters=True)
        assert box == {"k13_comp": 1, "k13_comp_general": 1}, box
        _assert_components(got, want, f"indel t={thr}")
        *join, join_work = _lib.indel_join(ctx, f, None, thr, counters=True)
        assert got[1] == len(join[1]) and work == join_work, (thr, work, join_work)
        assert 1 < want[2] < len(joins.sl) - 100


# ---- K7 ------------------------------------------------------------------------------------------------------------------------------

K7_MODES = ("WRatio", "token_set_ratio", "partial_ratio")


@pytest.mark.parametrize("mode", K7_MODES)
def test_k7_general(ctx, oracle_mod, monkeypatch, mode):
    """PFZ_K7_FORCE_GENERAL: 2 x CUs + 64 from-strings of word soup, '' and one-token strings among the first and the second rows,
    on the 2 x CUs workgroups of the general kernel against 48 to-strings; WRatio also as a self-match with every string's first
    occurrence left out.  First best choice and float64 score, bit for bit"""
    from polyfuzz_amd import _lib
    n_cu = ctx.info()["n_cu"]
    fl, tl = sc.k7_lists(n_cu)
    assert len(fl) == 2 * n_cu + 64 and len(tl) == 48
    monkeypatch.setenv("PFZ_K7_FORCE_GENERAL", "1")
    idx, score = _lib.fuzz_extract_one(ctx, fl, tl, mode)
    e_idx, e_score = oracle_mod.fuzz_extract_one(fl, tl, mode)
    np.testing.assert_array_equal(score, e_score, err_msg=mode)
    np.testing.assert_array_equal(idx, e_idx, err_msg=mode)
    assert (e_score[2 * n_cu:] == 100.0).any() and len(set(e_score[2 * n_cu:].tolist())) >= 3
    if mode == "WRatio":
        skip = sc.first_occurrence(fl)
        assert (skip != np.arange(len(fl))).sum() > 20
        idx, score = _lib.fuzz_extract_one(ctx, fl, fl, mode, skip)
        e_idx, e_score = oracle_mod.fuzz_extract_one(fl, fl, mode, skip)
        np.testing.assert_array_equal(score, e_score, err_msg="self-match")
        np.testing.assert_array_equal(idx, e_idx, err_msg="self-match")


# ---- K10 -----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def k10_case(oracle_mod):
    from tests.test_pairs_rescore_gpu import all_scores
    fl, tl, tab = sc.k10_lists()
    return fl, tl, tab, all_scores(oracle_mod, fl, tl)


@pytest.mark.parametrize("name", ("ratio", "levenshtein", "osa", "jaro", "jaro_winkler"))
def test_k10_two_general_rows_per_workgroup(ctx, k10_case, name):
    """200 from-strings, the general ones (beyond 64 characters) at the even positions: K10's general grid is one workgroup per
    general row, 100, and workgroup b is dealt the rows b and b + 100 -- two general rows for every even b.  (Under Jaro the grid
    is one workgroup per from-row, so those two scorers are held to the oracle on single rows.)"""
    from polyfuzz_amd import _lib
    from tests.test_pairs_rescore_gpu import _k10_counters, device_table, expected
    fl, tl, tab, sims = k10_case
    n_cu = ctx.info()["n_cu"]
    general = set(np.nonzero(lev_oracle.lengths(fl) > 64)[0].tolist())
    jaro = name in ("jaro", "jaro_winkler")
    grid = sc.k10_general_grid(len(fl), len(general), n_cu, jaro)
    dealt = sc.k10_rows_of_workgroups(len(fl), grid)
    twice = sum(1 for rows in dealt if len(general & set(rows)) >= 2)
    assert jaro or (grid == 100 and twice >= 40), (grid, twice)
    f, t, c = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl), device_table(ctx, tab)
    with _k10_counters(ctx) as box:
        got = _lib.pairs_rescore_topn(ctx, f, t, c, name, 8)
    assert box["launches"] == 1 and box["general"] == 1
    _assert_topn(got, expected(sims[name], tab, 8), name)
