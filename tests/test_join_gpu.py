"""GPU parity of K11 (EditDistance.join: every pair at or above a Levenshtein / OSA similarity, as CSR) against the definition
(tests/lev_oracle.py: the Wagner-Fischer table) thresholded on the host -- `sim >= t` on sim_matrix, row-major, i < j for the
self-join: every comparison is exact, == on indices, on int32 distances and on float64 scores."""
import ctypes
import os

import numpy as np
import pandas as pd
import pytest

from tests import lev_oracle

pytestmark = pytest.mark.gpu

SCORERS = lev_oracle.SCORERS
TWO_THIRDS = 1.0 - 1.0 / 3.0
# every pair; equal strings only; two everyday cut-offs; a score pairs DO attain (kept) and the next float64 (dropped)
THRESHOLDS = (0.0, 1.0, 0.5, 0.8, TWO_THIRDS, float(np.nextafter(TWO_THIRDS, 2.0)))
FROM_LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 130)
TO_SIZES = (1, 63, 64, 65, 300)


def _rand(rng, alpha, lo, hi, n):
    return ["".join(rng.choice(list(alpha), size=int(rng.integers(lo, hi + 1)))) for _ in range(n)]


def _edited(rng, s, alpha, k):
    s = list(s)
    for _ in range(k):
        kind, at = int(rng.integers(4)), int(rng.integers(0, len(s) + 1))
        if kind == 0:
            s.insert(at, str(rng.choice(list(alpha))))
        elif kind == 1 and len(s) > 1:
            del s[min(at, len(s) - 1)]
        elif kind == 2 and len(s) > 1:
            i = min(at, len(s) - 2)
            s[i], s[i + 1] = s[i + 1], s[i]
        elif s:
            s[min(at, len(s) - 1)] = str(rng.choice(list(alpha)))
    return "".join(s)


def _want(fl, tl, d, thr, self_join=False):
    """(row_ptr, idx, dist, sim) of the pairs with sim >= thr, row-major; self_join: i < j only"""
    sim = lev_oracle.sim_matrix(fl, tl, d)
    keep = sim >= thr
    if self_join:
        keep &= np.triu(np.ones(keep.shape, bool), 1)
    i, j = np.nonzero(keep)
    row_ptr = np.zeros(len(fl) + 1, np.int64)
    np.cumsum(np.bincount(i, minlength=len(fl)), out=row_ptr[1:])
    return row_ptr, j.astype(np.int32), d[i, j].astype(np.int32), sim[i, j]


def _assert_join(got, want, what):
    for g, w, part in zip(got, want, ("row_ptr", "idx", "dist", "sim")):
        assert g.dtype == w.dtype, (what, part, g.dtype)
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {part}")


def _launches(ctx, name):
    return ctx.prof_get(name)[1]


def _class_lists(alpha_name):
    """from-strings of every border length of the word classes (three each, one of them an edited copy of a to-string) and 300
    to-strings of lengths 0 .. 130 -- five groups, so every wave has several and a window cuts inside the plan; its prefixes of
    1, 63, 64 and 65 strings are the smaller to-lists.  Over "ab" (dense hits) or over 300 symbols (16-bit symbols, sparse hits)"""
    rng = np.random.default_rng(111 if alpha_name == "ab" else 112)
    alpha = "ab" if alpha_name == "ab" else "".join(chr(0x400 + k) for k in range(300))
    tl = [_rand(rng, alpha, 3, 3, 1)[0]] + _rand(rng, alpha, 0, 130, 288) + ["", "abab", alpha[:31], alpha[:2] * 32]
    tl += [_rand(rng, alpha, n, n, 1)[0] for n in (31, 32, 33, 63, 64, 65, 130)]
    tl = tl[:1] + [tl[k] for k in rng.permutation(np.arange(1, len(tl)))]
    assert len(tl) == 300
    fl = []
    for n in FROM_LENGTHS:
        fl += _rand(rng, alpha, n, n, 2)
        near = [s for s in tl if abs(len(s) - n) <= 2 and len(s) > 0]
        fl.append((_edited(rng, near[0], alpha, 2) + alpha[0] * n)[:n] if near else alpha[0] * n)
    fl += ["ababab", tl[5], tl[100], tl[200], alpha[:31], alpha[:2] * 32]      # d = 2 of M = 6 against "abab": exactly 1 - 1/3; copies: 1.0
    assert set(FROM_LENGTHS) <= set(map(len, fl))
    return fl, tl


@pytest.fixture(scope="module", params=("ab", "wide"))
def classes(request):
    fl, tl = _class_lists(request.param)
    return request.param, fl, tl, {name: lev_oracle.matrix(fl, tl, name) for name in SCORERS}


@pytest.mark.parametrize("name", SCORERS)
def test_word_classes_thresholds_and_to_list_sizes(ctx, classes, name):
    """~33 from-strings of lengths 0, 1, 31 .. 33, 63 .. 65 and 130 (32-bit words, 64-bit words, the general kernel) against
    to-lists of 1, 63, 64, 65 and 300 strings of lengths 0 .. 130, at every threshold of THRESHOLDS: 0.0 is the full matrix, 1.0
    the equal strings ('' against '' among them), 1 - 1/3 keeps the pairs that score exactly that and its float64 successor drops
    them.  Capacity left to the binding (its guess, and one repeat where the guess is short)."""
    from polyfuzz_amd import _lib
    alpha, fl, tl, want_d = classes
    assert len({c for s in tl for c in s}) > 256 if alpha == "wide" else len({c for s in tl for c in s}) == 2
    f = _lib.DeviceStrings.upload(ctx, fl)
    for n_to in TO_SIZES:
        t = _lib.DeviceStrings.upload(ctx, tl[:n_to])
        d = want_d[name][:, :n_to]
        ctx.prof_enable(True)
        ctx.prof_reset()
        try:
            for thr in THRESHOLDS:
                _assert_join(_lib.lev_join(ctx, f, t, name, thr), _want(fl, tl[:n_to], d, thr), f"{alpha} {name} n_to={n_to} t={thr!r}")
            ctx.sync()
            calls = _launches(ctx, "k11_join")                                     # (one per call; a short guess costs one repeat)
            assert len(THRESHOLDS) <= calls <= 2 * len(THRESHOLDS)
            assert _launches(ctx, "k11_join_general") == calls                     # (the from-strings of 65 and 130 characters)
        finally:
            ctx.prof_enable(False)
    sim = lev_oracle.sim_matrix(fl, tl, want_d[name])
    full = _want(fl, tl, want_d[name], 0.0)
    assert len(full[1]) == len(fl) * len(tl) and np.array_equal(full[2].reshape(len(fl), len(tl)), want_d[name])
    assert sim[fl.index(""), tl.index("")] == 1.0 and (sim == 1.0).sum() >= 6
    assert sim[fl.index("ababab"), tl.index("abab")] == TWO_THIRDS                 # attained exactly: kept at t, dropped just above
    if alpha == "ab":
        assert (sim >= 0.5).sum() > 300 and ((sim >= 0.8) & (sim < 1.0)).sum() >= 3 and (sim == TWO_THIRDS).sum() >= 1
    else:
        assert (sim >= 0.5).sum() < 100


def test_general_kernel_by_table_size(ctx):
    """one code point more than the 60 KiB table holds (7 680 in the to-list): every from-string, however short, is the general
    kernel's"""
    from polyfuzz_amd import _lib
    from tests.test_jaro_gpu import LDS_LIMIT_SYMBOLS, lds_limit_lists
    fl, tl = lds_limit_lists(LDS_LIMIT_SYMBOLS + 1, 100)
    assert len({c for s in tl for c in s}) == LDS_LIMIT_SYMBOLS + 1 > 7679 and min(map(len, fl)) <= 32
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for name in SCORERS:
        d = lev_oracle.matrix(fl, tl, name)
        ctx.prof_enable(True)
        ctx.prof_reset()
        try:
            for thr in (0.0, 0.3, 0.5, 1.0):
                _assert_join(_lib.lev_join(ctx, f, t, name, thr, capacity=len(fl) * len(tl)), _want(fl, tl, d, thr), f"{name} t={thr}")
            ctx.sync()
            assert _launches(ctx, "k11_join") == 4 and _launches(ctx, "k11_join_general") == 4
        finally:
            ctx.prof_enable(False)
        assert 10 <= (lev_oracle.sim_matrix(fl, tl, d) >= 0.5).sum() < 200


def _abandon_lists():
    """128 to-strings of ONE length (two groups, every lane walks the same 60 steps): near-duplicates of a base sentence, strings
    that share its first 30 to 50 characters and then diverge, and strangers; the from-strings are the base and edited copies"""
    rng = np.random.default_rng(113)
    alpha = "abcdefghijklmnopqrstuvwxyz "
    base = "the quick brown fox jumps over the lazy dog and runs far away"[:60]
    tl = []
    for k in range(128):
        if k % 3 == 0:
            s = _edited(rng, base, alpha, int(rng.integers(0, 6)))
        elif k % 3 == 1:
            s = base[:int(rng.integers(30, 51))] + _rand(rng, "xyzw", 40, 40, 1)[0]
        else:
            s = _rand(rng, alpha, 60, 60, 1)[0]
        tl.append((s + "q" * 60)[:60])
    fl = [base] + [(_edited(rng, base, alpha, int(rng.integers(1, 5))) + "q" * 60)[:int(rng.integers(56, 61))] for _ in range(11)]
    return fl, tl


@pytest.mark.parametrize("name", SCORERS)
def test_lanes_abandoned_mid_walk(ctx, name):
    """a group in which some lanes die early (strangers), some late (a long common prefix, then divergence) and some finish
    (near-duplicates): the hits are the oracle's, and the counters show all three -- every pair is inside the length window, fewer
    are finished, and the live lanes took fewer steps than the pairs have to-characters"""
    from polyfuzz_amd import _lib
    fl, tl = _abandon_lists()
    d = lev_oracle.matrix(fl, tl, name)
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for thr in (0.8, 0.9, 0.5):
        *got, work = _lib.lev_join(ctx, f, t, name, thr, counters=True)
        want = _want(fl, tl, d, thr)
        _assert_join(got, want, f"{name} t={thr}")
        n_pairs, all_steps = len(fl) * len(tl), len(fl) * sum(map(len, tl))
        print(f"K11 abandon {name} t={thr}: window {work['pairs_in_window']} finished {work['pairs_finished']} of {n_pairs} pairs, "
              f"steps {work['steps']} of {all_steps}, hits {len(want[1])}")
        assert work["pairs_in_window"] == n_pairs                 # lengths 56 .. 60 against 60: no length bound is below 0.9
        assert len(want[1]) <= work["pairs_finished"] < n_pairs and work["steps"] < all_steps
        assert work["steps"] >= 60 * work["pairs_finished"]
    assert 20 < len(_want(fl, tl, d, 0.8)[1]) < n_pairs // 2


def _raw_join(ctx, f, t, scorer, thr, cap, n_from, counters=False):
    """pfz_lev_join itself, with 8 guard words behind every buffer: (rc, total, row_ptr, idx, dist, sim[, work]) -- whole buffers"""
    from polyfuzz_amd import _lib
    row_ptr = np.full(n_from + 1 + 8, -7, np.int64)
    idx, dist, sim = np.full(cap + 8, -7, np.int32), np.full(cap + 8, -7, np.int32), np.full(cap + 8, -7.0, np.float64)
    total = ctypes.c_int64(-7)
    work = np.full(3 + 8, -7, np.int64) if counters else None
    rc = ctx.lib.pfz_lev_join(ctx.h, f.h, None if t is None else t.h, scorer, ctypes.c_double(thr), cap, _lib._ptr(row_ptr), _lib._ptr(idx),
                              _lib._ptr(dist), _lib._ptr(sim), ctypes.byref(total), _lib._ptr(work))
    return (rc, total.value, row_ptr, idx, dist, sim) + ((work,) if counters else ())


def test_capacity_total_and_guard_words(ctx, classes):
    """capacity = total, total - 1, 1 and 0 through pfz_lev_join: the total is exact every time; with room, exactly `total`
    entries and n + 1 row pointers are written and not a word behind them; without, the call says so through the total and
    writes none of the four arrays; the binding's one repeat then returns the full result.  Bad arguments: PFZ_ERR_INVALID."""
    from polyfuzz_amd import _lib
    alpha, fl, tl, want_d = classes
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    n = len(fl)
    for scorer, name in enumerate(SCORERS):
        want = _want(fl, tl, want_d[name], 0.5)
        total = len(want[1])
        assert total > 3
        for cap in (total, total + 5, total - 1, 1, 0):
            rc, got_total, row_ptr, idx, dist, sim = _raw_join(ctx, f, t, scorer, 0.5, cap, n)
            assert rc == 0 and got_total == total, (name, cap, rc, got_total)
            if cap >= total:
                _assert_join((row_ptr[:n + 1], idx[:total], dist[:total], sim[:total]), want, f"{name} capacity {cap}")
                assert (row_ptr[n + 1:] == -7).all() and (idx[total:] == -7).all() and (dist[total:] == -7).all() and (sim[total:] == -7.0).all()
            else:
                assert (row_ptr == -7).all() and (idx == -7).all() and (dist == -7).all() and (sim == -7.0).all(), (name, cap)
        for cap in (1, 0, total - 1, total):
            _assert_join(_lib.lev_join(ctx, f, t, name, 0.5, capacity=cap), want, f"{name} binding, capacity {cap}")
    for scorer, thr, cap in ((2, 0.5, 4), (-1, 0.5, 4), (0, float("nan"), 4), (0, 1.5, 4), (1, -0.25, 4), (0, float("inf"), 4), (0, 0.5, -1)):
        row_ptr, idx, dist, sim = np.zeros(n + 1, np.int64), np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(4)
        total = ctypes.c_int64(0)
        rc = ctx.lib.pfz_lev_join(ctx.h, f.h, t.h, scorer, ctypes.c_double(thr), cap, _lib._ptr(row_ptr), _lib._ptr(idx), _lib._ptr(dist),
                                  _lib._ptr(sim), ctypes.byref(total), None)
        assert rc == -1, (scorer, thr, cap, rc)
    with pytest.raises(KeyError):
        _lib.lev_join(ctx, f, t, "jaro", 0.5)
    # empty lists
    e = _lib.DeviceStrings.upload(ctx, [])
    for a, b, rows in ((e, t, 0), (f, e, n), (e, None, 0)):
        row_ptr, idx, dist, sim = _lib.lev_join(ctx, a, b, "osa", 0.0)
        assert row_ptr.tolist() == [0] * (rows + 1) and len(idx) == len(dist) == len(sim) == 0


def _self_list():
    """~200 strings of mixed lengths 0 .. 70 (four groups) with many repeats, '' three times, and near-duplicates; scattered"""
    rng = np.random.default_rng(114)
    uniq = _rand(rng, "ab", 0, 12, 40) + _rand(rng, "abcdefgh", 5, 70, 50)
    sl = uniq + [uniq[int(k)] for k in rng.integers(0, len(uniq), 50)] + ["", "", ""] + \
        [_edited(rng, uniq[int(k)], "abcdefgh", int(rng.integers(1, 4))) for k in rng.integers(40, len(uniq), 55)] + [uniq[60] + "z" * 40]
    return [sl[k] for k in rng.permutation(len(sl))]


@pytest.mark.parametrize("name", SCORERS)
def test_self_join(ctx, name):
    """to_strings NULL, and the from-list's own handle: each unordered pair once, as (i, j) with i < j, never (i, i), equal
    strings at different positions included -- the oracle's upper triangle, and the two-list result of the list against a second
    upload of itself filtered to i < j.  Counters: the pairs inside the window are the OWNED ones (each unordered pair counted
    once) whose length bound passes; at t = 0 all n (n - 1) / 2 are finished."""
    from polyfuzz_amd import _lib
    sl = _self_list()
    n = len(sl)
    assert 190 <= n <= 210 and len(set(sl)) < n - 40 and sl.count("") >= 3 and max(map(len, sl)) > 64
    d = lev_oracle.matrix(sl, sl, name)
    f, f2 = _lib.DeviceStrings.upload(ctx, sl), _lib.DeviceStrings.upload(ctx, sl)
    ln = lev_oracle.lengths(sl)
    bound = lev_oracle.similarity(np.abs(ln[:, None] - ln[None, :]), ln[:, None], ln[None, :])
    upper = np.triu(np.ones((n, n), bool), 1)
    for thr in THRESHOLDS:
        want = _want(sl, sl, d, thr, self_join=True)
        *got, work = _lib.lev_join(ctx, f, None, name, thr, counters=True)
        _assert_join(got, want, f"{name} self t={thr!r}")
        _assert_join(_lib.lev_join(ctx, f, f, name, thr), want, f"{name} self (own handle) t={thr!r}")
        row_ptr, idx, dist, sim = _lib.lev_join(ctx, f, f2, name, thr)
        rows = np.repeat(np.arange(n), np.diff(row_ptr))
        keep = rows < idx
        np.testing.assert_array_equal(rows[keep], np.repeat(np.arange(n), np.diff(want[0])))
        _assert_join((idx[keep], dist[keep], sim[keep]), want[1:], f"{name} two-list, filtered, t={thr!r}")
        assert len(idx) == 2 * len(want[1]) + n                   # (both orders and the diagonal)
        assert work["pairs_in_window"] == int(((bound >= thr) & upper).sum()), (name, thr)
        assert len(want[1]) <= work["pairs_finished"] <= work["pairs_in_window"]
        if thr == 0.0:
            assert work["pairs_finished"] == n * (n - 1) // 2 == len(want[1])
            assert work["steps"] == int((np.maximum(ln[:, None], ln[None, :]) * upper).sum())      # the owner is the shorter: it walks the longer
    eq = np.array([[a == b for b in sl] for a in sl]) & upper
    assert eq.sum() > 50 and len(_want(sl, sl, d, 1.0, self_join=True)[1]) == eq.sum()


@pytest.mark.parametrize("name", SCORERS)
def test_counters_two_lists(ctx, classes, name):
    """pairs_in_window == #{(i, j): lev_length_bound(la, lb) >= t}, from the lengths alone; finished <= window; at t = 0 every
    pair is finished and the steps are every to-character of every pair"""
    from polyfuzz_amd import _lib
    alpha, fl, tl, want_d = classes
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    la, lb = lev_oracle.lengths(fl)[:, None], lev_oracle.lengths(tl)[None, :]
    bound = lev_oracle.similarity(np.abs(la - lb), la, lb)
    for thr in THRESHOLDS:
        *got, work = _lib.lev_join(ctx, f, t, name, thr, counters=True)
        hits = len(got[1])
        assert work["pairs_in_window"] == int((bound >= thr).sum()), (name, thr, work)
        assert hits <= work["pairs_finished"] <= work["pairs_in_window"], (name, thr, work)
        if thr == 0.0:
            assert work["pairs_finished"] == len(fl) * len(tl) and work["steps"] == len(fl) * int(lb.sum())
        if thr == 1.0:
            assert work["pairs_in_window"] == int((la == lb).sum())


def test_determinism(ctx, classes):
    """the same call three times: byte-identical arrays (the appends race, the sort of distinct keys forgets it)"""
    from polyfuzz_amd import _lib
    alpha, fl, tl, want_d = classes
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for to in (t, None):
        runs = [_lib.lev_join(ctx, f, to, "osa", 0.25) for _ in range(3)]
        assert len(runs[0][1]) > 0
        for other in runs[1:]:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(runs[0], other))


def test_matcher_and_single_linkage(ctx):
    """EditDistance.join: the frame From, To, Similarity == the oracle's pairs in (from-index, to-index) order, unrounded and NOT
    normalised whatever `normalize` says; the self-join form; and the frame goes through single_linkage, which then finds a
    cluster of three near-duplicates that no single best partner per string need chain"""
    from polyfuzz_amd.linkage import single_linkage
    from polyfuzz_amd.models import EditDistance
    rng = np.random.default_rng(115)
    tl = ["acme holdings ltd", "acme holding ltd", "acme holdings ltd.", "globex corp", "globex corporation", "initech", "", "umbrella"] + \
        _rand(rng, "abcdefgh ", 5, 40, 60)
    fl = ["acme holdings ltd", "globex corp.", "initech", "", "zzzz"] + [_edited(rng, s, "abcdefgh ", 2) for s in tl[8:40]]
    for name in SCORERS:
        d = lev_oracle.matrix(fl, tl, name)
        for normalize in (True, False):
            for thr in (0.8, 0.5, 1.0):
                row_ptr, idx, _, sim = _want(fl, tl, d, thr)
                rows = np.repeat(np.arange(len(fl)), np.diff(row_ptr))
                want = pd.DataFrame({"From": [fl[i] for i in rows], "To": [tl[j] for j in idx], "Similarity": sim})
                got = EditDistance(scorer=name, normalize=normalize).join(fl, tl, thr)
                assert list(got.columns) == ["From", "To", "Similarity"] and got["Similarity"].dtype == np.float64
                pd.testing.assert_frame_equal(got, want, check_exact=True)
        assert "zzzz" not in set(EditDistance(scorer=name).join(fl, tl, 0.5)["From"])          # no partner: no row
        # default threshold, self-join
        ds = lev_oracle.matrix(tl, tl, name)
        row_ptr, idx, _, sim = _want(tl, tl, ds, 0.8, self_join=True)
        rows = np.repeat(np.arange(len(tl)), np.diff(row_ptr))
        got = EditDistance(scorer=name).join(tl)
        pd.testing.assert_frame_equal(got, pd.DataFrame({"From": [tl[i] for i in rows], "To": [tl[j] for j in idx], "Similarity": sim}),
                                      check_exact=True)
        clusters, mapping, names = single_linkage(got, 0.85)
        acme = {"acme holdings ltd", "acme holding ltd", "acme holdings ltd."}
        assert len({mapping[s] for s in acme}) == 1 and acme <= set(clusters[mapping["acme holdings ltd"]])
        assert "initech" not in mapping


def test_title_width_fixture_and_matrix_arm(ctx):
    """the 2 000 rows of tests/golden/c3_lev_join_oracle.npz against all 20 000 titles, at the fixture's floor, 0.8 and 0.9: the
    pairs, distances and scores == the fixture's (a join at t >= floor is the fixture filtered by `similarity >= t`).  Second arm,
    independent of every pruning rule of K11: the same rows through _lib.lev_matrix -- every pair walked by K9 -- thresholded on
    the host."""
    from polyfuzz_amd import _lib, datasets
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c3_lev_join_oracle.npz"))
    fl, tl = datasets.c3_lists()
    rows, floor = g["rows"], float(g["floor"])
    assert len(fl) == len(tl) == 20_000 and str(g["source"]) == "oracle" and len(rows) == 2000
    sub = [fl[i] for i in rows]
    f, t = _lib.DeviceStrings.upload(ctx, sub), _lib.DeviceStrings.upload(ctx, tl)
    la, lb = lev_oracle.lengths(sub), lev_oracle.lengths(tl)
    for name in SCORERS:
        i, j, d = (g[f"{k}_{name}"] for k in ("from", "to", "distance"))
        sim = lev_oracle.similarity(d, la[i], lb[j])
        got = {}
        for thr in (floor, 0.8, 0.9):
            keep = sim >= thr
            row_ptr = np.zeros(len(rows) + 1, np.int64)
            np.cumsum(np.bincount(i[keep], minlength=len(rows)), out=row_ptr[1:])
            *got[thr], work = _lib.lev_join(ctx, f, t, name, thr, counters=True)
            _assert_join(got[thr], (row_ptr, j[keep], d[keep], sim[keep]), f"{name} fixture t={thr}")
            n_pairs, all_steps = len(rows) * len(tl), len(rows) * int(lb.sum())
            print(f"K11 fixture rows {name} t={thr}: hits {int(keep.sum())}, in window {work['pairs_in_window'] / n_pairs:.4f}, finished "
                  f"{work['pairs_finished'] / n_pairs:.4f} of the pairs, steps {work['steps'] / all_steps:.4f} of all steps")
        # every pair walked by K9, in shards of 500 rows; thresholded here
        parts = {thr: [] for thr in got}
        for b in range(0, len(rows), 500):
            dm = _lib.lev_matrix(ctx, f, t, name, b, b + 500)
            sm = lev_oracle.similarity(dm, la[b:b + 500, None], lb[None, :])
            for thr in got:
                ii, jj = np.nonzero(sm >= thr)
                parts[thr].append((ii + b, jj, dm[ii, jj], sm[ii, jj]))
        for thr in got:
            ii, jj, dd, ss = (np.concatenate([p[k] for p in parts[thr]]) for k in range(4))
            row_ptr = np.zeros(len(rows) + 1, np.int64)
            np.cumsum(np.bincount(ii, minlength=len(rows)), out=row_ptr[1:])
            _assert_join(got[thr], (row_ptr, jj.astype(np.int32), dd.astype(np.int32), ss), f"{name} matrix arm t={thr}")
