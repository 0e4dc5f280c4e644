"""GPU parity of K20 (models.JaroWinkler.join: every pair at or above a Jaro / Jaro-Winkler score, as CSR) against the definition
(oracle/jaro.c == tests/jaro_oracle.py, bit for bit) thresholded on the host -- `score >= t` on the matrix, row-major, i < j for the
self-join: every comparison is exact, == on indices and on float64 scores."""
import ctypes

import numpy as np
import pandas as pd
import pytest

from tests.test_jaro_join_cpu import host_lib, window_pairs
from tests.test_join_gpu import _abandon_lists, _assert_join, _class_lists, _launches, _self_list

pytestmark = pytest.mark.gpu

SCORERS = ("jaro", "jaro_winkler")
TO_SIZES = (1, 63, 64, 65, 300)


def _want(m, thr, self_join=False):
    """(row_ptr, idx, score) of the pairs of the score matrix m with score >= thr, row-major; self_join: i < j only"""
    keep = m >= thr
    if self_join:
        keep &= np.triu(np.ones(keep.shape, bool), 1)
    i, j = np.nonzero(keep)
    row_ptr = np.zeros(m.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(i, minlength=m.shape[0]), out=row_ptr[1:])
    return row_ptr, j.astype(np.int32), m[i, j]


def _attained(m):
    """a score strictly between 0.8 and 1 that pairs of the matrix DO attain (kept at t, dropped at the next float64)"""
    return float(np.sort(m[(m > 0.8) & (m < 1.0)])[0])


def _long_strings(alpha_name):
    """to-strings of 255, 256, 257 and 300 characters: the last two are beyond the register kernels' four flag words"""
    rng = np.random.default_rng(121)
    alpha = "ab" if alpha_name == "ab" else "".join(chr(0x400 + k) for k in range(300))
    return ["".join(rng.choice(list(alpha), size=n)) for n in (255, 256, 257, 300)]


def class_lists(alpha_name):
    """the lists of the `classes` fixture (tests/test_jaro_sweep_gpu.py records the work of K20 and K21 on them)"""
    fl, tl = _class_lists(alpha_name)
    tl = tl + _long_strings(alpha_name)
    # from-strings of <= 64 that share their start with a to-string beyond 256, and two long near-copies of such to-strings
    fl = fl + [tl[-1][:64], tl[-2][:40], tl[-1][1:], tl[-3][:-2]]
    return fl, tl


@pytest.fixture(scope="module", params=("ab", "wide"))
def classes(request, oracle_mod):
    fl, tl = class_lists(request.param)
    return request.param, fl, tl, {name: oracle_mod.jaro_matrix(fl, tl, name) for name in SCORERS}


@pytest.mark.parametrize("name", SCORERS)
def test_word_classes_thresholds_and_to_list_sizes(ctx, classes, name):
    """~43 from-strings of lengths 0, 1, 31 .. 33, 63 .. 65 and 130 (32-bit words, 64-bit words, the general kernel) against
    to-lists of 1, 63, 64, 65 and 300 strings of lengths 0 .. 130, and against those 300 with four of 255 .. 300 characters (the
    groups beyond 256, the general kernel's for every from-string): 0.0 is the full matrix, empty strings included; an attained
    score is kept at t and dropped at its float64 successor"""
    from polyfuzz_amd import _lib
    alpha, fl, tl, want_m = classes
    m_all = want_m[name]
    thresholds = (0.0, 1.0, 0.5, 0.8, 0.9, _attained(m_all[:, :300]), float(np.nextafter(_attained(m_all[:, :300]), 2.0)))
    f = _lib.DeviceStrings.upload(ctx, fl)
    for n_to in TO_SIZES + (len(tl),):
        t = _lib.DeviceStrings.upload(ctx, tl[:n_to])
        m = m_all[:, :n_to]
        ctx.prof_enable(True)
        ctx.prof_reset()
        try:
            for thr in thresholds:
                got = _lib.jaro_join(ctx, f, t, name, thr, capacity=m.size)
                _assert_join(got, _want(m, thr), f"{alpha} {name} n_to={n_to} t={thr!r}")
                assert got[2].dtype == np.float64 and got[1].dtype == np.int32
            ctx.sync()
            assert _launches(ctx, "k20_join") == len(thresholds)                   # (the capacity has room: no repeat)
            # the from-strings of 65 and 130 characters; and, with groups beyond 256, the two register classes against those
            assert _launches(ctx, "k20_join_general") == len(thresholds) * (3 if n_to == len(tl) else 1)
        finally:
            ctx.prof_enable(False)
    full = _lib.jaro_join(ctx, f, _lib.DeviceStrings.upload(ctx, tl), name, 0.0)             # (the binding's guess is short: one repeat)
    assert len(full[1]) == len(fl) * len(tl) and np.array_equal(full[2].reshape(len(fl), len(tl)), m_all)
    assert "" in fl and "" in tl and m_all[fl.index(""), tl.index("")] == 0.0
    # the oracle alone: hits strictly between none and all at 0.8 and 0.9, also among the pairs with the long to-strings
    for thr in (0.8, 0.9):
        assert 5 < (m_all >= thr).sum() < m_all.size // 2
    # (a from-string of 64 characters against the 300 it begins: all 64 matched, (1 + 64 / 300 + 1) / 3 -- a hit of the general
    # kernel's launch for the register rows at 0.5, outside every window from 0.8 on)
    assert 0.7 < m_all[len(fl) - 4, len(tl) - 1] < 0.85 and (m_all[:, 300:] >= 0.5).sum() > 4 and (m_all[:, 300:] >= 0.9).sum() >= 1
    if alpha == "ab":
        assert (m_all >= 0.9).sum() > 100 and ((m_all >= 0.8) & (m_all < 0.9)).sum() > 1000


def test_general_kernel_by_table_size(ctx, oracle_mod):
    """one code point more than the 60 KiB table holds: every from-string, however short, is the general kernel's"""
    from polyfuzz_amd import _lib
    from tests.test_jaro_gpu import LDS_LIMIT_SYMBOLS, lds_limit_lists
    fl, tl = lds_limit_lists(LDS_LIMIT_SYMBOLS + 1, 100)
    assert len({c for s in tl for c in s}) == LDS_LIMIT_SYMBOLS + 1 > 7679 and min(map(len, fl)) <= 32
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for name in SCORERS:
        m = oracle_mod.jaro_matrix(fl, tl, name)
        ctx.prof_enable(True)
        ctx.prof_reset()
        try:
            for thr in (0.0, 0.3, 0.5, 0.9, 1.0):
                _assert_join(_lib.jaro_join(ctx, f, t, name, thr, capacity=m.size), _want(m, thr), f"{name} t={thr}")
            ctx.sync()
            assert _launches(ctx, "k20_join") == 5 and _launches(ctx, "k20_join_general") == 5
        finally:
            ctx.prof_enable(False)
        assert 0 < (m >= 0.5).sum() < m.size


@pytest.mark.parametrize("name", SCORERS)
def test_lanes_abandoned_mid_sweep(ctx, oracle_mod, name):
    """128 to-strings of one length, some strangers, some that share a long prefix and then diverge, some near-duplicates: the hits
    are the oracle's, and the counters show every stage at work -- hits <= scored <= alive after sweep 1 < window <= pairs, fewer
    sweep-1 steps than the pairs have to-characters, and the window is what the host-compiled length bound admits"""
    from polyfuzz_amd import _lib
    fl, tl = _abandon_lists()
    m = oracle_mod.jaro_matrix(fl, tl, name)
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    host = host_lib()
    n_pairs, all_steps = len(fl) * len(tl), len(fl) * sum(map(len, tl))
    for thr in (0.8, 0.9, 0.95):
        *got, work = _lib.jaro_join(ctx, f, t, name, thr, counters=True)
        want = _want(m, thr)
        _assert_join(got, want, f"{name} t={thr}")
        hits = len(want[1])
        print(f"K20 abandon {name} t={thr}: {work} of {n_pairs} pairs, {all_steps} steps, hits {hits}")
        assert hits <= work["pairs_scored"] <= work["pairs_alive_after_sweep1"] < work["pairs_in_window"] <= n_pairs
        assert 0 < work["steps"] < all_steps
        assert work["pairs_in_window"] == window_pairs(host, map(len, fl), list(map(len, tl)), thr, SCORERS.index(name))
    assert 20 < len(_want(m, 0.9)[1]) < n_pairs // 2


def _raw_join(ctx, f, t, scorer, thr, cap, n_from):
    """pfz_jaro_join itself, with 8 guard words behind every buffer: (rc, total, row_ptr, idx, sim) -- whole buffers"""
    from polyfuzz_amd import _lib
    row_ptr = np.full(n_from + 1 + 8, -7, np.int64)
    idx, sim = np.full(cap + 8, -7, np.int32), np.full(cap + 8, -7.0, np.float64)
    total = ctypes.c_int64(-7)
    rc = ctx.lib.pfz_jaro_join(ctx.h, f.h, None if t is None else t.h, scorer, ctypes.c_double(thr), cap, _lib._ptr(row_ptr), _lib._ptr(idx),
                               _lib._ptr(sim), ctypes.byref(total), None)
    return rc, total.value, row_ptr, idx, sim


def test_capacity_total_and_guard_words(ctx, classes):
    """capacity = total, total + 5, total - 1, 1 and 0 through pfz_jaro_join: the total is exact every time; with room, exactly
    `total` entries and n + 1 row pointers are written and not a word behind them; without, none of the three arrays is written;
    the binding's one repeat then returns the full result.  Bad arguments: PFZ_ERR_INVALID."""
    from polyfuzz_amd import _lib
    alpha, fl, tl, want_m = classes
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    n = len(fl)
    for scorer, name in enumerate(SCORERS):
        want = _want(want_m[name], 0.8)
        total = len(want[1])
        assert total > 6
        for cap in (total, total + 5, total - 1, 1, 0):
            rc, got_total, row_ptr, idx, sim = _raw_join(ctx, f, t, scorer, 0.8, cap, n)
            assert rc == 0 and got_total == total, (name, cap, rc, got_total)
            if cap >= total:
                _assert_join((row_ptr[:n + 1], idx[:total], sim[:total]), want, f"{name} capacity {cap}")
                assert (row_ptr[n + 1:] == -7).all() and (idx[total:] == -7).all() and (sim[total:] == -7.0).all()
            else:
                assert (row_ptr == -7).all() and (idx == -7).all() and (sim == -7.0).all(), (name, cap)
        for cap in (1, 0, total - 1, total):
            _assert_join(_lib.jaro_join(ctx, f, t, name, 0.8, capacity=cap), want, f"{name} binding, capacity {cap}")
    for scorer, thr, cap in ((2, 0.5, 4), (-1, 0.5, 4), (0, float("nan"), 4), (0, 1.5, 4), (1, -0.25, 4), (0, float("inf"), 4), (0, 0.5, -1)):
        row_ptr, idx, sim = np.zeros(n + 1, np.int64), np.zeros(4, np.int32), np.zeros(4)
        total = ctypes.c_int64(0)
        rc = ctx.lib.pfz_jaro_join(ctx.h, f.h, t.h, scorer, ctypes.c_double(thr), cap, _lib._ptr(row_ptr), _lib._ptr(idx), _lib._ptr(sim),
                                   ctypes.byref(total), None)
        assert rc == -1, (scorer, thr, cap, rc)
    with pytest.raises(KeyError):
        _lib.jaro_join(ctx, f, t, "levenshtein", 0.5)
    e = _lib.DeviceStrings.upload(ctx, [])
    for a, b, rows in ((e, t, 0), (f, e, n), (e, None, 0)):
        row_ptr, idx, sim = _lib.jaro_join(ctx, a, b, "jaro", 0.0)
        assert row_ptr.tolist() == [0] * (rows + 1) and len(idx) == len(sim) == 0


@pytest.mark.parametrize("name", SCORERS)
def test_self_join(ctx, oracle_mod, name):
    """to_strings NULL, and the from-list's own handle: each unordered pair once, as (i, j) with i < j -- From the earlier position
    --, never (i, i), equal strings at different positions included: the strict upper triangle of the oracle's matrix.  At t = 0
    every unordered pair is in the window, alive and scored."""
    from polyfuzz_amd import _lib
    sl = _self_list()
    n = len(sl)
    assert 190 <= n <= 210 and len(set(sl)) < n - 40 and sl.count("") >= 3 and max(map(len, sl)) > 64
    m = oracle_mod.jaro_matrix(sl, sl, name)
    f = _lib.DeviceStrings.upload(ctx, sl)
    for thr in (0.0, 1.0, 0.5, 0.8, 0.9, _attained(m), float(np.nextafter(_attained(m), 2.0))):
        want = _want(m, thr, self_join=True)
        *got, work = _lib.jaro_join(ctx, f, None, name, thr, counters=True)
        _assert_join(got, want, f"{name} self t={thr!r}")
        rows = np.repeat(np.arange(n), np.diff(got[0]))
        assert (rows < got[1]).all()
        _assert_join(_lib.jaro_join(ctx, f, f, name, thr), want, f"{name} self (own handle) t={thr!r}")
        assert len(want[1]) <= work["pairs_scored"] <= work["pairs_alive_after_sweep1"] <= work["pairs_in_window"] <= n * (n - 1) // 2
        if thr == 0.0:
            assert work["pairs_scored"] == n * (n - 1) // 2 == len(want[1])
    eq = np.array([[a == b and a != "" for b in sl] for a in sl]) & np.triu(np.ones((n, n), bool), 1)
    assert eq.sum() > 50 and len(_want(m, 1.0, self_join=True)[1]) == eq.sum()      # ('' against '' scores 0.0)


def test_determinism_and_pool_fill(ctx, classes):
    """the same call twice: byte-identical arrays (the appends race, the sort of distinct keys forgets it) -- and the same bytes
    under the allocator's fill words 0x0, 0x1 and 0x0000000100000001"""
    from polyfuzz_amd import _lib
    alpha, fl, tl, want_m = classes
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for to in (t, None):
        a, b = (_lib.jaro_join(ctx, f, to, "jaro_winkler", 0.7) for _ in range(2))
        assert len(a[1]) > 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    seen = []
    try:
        for fill in (_lib.Context.POOL_FILL_ZERO, _lib.Context.POOL_FILL_ONE64, _lib.Context.POOL_FILL_ONE32):
            ctx.pool_fill(fill)
            f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
            got = _lib.jaro_join(ctx, f, t, "jaro_winkler", 0.8) + _lib.jaro_join(ctx, t, None, "jaro", 0.8)
            _assert_join(got[:3], _want(want_m["jaro_winkler"], 0.8), f"fill {fill}")
            seen.append(b"".join(x.tobytes() for x in got))
    finally:
        ctx.pool_fill(0)
    assert seen[0] == seen[1] == seen[2]


@pytest.fixture(scope="module")
def titles(oracle_mod):
    from polyfuzz_amd import datasets
    fl, tl = datasets.c3_lists()
    assert len(fl) == len(tl) == 20_000
    return fl[:256], tl, {name: oracle_mod.jaro_matrix(fl[:256], tl, name) for name in SCORERS}


@pytest.mark.parametrize("name", SCORERS)
def test_title_width(ctx, titles, name):
    """the first 256 titles against all 20 000 at 0.9 and 0.8: the pairs and scores are those of K8's own matrix entry -- every
    pair scored, no pruning rule -- thresholded on the host, and the oracle's"""
    from polyfuzz_amd import _lib
    sub, tl, want_m = titles
    f, t = _lib.DeviceStrings.upload(ctx, sub), _lib.DeviceStrings.upload(ctx, tl)
    k8 = _lib.jaro_matrix(ctx, f, t, name)
    np.testing.assert_array_equal(k8, want_m[name])
    n_pairs, all_steps = len(sub) * len(tl), len(sub) * sum(map(len, tl))
    for thr in (0.9, 0.8):
        *got, work = _lib.jaro_join(ctx, f, t, name, thr, counters=True)
        _assert_join(got, _want(k8, thr), f"{name} titles t={thr} against K8's matrix")
        _assert_join(got, _want(want_m[name], thr), f"{name} titles t={thr} against the oracle")
        print(f"K20 titles {name} t={thr}: hits {len(got[1])}, in window {work['pairs_in_window'] / n_pairs:.4f}, alive after sweep 1 "
              f"{work['pairs_alive_after_sweep1'] / n_pairs:.4f}, scored {work['pairs_scored'] / n_pairs:.5f} of the pairs, steps "
              f"{work['steps'] / all_steps:.4f} of all steps")
        assert 0 < len(got[1]) < n_pairs // 100


def test_matcher_frames(ctx, classes, oracle_mod):
    """JaroWinkler.join: the frame From, To, Similarity == the oracle's pairs in (from-index, to-index) order, column by column,
    unrounded and NOT normalised whatever `normalize` says; the self-join with the default threshold; `match` is EditDistance's"""
    from polyfuzz_amd.models import EditDistance, JaroWinkler
    alpha, fl, tl, want_m = classes
    for name, winkler in (("jaro_winkler", True), ("jaro", False)):
        for normalize in (True, False):
            matcher = JaroWinkler(winkler=winkler, normalize=normalize)
            for thr in (0.8, 0.9, 1.0):
                row_ptr, idx, sim = _want(want_m[name], thr)
                rows = np.repeat(np.arange(len(fl)), np.diff(row_ptr))
                got = matcher.join(fl, tl, thr)
                assert list(got.columns) == ["From", "To", "Similarity"] and got["Similarity"].dtype == np.float64
                assert got["From"].tolist() == [fl[i] for i in rows] and got["To"].tolist() == [tl[j] for j in idx]
                np.testing.assert_array_equal(got["Similarity"].to_numpy(), sim)
                assert set(matcher.last_timings) == {"device", "frame"}
        ms = oracle_mod.jaro_matrix(tl, tl, name)
        row_ptr, idx, sim = _want(ms, 0.9, self_join=True)
        rows = np.repeat(np.arange(len(tl)), np.diff(row_ptr))
        got = JaroWinkler(winkler=winkler).join(tl)
        assert list(got.columns) == ["From", "To", "Similarity"] and got["Similarity"].dtype == np.float64
        assert got["From"].tolist() == [tl[i] for i in rows] and got["To"].tolist() == [tl[j] for j in idx]
        np.testing.assert_array_equal(got["Similarity"].to_numpy(), sim)
        assert len(got) > 0 or alpha == "wide"                 # (over 300 symbols no two of these strings come close)
        pd.testing.assert_frame_equal(JaroWinkler(winkler=winkler).match(fl[3:], tl), EditDistance(scorer=name).match(fl[3:], tl), check_exact=True)
