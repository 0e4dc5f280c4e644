"""GPU parity of K13's join (every pair at or above an Indel similarity, as CSR) against the definition (tests/indel_oracle.py:
the textbook LCS table) thresholded on the host -- `sim >= t` on sim_matrix, row-major, i < j for the self-join: every comparison
is exact, == on indices, on int32 distances and on float64 scores.  The lists are tests/test_join_gpu.py's: they sit on every
border of the word classes, the groups and the window."""
import ctypes

import numpy as np
import pytest

from tests import indel_oracle
from tests.test_join_gpu import FROM_LENGTHS, TO_SIZES, _abandon_lists, _assert_join, _class_lists, _launches, _self_list

pytestmark = pytest.mark.gpu

ATT = float(indel_oracle.similarity(4, 6, 4))          # "ababab" against "abab": attained exactly
# every pair; equal strings only; two everyday cut-offs; a score pairs DO attain (kept) and the next float64 (dropped)
THRESHOLDS = (0.0, 1.0, 0.5, 0.8, ATT, float(np.nextafter(ATT, 2.0)))


def _want(fl, tl, lcs, thr, self_join=False):
    """(row_ptr, idx, dist, sim) of the pairs with sim >= thr, row-major; self_join: i < j only"""
    sim = indel_oracle.sim_matrix(fl, tl, lcs)
    keep = sim >= thr
    if self_join:
        keep &= np.triu(np.ones(keep.shape, bool), 1)
    i, j = np.nonzero(keep)
    row_ptr = np.zeros(len(fl) + 1, np.int64)
    np.cumsum(np.bincount(i, minlength=len(fl)), out=row_ptr[1:])
    la, lb = indel_oracle.lengths(fl), indel_oracle.lengths(tl)
    return row_ptr, j.astype(np.int32), indel_oracle.distance(lcs[i, j], la[i], lb[j]), sim[i, j]


def _bound(la, lb):
    """the length bound: the similarity of lcs = min(la, lb)"""
    return indel_oracle.similarity(np.minimum(la, lb), la, lb)


@pytest.fixture(scope="module", params=("ab", "wide"))
def classes(request):
    fl, tl = _class_lists(request.param)
    return request.param, fl, tl, indel_oracle.lcs_matrix(fl, tl)


def test_word_classes_thresholds_and_to_list_sizes(ctx, classes):
    """~33 from-strings of lengths 0, 1, 31 .. 33, 63 .. 65 and 130 (32-bit words, 64-bit words, the general kernel) against
    to-lists of 1, 63, 64, 65 and 300 strings of lengths 0 .. 130, at every threshold of THRESHOLDS.  Capacity left to the binding
    (its guess, and one repeat where the guess is short)."""
    from polyfuzz_amd import _lib
    alpha, fl, tl, lcs = classes
    assert len({c for s in tl for c in s}) > 256 if alpha == "wide" else len({c for s in tl for c in s}) == 2
    assert set(FROM_LENGTHS) <= set(map(len, fl))
    f = _lib.DeviceStrings.upload(ctx, fl)
    for n_to in TO_SIZES:
        t = _lib.DeviceStrings.upload(ctx, tl[:n_to])
        ctx.prof_enable(True)
        ctx.prof_reset()
        try:
            for thr in THRESHOLDS:
                _assert_join(_lib.indel_join(ctx, f, t, thr), _want(fl, tl[:n_to], lcs[:, :n_to], thr), f"{alpha} n_to={n_to} t={thr!r}")
            ctx.sync()
            calls = _launches(ctx, "k13_join")                                     # (one per call; a short guess costs one repeat)
            assert len(THRESHOLDS) <= calls <= 2 * len(THRESHOLDS)
            assert _launches(ctx, "k13_join_general") == calls                     # (the from-strings of 65 and 130 characters)
        finally:
            ctx.prof_enable(False)
    sim = indel_oracle.sim_matrix(fl, tl, lcs)
    full = _want(fl, tl, lcs, 0.0)
    assert len(full[1]) == len(fl) * len(tl)
    assert sim[fl.index(""), tl.index("")] == 1.0 and (sim == 1.0).sum() >= 6
    assert ATT == 0.8 and sim[fl.index("ababab"), tl.index("abab")] == ATT         # attained exactly: kept at t, dropped just above
    if alpha == "ab":
        assert (sim >= 0.5).sum() > 300 and ((sim >= 0.8) & (sim < 1.0)).sum() >= 3 and (sim == ATT).sum() >= 1
    else:
        assert (sim >= 0.5).sum() < 100


def test_general_kernel_by_table_size(ctx):
    """one code point more than the 60 KiB table holds: every from-string, however short, is the general kernel's"""
    from polyfuzz_amd import _lib
    from tests.test_jaro_gpu import LDS_LIMIT_SYMBOLS, lds_limit_lists
    fl, tl = lds_limit_lists(LDS_LIMIT_SYMBOLS + 1, 100)
    assert len({c for s in tl for c in s}) == LDS_LIMIT_SYMBOLS + 1 > 7679 and min(map(len, fl)) <= 32
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    lcs = indel_oracle.lcs_matrix(fl, tl)
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        for thr in (0.0, 0.3, 0.5, 1.0):
            _assert_join(_lib.indel_join(ctx, f, t, thr, capacity=len(fl) * len(tl)), _want(fl, tl, lcs, thr), f"t={thr}")
        ctx.sync()
        assert _launches(ctx, "k13_join") == 4 and _launches(ctx, "k13_join_general") == 4
    finally:
        ctx.prof_enable(False)
    assert len(_want(fl, tl, lcs, 0.5)[1]) > 0


def test_lanes_abandoned_mid_walk(ctx):
    """a group in which some lanes die early (strangers), some late (a long common prefix, then divergence) and some finish
    (near-duplicates): the hits are the oracle's, and the counters show all three"""
    from polyfuzz_amd import _lib
    fl, tl = _abandon_lists()
    lcs = indel_oracle.lcs_matrix(fl, tl)
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    la, lb = indel_oracle.lengths(fl)[:, None], indel_oracle.lengths(tl)[None, :]
    n_pairs, all_steps = len(fl) * len(tl), len(fl) * sum(map(len, tl))
    assert (_bound(la, lb) >= 0.9).all()                          # lengths 56 .. 60 against 60
    for thr in (0.8, 0.9, 0.95):
        *got, work = _lib.indel_join(ctx, f, t, thr, counters=True)
        want = _want(fl, tl, lcs, thr)
        _assert_join(got, want, f"t={thr}")
        print(f"K13 abandon t={thr}: window {work['pairs_in_window']} finished {work['pairs_finished']} of {n_pairs} pairs, "
              f"steps {work['steps']} of {all_steps}, hits {len(want[1])}")
        assert work["pairs_in_window"] == int((_bound(la, lb) >= thr).sum())
        if thr <= 0.9:
            assert work["pairs_in_window"] == n_pairs
        assert len(want[1]) <= work["pairs_finished"] < n_pairs and work["steps"] < all_steps
        assert work["steps"] >= 60 * work["pairs_finished"]
    assert 20 < len(_want(fl, tl, lcs, 0.8)[1]) < n_pairs // 2


def _raw_join(ctx, f, t, thr, cap, n_from):
    """pfz_indel_join itself, with 8 guard words behind every buffer: (rc, total, row_ptr, idx, dist, sim) -- whole buffers"""
    from polyfuzz_amd import _lib
    row_ptr = np.full(n_from + 1 + 8, -7, np.int64)
    idx, dist, sim = np.full(cap + 8, -7, np.int32), np.full(cap + 8, -7, np.int32), np.full(cap + 8, -7.0, np.float64)
    total = ctypes.c_int64(-7)
    rc = ctx.lib.pfz_indel_join(ctx.h, f.h, None if t is None else t.h, ctypes.c_double(thr), cap, _lib._ptr(row_ptr), _lib._ptr(idx),
                                _lib._ptr(dist), _lib._ptr(sim), ctypes.byref(total), None)
    return rc, total.value, row_ptr, idx, dist, sim


def test_capacity_total_and_guard_words(ctx, classes):
    """capacity = total, total + 5, total - 1, 1 and 0 through pfz_indel_join: the total is exact every time; with room, exactly
    `total` entries and n + 1 row pointers are written and not a word behind them; without, the call says so through the total
    and writes none of the four arrays; the binding's one repeat then returns the full result.  Bad arguments: PFZ_ERR_INVALID."""
    from polyfuzz_amd import _lib
    alpha, fl, tl, lcs = classes
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    n = len(fl)
    want = _want(fl, tl, lcs, 0.5)
    total = len(want[1])
    assert total > 3
    for cap in (total, total + 5, total - 1, 1, 0):
        rc, got_total, row_ptr, idx, dist, sim = _raw_join(ctx, f, t, 0.5, cap, n)
        assert rc == 0 and got_total == total, (cap, rc, got_total)
        if cap >= total:
            _assert_join((row_ptr[:n + 1], idx[:total], dist[:total], sim[:total]), want, f"capacity {cap}")
            assert (row_ptr[n + 1:] == -7).all() and (idx[total:] == -7).all() and (dist[total:] == -7).all() and (sim[total:] == -7.0).all()
        else:
            assert (row_ptr == -7).all() and (idx == -7).all() and (dist == -7).all() and (sim == -7.0).all(), cap
    for cap in (1, 0, total - 1, total):
        _assert_join(_lib.indel_join(ctx, f, t, 0.5, capacity=cap), want, f"binding, capacity {cap}")
    for thr, cap in ((float("nan"), 4), (1.5, 4), (-0.25, 4), (float("inf"), 4), (0.5, -1)):
        row_ptr, idx, dist, sim = np.zeros(n + 1, np.int64), np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(4)
        tot = ctypes.c_int64(0)
        rc = ctx.lib.pfz_indel_join(ctx.h, f.h, t.h, ctypes.c_double(thr), cap, _lib._ptr(row_ptr), _lib._ptr(idx), _lib._ptr(dist),
                                    _lib._ptr(sim), ctypes.byref(tot), None)
        assert rc == -1, (thr, cap, rc)
    # empty lists
    e = _lib.DeviceStrings.upload(ctx, [])
    for a, b, rows in ((e, t, 0), (f, e, n), (e, None, 0)):
        row_ptr, idx, dist, sim = _lib.indel_join(ctx, a, b, 0.0)
        assert row_ptr.tolist() == [0] * (rows + 1) and len(idx) == len(dist) == len(sim) == 0


def test_self_join(ctx):
    """to_strings NULL, and the from-list's own handle: each unordered pair once, as (i, j) with i < j -- the oracle's upper
    triangle, and the two-list result of the list against a second upload of itself filtered to i < j.  Counters: the pairs inside
    the window are the OWNED ones whose length bound passes; at t = 0 all n (n - 1) / 2 are finished."""
    from polyfuzz_amd import _lib
    sl = _self_list()
    n = len(sl)
    assert 190 <= n <= 210 and len(set(sl)) < n - 40 and sl.count("") >= 3 and max(map(len, sl)) > 64
    lcs = indel_oracle.lcs_matrix(sl, sl)
    f, f2 = _lib.DeviceStrings.upload(ctx, sl), _lib.DeviceStrings.upload(ctx, sl)
    ln = indel_oracle.lengths(sl)
    bound = _bound(ln[:, None], ln[None, :])
    upper = np.triu(np.ones((n, n), bool), 1)
    for thr in THRESHOLDS:
        want = _want(sl, sl, lcs, thr, self_join=True)
        *got, work = _lib.indel_join(ctx, f, None, thr, counters=True)
        _assert_join(got, want, f"self t={thr!r}")
        _assert_join(_lib.indel_join(ctx, f, f, thr), want, f"self (own handle) t={thr!r}")
        row_ptr, idx, dist, sim = _lib.indel_join(ctx, f, f2, thr)
        rows = np.repeat(np.arange(n), np.diff(row_ptr))
        keep = rows < idx
        np.testing.assert_array_equal(rows[keep], np.repeat(np.arange(n), np.diff(want[0])))
        _assert_join((idx[keep], dist[keep], sim[keep]), want[1:], f"two-list, filtered, t={thr!r}")
        assert len(idx) == 2 * len(want[1]) + n                   # (both orders and the diagonal)
        assert work["pairs_in_window"] == int(((bound >= thr) & upper).sum()), thr
        assert len(want[1]) <= work["pairs_finished"] <= work["pairs_in_window"]
        if thr == 0.0:
            assert work["pairs_finished"] == n * (n - 1) // 2 == len(want[1])
            assert work["steps"] == int((np.maximum(ln[:, None], ln[None, :]) * upper).sum())      # the owner is the shorter: it walks the longer
    eq = np.array([[a == b for b in sl] for a in sl]) & upper
    assert eq.sum() > 50 and len(_want(sl, sl, lcs, 1.0, self_join=True)[1]) == eq.sum()
    assert len(_want(sl, sl, lcs, 0.5, self_join=True)[1]) > len(_want(sl, sl, lcs, 0.8, self_join=True)[1]) > eq.sum()


def test_counters_two_lists(ctx, classes):
    """pairs_in_window == #{(i, j): indel_similarity(min(la, lb), la, lb) >= t}, from the lengths alone; finished <= window; at
    t = 0 every pair is finished and the steps are every to-character of every pair"""
    from polyfuzz_amd import _lib
    alpha, fl, tl, lcs = classes
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    la, lb = indel_oracle.lengths(fl)[:, None], indel_oracle.lengths(tl)[None, :]
    bound = _bound(la, lb)
    for thr in THRESHOLDS:
        *got, work = _lib.indel_join(ctx, f, t, thr, counters=True)
        hits = len(got[1])
        assert work["pairs_in_window"] == int((bound >= thr).sum()), (thr, work)
        assert hits <= work["pairs_finished"] <= work["pairs_in_window"], (thr, work)
        if thr == 0.0:
            assert work["pairs_finished"] == len(fl) * len(tl) and work["steps"] == len(fl) * int(lb.sum())
        if thr == 1.0:
            assert work["pairs_in_window"] == int((la == lb).sum())


def test_determinism(ctx, classes):
    """the same call three times: byte-identical arrays (the appends race, the sort of distinct keys forgets it)"""
    from polyfuzz_amd import _lib
    alpha, fl, tl, lcs = classes
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for to in (t, None):
        runs = [_lib.indel_join(ctx, f, to, 0.25) for _ in range(3)]
        assert len(runs[0][1]) > 0
        for other in runs[1:]:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(runs[0], other))


def test_title_width_against_k4_matrix(ctx):
    """the first 1 000 rows of the title lists against all 20 000 titles at 0.6, 0.8 and 0.9 == the same rows through
    _lib.indel_matrix -- every pair walked by K4, which shares none of K13's pruning -- in shards of 500: the LCS recovered from
    each ratio (_lib.indel_lcs_of_ratio, verified bit for bit), the definition thresholded on the host"""
    from polyfuzz_amd import _lib, datasets
    fl, tl = datasets.c3_lists()
    assert len(fl) == len(tl) == 20_000
    sub = fl[:1000]
    f, t = _lib.DeviceStrings.upload(ctx, sub), _lib.DeviceStrings.upload(ctx, tl)
    la, lb = indel_oracle.lengths(sub), indel_oracle.lengths(tl)
    thresholds = (0.6, 0.8, 0.9)
    parts = {thr: [] for thr in thresholds}
    for b in range(0, len(sub), 500):
        ratio = _lib.indel_matrix(ctx, f, t, b, b + 500)
        s = la[b:b + 500, None].astype(np.int64) + lb[None, :]
        lcs = _lib.indel_lcs_of_ratio(ratio, s)
        sm = indel_oracle.similarity(lcs, la[b:b + 500, None], lb[None, :])
        for thr in thresholds:
            ii, jj = np.nonzero(sm >= thr)
            parts[thr].append((ii + b, jj, indel_oracle.distance(lcs[ii, jj], la[ii + b], lb[jj]), sm[ii, jj]))
    n_pairs, all_steps = len(sub) * len(tl), len(sub) * int(lb.sum())
    for thr in thresholds:
        ii, jj, dd, ss = (np.concatenate([p[k] for p in parts[thr]]) for k in range(4))
        row_ptr = np.zeros(len(sub) + 1, np.int64)
        np.cumsum(np.bincount(ii, minlength=len(sub)), out=row_ptr[1:])
        *got, work = _lib.indel_join(ctx, f, t, thr, counters=True)
        _assert_join(got, (row_ptr, jj.astype(np.int32), dd.astype(np.int32), ss), f"matrix arm t={thr}")
        assert len(jj) > 0
        print(f"K13 title rows t={thr}: hits {len(jj)}, in window {work['pairs_in_window'] / n_pairs:.4f}, finished "
              f"{work['pairs_finished'] / n_pairs:.4f} of the pairs, steps {work['steps'] / all_steps:.4f} of all steps")
