"""K17 on the GPU: a TF-IDF threshold join left in HBM (pfz_cossim_join_dev) as the blocking key of K16's walk (pfz_pairs_join_keys,
pfz_pairs_components_keys; BlockedEditDistance(blocking_similarity=b).join / .components).  The candidate pairs are K15's -- taken
from the existing pfz_cossim_join --, their scores the oracles' (tests/pairs_join_cases.py all_scores) or, on the hub lists, the
all-pairs kernels' that existing tests hold to the oracles; every comparison is == on row pointers, indices, score bits and labels."""
import ctypes

import numpy as np
import pytest

from tests import blocked_threshold_cases as C
from tests import lev_oracle
from tests import pairs_join_cases as P

pytestmark = pytest.mark.gpu
_cache = {}


def _S():
    from polyfuzz_amd import _lib
    return _lib.PAIR_SLICE


def _fitted(ctx, key, fl, tl):
    """(TFIDF model, from-side DeviceCSR, DeviceIndex, raw from-list on the device, raw to-list or None), fitted once per case"""
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import TFIDF
    if key not in _cache:
        m = TFIDF(n_gram_range=(3, 3), clean_string=True)
        from_dev, _ = m._extract_tf_idf(list(fl), None if tl is None else list(tl), True)
        f = _lib.DeviceStrings.upload(ctx, list(fl))
        t = None if tl is None else _lib.DeviceStrings.upload(ctx, list(tl))
        _cache[key] = (m, from_dev, m._dev_index, f, t)
    return _cache[key]


def _k15(ctx, key, fl, tl, b):
    """K15's pairs by the existing entry, downloaded: (row_ptr, idx, sim) -- and the same pairs as a handle"""
    from polyfuzz_amd import _lib
    if (key, b) not in _cache:
        _, from_dev, index, _, _ = _fitted(ctx, key, fl, tl)
        row_ptr, idx, sim, _ = _lib.sparse_join(ctx, index, from_dev, b, self_join=tl is None)
        _cache[key, b] = (row_ptr, idx, sim, _lib.sparse_join_dev(ctx, index, from_dev, b, self_join=tl is None))
    return _cache[key, b]


def _assert_csr(got, want, what):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.float64, what
    for g, w in zip(got[:3], want[:3]):
        np.testing.assert_array_equal(g, w, err_msg=str(what))


def _attained(sim, row_ptr, idx):
    rows = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    s = np.unique(sim[rows, idx])
    s = s[(s > 0.0) & (s < 1.0)]
    return float(s[len(s) // 2])


# ---- 1. the handle equals K15 ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["two_lists", "self"])
def test_handle_equals_k15(ctx, case):
    from polyfuzz_amd import _lib
    fl, tl = C.company_two_lists() if case == "two_lists" else (C.company_self(), None)
    _, from_dev, index, _, _ = _fitted(ctx, ("company", case), fl, tl)
    for b in (0.9, 0.6):
        row_ptr, idx, sim, counts = _lib.sparse_join(ctx, index, from_dev, b, self_join=tl is None, counters=True)
        total = len(idx)
        assert total > 1
        for hint in (1, total - 1, total, total + 7, None):          # the repeat path, and the single pass
            pairs, work = _lib.sparse_join_dev(ctx, index, from_dev, b, self_join=tl is None, capacity_hint=hint, counters=True)
            assert (pairs.n, pairs.n_from, pairs.n_to, pairs.self_join) == (total, len(fl), len(tl or fl), tl is None)
            got = pairs.download()
            assert got[2].dtype == np.float32
            np.testing.assert_array_equal(got[0], row_ptr)
            np.testing.assert_array_equal(got[1], idx)
            np.testing.assert_array_equal(got[2].view(np.uint32), sim.view(np.uint32))
            assert work == {k: counts[k] for k in _lib.SPARSE_JOIN_COUNTERS}
            pairs.free()
    # a b no pair reaches
    fl, tl = C.company_two_lists_distinct() if case == "two_lists" else (C.company_self_distinct(), None)
    _, from_dev, index, _, _ = _fitted(ctx, ("distinct", case), fl, tl)
    assert len(_lib.sparse_join(ctx, index, from_dev, 1.0, self_join=tl is None)[1]) == 0
    pairs = _lib.sparse_join_dev(ctx, index, from_dev, 1.0, self_join=tl is None)
    row_ptr, idx, sim = pairs.download()
    assert pairs.n == 0 and not row_ptr.any() and len(row_ptr) == len(fl) + 1 and len(idx) == len(sim) == 0


# ---- 2. the keys join equals the definition; 3. and K16 on the same pairs -----------------------------------------------------------

def _small(case):
    if case == "two_lists":
        return C.small_two_lists()
    strings, sims = C.small_self()
    return strings, None, sims


@pytest.mark.parametrize("name", P.FOUR)
@pytest.mark.parametrize("case", ["two_lists", "self"])
def test_keys_join_equals_the_definition(ctx, case, name):
    from polyfuzz_amd import _lib
    fl, tl, sims = _small(case)
    _, _, _, f, t = _fitted(ctx, ("small", case), fl, tl)
    row_ptr, idx, _, pairs = _k15(ctx, ("small", case), fl, tl, C.B)
    assert pairs.n == len(idx) >= 50
    for thr in P.THRESHOLDS + (_attained(sims[name], row_ptr, idx),):
        want = C.expected_keys_join(sims[name], row_ptr, idx, thr)
        got = _lib.pairs_join_keys(ctx, f, t, pairs, name, thr, counters=True)
        _assert_csr(got, want, (case, name, thr))
        assert got[3] == {"candidates": len(idx), "scored": len(idx), "pairs": len(want[1]), "items": C.items_of(row_ptr, _S())}
        if tl is None:
            assert (np.repeat(np.arange(len(fl)), np.diff(got[0])) < got[1]).all()
            _assert_csr(_lib.pairs_join_keys(ctx, f, f, pairs, name, thr), want, (case, name, thr, "own handle"))
    assert 0 < len(want[1]) < len(idx)          # the attained score is a threshold, and equal is kept
    _assert_csr(_lib.pairs_join_keys(ctx, f, t, pairs, _lib.PAIR_SCORERS[name], 0.5), C.expected_keys_join(sims[name], row_ptr, idx, 0.5), name)


@pytest.mark.parametrize("name", P.FOUR)
def test_keys_join_equals_k16_on_the_same_pairs(ctx, name):
    from polyfuzz_amd import _lib
    fl, tl, _ = C.small_two_lists()
    _, _, _, f, t = _fitted(ctx, ("small", "two_lists"), fl, tl)
    row_ptr, idx, _, pairs = _k15(ctx, ("small", "two_lists"), fl, tl, C.B)
    assert 0 < np.diff(row_ptr).max() <= 64
    table = P.device_table(ctx, C.padded_table(row_ptr, idx))
    for thr in P.THRESHOLDS:
        got = _lib.pairs_join_keys(ctx, f, t, pairs, name, thr)
        want = _lib.pairs_join(ctx, f, t, table, name, thr)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (name, thr)


# ---- 4. slice and chunk borders ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", P.FOUR)
def test_slice_and_chunk_borders(ctx, name):
    from polyfuzz_amd import _lib
    S = _S()
    fl, tl, sizes, sims = C.borders(S)
    _, _, _, f, t = _fitted(ctx, "borders", fl, tl)
    row_ptr, idx, _, pairs = _k15(ctx, "borders", fl, tl, C.B)
    assert np.diff(row_ptr).tolist() == sizes == C.border_sizes(S) and row_ptr[-1] == pairs.n == sum(sizes)
    assert sizes[-1] > 0                                              # the last row's range ends at the last key
    items = sum(-(-s // S) for s in sizes)
    assert items == C.items_of(row_ptr, S) >= 12                  # (12 when no two of the sizes coincide)
    for thr in P.THRESHOLDS:
        want = C.expected_keys_join(sims[name], row_ptr, idx, thr)
        got = _lib.pairs_join_keys(ctx, f, t, pairs, name, thr, counters=True)
        _assert_csr(got, want, (name, thr))
        assert got[3] == {"candidates": pairs.n, "scored": pairs.n, "pairs": len(want[1]), "items": items}
    assert 0 < len(C.expected_keys_join(sims[name], row_ptr, idx, 0.8)[1]) < pairs.n


# ---- 5. a hub ----------------------------------------------------------------------------------------------------------------------

def _device_scores(ctx, oracle_mod, strings, f):
    """{scorer: float64 [n, n]} from the all-pairs kernels (K9, K8), cross-checked against the oracles on 200 pairs"""
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(len(strings))
    rows, cols = rng.choice(len(strings), 10, replace=False), rng.choice(len(strings), 20, replace=False)
    sub_f, sub_t = [strings[i] for i in rows], [strings[j] for j in cols]
    out = {}
    for name in lev_oracle.SCORERS:
        out[name] = lev_oracle.sim_matrix(strings, strings, _lib.lev_matrix(ctx, f, f, name))
        want = lev_oracle.sim_matrix(sub_f, sub_t, lev_oracle.matrix(sub_f, sub_t, name))
        np.testing.assert_array_equal(out[name][np.ix_(rows, cols)], want, err_msg=name)
    for name in ("jaro", "jaro_winkler"):
        out[name] = _lib.jaro_matrix(ctx, f, f, name)
        np.testing.assert_array_equal(out[name][np.ix_(rows, cols)], oracle_mod.jaro_matrix(sub_f, sub_t, name), err_msg=name)
    return out


@pytest.mark.parametrize("position,length", [("first", 20), ("first", 50), ("first", 80), ("last", 20), ("last", 50), ("last", 80)])
def test_hub(ctx, oracle_mod, position, length):
    """one string with 2 S + 40 partners: three slices, in 32-bit words, in 64-bit words and in the general kernel; with the hub
    last its pairs belong to the other rows"""
    from polyfuzz_amd import _lib
    S = _S()
    strings, h, partners = C.hub(position, length, S)
    key = ("hub", position, length)
    _, _, _, f, _ = _fitted(ctx, key, strings, None)
    row_ptr, idx, _, pairs = _k15(ctx, key, strings, None, C.B)
    assert (np.diff(row_ptr)[0] if h == 0 else (idx == h).sum()) == partners == 2 * S + 40
    sims = _device_scores(ctx, oracle_mod, strings, f)
    for name in P.FOUR:
        for thr in P.THRESHOLDS:
            want = C.expected_keys_join(sims[name], row_ptr, idx, thr)
            got = _lib.pairs_join_keys(ctx, f, None, pairs, name, thr, counters=True)
            _assert_csr(got, want, (position, length, name, thr))
            assert got[3] == {"candidates": pairs.n, "scored": pairs.n, "pairs": len(want[1]), "items": C.items_of(row_ptr, S)}


@pytest.mark.parametrize("name", ["jaro", "jaro_winkler"])
def test_hub_hands_its_last_slice_to_the_general_kernel(ctx, oracle_mod, name):
    """a partner of more than 256 characters in the hub's LAST slice only: that item is the general kernel's, the hub's other
    slices stay in registers, and every pair is scored once"""
    from polyfuzz_amd import _lib
    S = _S()
    strings, h, partners = C.hub("first", 20, S, True)
    n = len(strings)
    assert h == 0 and len(strings[-1]) >= 300 and max(map(len, strings[:-1])) <= 256
    _, _, _, f, _ = _fitted(ctx, "hub_long", strings, None)
    row_ptr, idx, _, pairs = _k15(ctx, "hub_long", strings, None, C.B)
    mine = idx[row_ptr[0]:row_ptr[1]]
    assert len(mine) == partners == 2 * S + 40 and mine[-1] == n - 1 and (mine[:2 * S] < n - 1).all()      # in the third slice alone
    sims = _device_scores(ctx, oracle_mod, strings, f)
    ctx.prof_enable(True)
    try:
        for thr in P.THRESHOLDS:
            ctx.prof_reset()
            got = _lib.pairs_join_keys(ctx, f, None, pairs, name, thr, capacity=pairs.n, counters=True)      # (room: one call)
            ctx.sync()
            assert ctx.prof_get("k16_pairs_join_general")[1] == 1 and ctx.prof_get("k16_pairs_join")[1] == 1
            want = C.expected_keys_join(sims[name], row_ptr, idx, thr)
            _assert_csr(got, want, (name, thr))
            assert got[3]["scored"] == got[3]["candidates"] == pairs.n and got[3]["pairs"] == len(want[1])
    finally:
        ctx.prof_enable(False)
    label, n_pairs, _, counts = _lib.pairs_components_keys(ctx, f, pairs, name, 0.8, counters=True)
    want = C.expected_keys_join(sims[name], row_ptr, idx, 0.8)
    np.testing.assert_array_equal(label, P.expected_labels(n, want[0], want[1]))
    assert n_pairs == len(want[1]) and counts["scored"] == pairs.n


# ---- 6. capacity -------------------------------------------------------------------------------------------------------------------

def _raw_join_keys(ctx, f, t, pairs, scorer, thr, cap, n_from, counters=True):
    """pfz_pairs_join_keys itself, with 8 guard words behind every buffer: (rc, total, row_ptr, idx, sim, counters)"""
    from polyfuzz_amd import _lib
    row_ptr = np.full(n_from + 1 + 8, -7, np.int64)
    idx, sim = np.full(max(cap, 0) + 8, -7, np.int32), np.full(max(cap, 0) + 8, -7.0, np.float64)
    total, work = ctypes.c_int64(-7), np.full(4 + 8, -7, np.int64)
    rc = ctx.lib.pfz_pairs_join_keys(ctx.h, f.h, None if t is None else t.h, pairs.h, scorer, ctypes.c_double(thr), cap,
                                     _lib._ptr(row_ptr), _lib._ptr(idx), _lib._ptr(sim), ctypes.byref(total),
                                     _lib._ptr(work) if counters else None)
    return rc, total.value, row_ptr, idx, sim, work


@pytest.mark.parametrize("case", ["two_lists", "self"])
def test_capacity(ctx, case):
    from polyfuzz_amd import _lib
    fl, tl, sims = _small(case)
    _, _, _, f, t = _fitted(ctx, ("small", case), fl, tl)
    row_ptr, idx, _, pairs = _k15(ctx, ("small", case), fl, tl, C.B)
    want = C.expected_keys_join(sims["levenshtein"], row_ptr, idx, 0.5)
    total, n = len(want[1]), len(fl)
    assert total > 1
    rc, got, r_ptr, r_idx, r_sim, work = _raw_join_keys(ctx, f, t, pairs, 1, 0.5, total - 1, n)
    assert rc == 0 and got == total                                            # PFZ_OK, the exact total ...
    assert (r_ptr == -7).all() and (r_idx == -7).all() and (r_sim == -7.0).all()      # ... and nothing written
    assert work[:4].tolist() == [pairs.n, pairs.n, total, C.items_of(row_ptr, _S())] and (work[4:] == -7).all()
    rc, got, r_ptr, r_idx, r_sim, _ = _raw_join_keys(ctx, f, t, pairs, 1, 0.5, total, n)
    assert rc == 0 and got == total
    np.testing.assert_array_equal(r_ptr[:n + 1], want[0])
    np.testing.assert_array_equal(r_idx[:total], want[1])
    np.testing.assert_array_equal(r_sim[:total], want[2])
    assert (r_ptr[n + 1:] == -7).all() and (r_idx[total:] == -7).all() and (r_sim[total:] == -7.0).all()
    # the binding's one repeat gives the same
    _assert_csr(_lib.pairs_join_keys(ctx, f, t, pairs, "levenshtein", 0.5, capacity=1), want, case)
    rc, got, r_ptr, _, _, _ = _raw_join_keys(ctx, f, t, pairs, 1, 0.5, 0, n, counters=False)
    assert rc == 0 and got == total and (r_ptr == -7).all()


# ---- 7. components -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", P.FOUR)
def test_components(ctx, name):
    from polyfuzz_amd import _lib
    strings, sims = C.small_self()
    n = len(strings)
    _, _, _, f, _ = _fitted(ctx, ("small", "self"), strings, None)
    row_ptr, idx, _, pairs = _k15(ctx, ("small", "self"), strings, None, C.B)
    for thr in P.THRESHOLDS:
        want = C.expected_keys_join(sims[name], row_ptr, idx, thr)
        labels = P.expected_labels(n, want[0], want[1])
        label, n_pairs, components, counts = _lib.pairs_components_keys(ctx, f, pairs, name, thr, counters=True)
        assert label.dtype == np.int32
        np.testing.assert_array_equal(label, labels, err_msg=str((name, thr)))
        assert n_pairs == len(want[1]) and components == len(set(labels.tolist()))
        assert counts == {"candidates": pairs.n, "scored": pairs.n, "pairs": n_pairs, "items": C.items_of(row_ptr, _S())}
    assert 1 < components < n
    fl, tl, _ = C.small_two_lists()
    _, _, _, f2, _ = _fitted(ctx, ("small", "two_lists"), fl, tl)
    two = _k15(ctx, ("small", "two_lists"), fl, tl, C.B)[3]
    with pytest.raises(_lib.PfzError, match="two-list"):
        _lib.pairs_components_keys(ctx, f2, two, name, 0.5)


# ---- 8. the matcher ------------------------------------------------------------------------------------------------------------------

def _frames_equal(got, want):
    assert list(got.columns) == ["From", "To", "Similarity"] and len(got) == len(want)
    assert got["From"].tolist() == want["From"].tolist() and got["To"].tolist() == want["To"].tolist()
    np.testing.assert_array_equal(got["Similarity"].to_numpy(), want["Similarity"].to_numpy())


@pytest.mark.parametrize("name", P.FOUR)
def test_matcher(ctx, name):
    from polyfuzz_amd import linkage
    from polyfuzz_amd.models import BlockedEditDistance
    fl, tl, sims = C.small_two_lists()
    fl, tl = list(fl), list(tl)
    row_ptr, idx, _, pairs = _k15(ctx, ("small", "two_lists"), tuple(fl), tuple(tl), C.B)
    m = BlockedEditDistance(name, blocking_similarity=C.B, candidates=2, top_n=2, min_similarity=0.99)      # (none of which plays a part)
    for thr in (0.5, 0.8):
        want = C.expected_keys_join(sims[name], row_ptr, idx, thr)
        frame = m.join(fl, tl, thr)
        _frames_equal(frame, P.frame_of(fl, tl, *want))
        assert m.last_counts == {"candidates": pairs.n, "scored": pairs.n, "pairs": len(want[1]), "items": C.items_of(row_ptr, _S())}
        assert set(m.last_timings) == {"tfidf", "k16", "frame"}
        _frames_equal(m.join(fl, list(tl), thr, re_train=False), frame)          # an equal to-list: the resident one is reused
    empty = m.join([], tl, 0.5)
    assert list(empty.columns) == ["From", "To", "Similarity"] and len(empty) == 0 and m.last_counts["pairs"] == 0
    # the self-join, the components and the linkage
    strings, sims = C.small_self()
    strings = list(strings)
    row_ptr, idx, _, pairs = _k15(ctx, ("small", "self"), tuple(strings), None, C.B)
    for thr in (0.5, 0.8):
        want = C.expected_keys_join(sims[name], row_ptr, idx, thr)
        _frames_equal(m.join(strings, None, thr), P.frame_of(strings, strings, *want))
        labels = P.expected_labels(len(strings), want[0], want[1])
        np.testing.assert_array_equal(m.components(strings, thr), labels)
        assert m.last_counts == {"candidates": pairs.n, "scored": pairs.n, "pairs": len(want[1]), "items": C.items_of(row_ptr, _S()),
                                 "components": len(set(labels.tolist()))}
        clusters, id_map, _ = linkage.connected_components(strings, m, thr)
        assert clusters == linkage.dicts_from_labels(strings, labels)[0]
    # match ranks, and needs the table: the keyword changes nothing there
    plain = BlockedEditDistance(name, candidates=8, top_n=2)
    keyed = BlockedEditDistance(name, candidates=8, top_n=2, blocking_similarity=0.3)
    a, b = plain.match(fl, tl), keyed.match(fl, tl)
    assert list(a.columns) == list(b.columns)
    for col in a.columns:
        if col.startswith("Similarity"):
            np.testing.assert_array_equal(a[col].to_numpy(), b[col].to_numpy())
        else:
            assert a[col].tolist() == b[col].tolist()


# ---- 9. what the feature is for ------------------------------------------------------------------------------------------------------

def test_forty_copies_are_780_pairs(ctx):
    """derivable: 40 copies of one name are 40 * 39 / 2 pairs at similarity 1.0, and a table of 8 neighbours per row cannot hold
    more than 40 * 8 = 320 cells between them"""
    from polyfuzz_amd.models import BlockedEditDistance, EditDistance
    names, at = C.copies()
    names = list(names)
    exact = EditDistance(scorer="levenshtein").join(names, min_similarity=1.0)
    assert len(exact) == 780
    got = BlockedEditDistance("levenshtein", blocking_similarity=0.9).join(names, None, 1.0)
    _frames_equal(got, exact)
    assert set(got["From"]) == set(got["To"]) == {names[at[0]]}
    table = BlockedEditDistance("levenshtein", candidates=8).join(names, None, 1.0)
    assert len(table) <= 320 < 780
    labels = BlockedEditDistance("levenshtein", blocking_similarity=0.9).components(names, 1.0)
    assert (labels[at] == at[0]).all() and len(set(labels.tolist())) == 61


# ---- 10. the raw ABI's refusals --------------------------------------------------------------------------------------------------------

def test_raw_abi_refusals(ctx):
    from polyfuzz_amd import _lib
    fl, tl, _ = C.small_two_lists()
    _, from_dev, index, f, t = _fitted(ctx, ("small", "two_lists"), fl, tl)
    two = _k15(ctx, ("small", "two_lists"), fl, tl, C.B)[3]
    strings, _ = C.small_self()
    _, self_csr, self_index, s, _ = _fitted(ctx, ("small", "self"), strings, None)
    one = _k15(ctx, ("small", "self"), strings, None, C.B)[3]
    n = len(fl)
    row_ptr, idx, sim = np.zeros(n + 400, np.int64), np.zeros(8192, np.int32), np.zeros(8192, np.float64)
    label = np.zeros(len(strings), np.int32)
    total, a, b = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    ptr = _lib._ptr

    def join(f_=f, t_=t, p=two, scorer=1, thr=0.5, cap=8192, rp=row_ptr, ix=idx, sm=sim, tot=total):
        return ctx.lib.pfz_pairs_join_keys(ctx.h, f_.h if f_ is not None else None, t_.h if t_ is not None else None, p.h if p is not None else None, scorer,
                                           ctypes.c_double(thr), cap, ptr(rp), ptr(ix), ptr(sm), ctypes.byref(tot) if tot is not None else None, None)

    def comp(s_=s, p=one, scorer=1, thr=0.5, lab=label, pa=a, co=b):
        return ctx.lib.pfz_pairs_components_keys(ctx.h, s_.h if s_ is not None else None, p.h if p is not None else None, scorer, ctypes.c_double(thr), ptr(lab),
                                                 ctypes.byref(pa) if pa is not None else None, ctypes.byref(co) if co is not None else None, None)
    assert join() == 0 and comp() == 0
    INVALID = -1
    for call in (join, comp):
        assert call(scorer=0) == INVALID
        assert b"0 .. 100" in ctx.lib.pfz_last_error()                         # K16's message
        for bad in (5, -1):
            assert call(scorer=bad) == INVALID
        for bad in (float("nan"), -0.1, 1.5, float("inf")):
            assert call(thr=bad) == INVALID
        assert call(p=None) == INVALID
    assert join(cap=-1) == INVALID
    assert join(f_=s) == INVALID and join(t_=s) == INVALID                    # list sizes differ from the handle's
    assert comp(s_=f) == INVALID
    assert join(f_=s, t_=f, p=one) == INVALID                                  # a self handle with another to-list
    other = _lib.DeviceStrings.upload(ctx, list(strings))
    assert join(f_=s, t_=other, p=one) == INVALID                              # ... also one of the same size
    assert join(f_=s, t_=None, p=one) == 0 and join(f_=s, t_=s, p=one) == 0
    assert join(t_=None) == INVALID                                            # a two-list handle without a to-list
    assert comp(s_=f, p=two) == INVALID                                        # the components of a two-list handle
    assert join(rp=None) == INVALID and join(tot=None) == INVALID and join(ix=None) == INVALID and join(sm=None) == INVALID
    assert join(f_=None) == INVALID and comp(s_=None) == INVALID
    assert comp(lab=None) == INVALID and comp(pa=None) == INVALID and comp(co=None) == INVALID
    # pfz_cossim_join_dev and the accessors
    h = ctypes.c_void_p()
    dev = lambda ix=index, m=from_dev, self_join=0, thr=0.5, hint=0, out=h: ctx.lib.pfz_cossim_join_dev(
        ctx.h, ix.h if ix is not None else None, m.h if m is not None else None, self_join, ctypes.c_double(thr), hint, ctypes.byref(out) if out is not None else None, None)
    assert dev(ix=None) == INVALID and dev(m=None) == INVALID and dev(out=None) == INVALID and dev(hint=-1) == INVALID
    for bad in (float("nan"), -0.1, 1.5):
        assert dev(thr=bad) == INVALID
    assert dev(self_join=1) == INVALID                                         # not the matrix the index was built from
    assert dev(ix=self_index) == INVALID                                       # another vocabulary
    assert h.value is None
    n_out = ctypes.c_int64(0)
    assert ctx.lib.pfz_pairs_count(None, ctypes.byref(n_out)) == INVALID and ctx.lib.pfz_pairs_count(two.h, None) == INVALID
    assert ctx.lib.pfz_pairs_download(ctx.h, two.h, None, ptr(idx), None) == INVALID
    assert ctx.lib.pfz_pairs_download(ctx.h, two.h, ptr(row_ptr), None, None) == INVALID
    ctx.lib.pfz_pairs_free(None)
