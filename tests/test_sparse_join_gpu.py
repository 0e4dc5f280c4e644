"""K15 on the GPU: pfz_cossim_join (TFIDF.join) against the existing path -- pfz_cossim_topn on the same index with lower_bound 0,
thresholded on the host, pairs and float32 score BITS equal -- and against the float64 oracle of oracle/tfidf_numpy.py; the
thresholds 0 and 1, the capacity contract, one list as two handles, the counters and the facade."""
import ctypes

import numpy as np
import pytest

from tests import sparse_join_cases as C

pytestmark = pytest.mark.gpu
ALL_CASES = list(C.SELF_CASES) + [C.TWO_LIST_CASE]


def _assert_same_pairs(got, want, what):
    (rows, cols, sim), (e_rows, e_cols, e_val) = got, want
    assert len(rows) == len(e_rows), (what, len(rows), len(e_rows))
    np.testing.assert_array_equal(rows, e_rows, err_msg=what)
    np.testing.assert_array_equal(cols, e_cols, err_msg=what)
    np.testing.assert_array_equal(sim.view(np.uint32), e_val.view(np.uint32), err_msg=what)


@pytest.mark.parametrize("t", C.THRESHOLDS)
@pytest.mark.parametrize("name", ALL_CASES)
def test_pairs_and_score_bits_equal_the_existing_path(ctx, name, t):
    _, from_dev, _, self_join = C.fitted(ctx, name)
    rows, cols, sim, row_ptr, counts = C.join(ctx, name, t)
    assert sim.dtype == np.float32 and row_ptr[0] == 0 and row_ptr[-1] == len(cols) and len(row_ptr) == from_dev.n_rows + 1
    assert counts["pairs"] == len(rows) > 0
    _assert_same_pairs((rows, cols, sim), C.existing_path(ctx, name, t), f"{name} t={t}")
    assert (np.diff(row_ptr) >= 0).all()
    same_row = rows[1:] == rows[:-1]
    assert (cols[1:][same_row] > cols[:-1][same_row]).all()      # ascending within a row
    if self_join:
        assert (cols > rows).all()


def test_the_spliced_case_runs_the_paths_it_is_there_for(ctx):
    """150 contiguous copies: rows with more than 64 hits in one sweep step; documents: rows beyond 64 n-grams that find their copy"""
    strings, _ = C.lists("spliced")
    n = len(strings)
    rows, cols, sim, row_ptr, _ = C.join(ctx, "spliced", 0.9)
    per_row = np.diff(row_ptr)
    assert per_row[2900] >= 149 and (cols[row_ptr[2900]:row_ptr[2901]][-149:] == np.arange(2901, 3050)).all()
    indptr = C.fitted(ctx, "spliced")[1].download()[0]
    for i in range(300):                                          # an equal string in another block is a pair (unless it has no n-gram)
        assert indptr[i + 1] == indptr[i] or 2600 + i in cols[row_ptr[i]:row_ptr[i + 1]], i
    cols8, ptr8 = C.join(ctx, "spliced", 0.8)[1], C.join(ctx, "spliced", 0.8)[3]
    for d in range(n - 10, n, 2):                                 # document d and its edited copy d + 1 (2 % of 300 characters: about 0.94)
        assert indptr[d + 1] - indptr[d] > 64
        assert cols8[ptr8[d]:ptr8[d + 1]].tolist() == [d + 1]


@pytest.mark.parametrize("t", C.THRESHOLDS)
@pytest.mark.parametrize("name", list(C.ORACLE_HITS))
def test_against_the_float64_oracle(ctx, oracle_mod, name, t):
    """every pair with cosine >= t + 1e-5 is present, none with cosine < t - 1e-5, every score within 1e-5 -- on inputs whose
    band (pairs within 1e-5 of t) is at most 0.5 % of the oracle's hits, which is asserted on the oracle alone first"""
    hits, band = C.oracle_counts(name, t)
    assert (hits, band) == C.ORACLE_HITS[name][t]
    assert band <= 0.005 * hits
    cos = C.oracle_pairs(name)
    rows, cols, sim, _, counts = C.join(ctx, name, t)
    exact = np.asarray(cos[rows, cols]).ravel()                   # (0 where the oracle's cosine is below its floor of 0.5)
    print(f"{name} t={t}: device {len(rows)} hits, oracle {hits} (band {band}), max |score - cosine| "
          f"{np.abs(sim - exact).max(initial=0.0):.3g}")
    found = set(zip(rows.tolist(), cols.tolist()))
    o = cos.tocoo()
    must = o.data >= t + C.BAND
    assert all(p in found for p in zip(o.row[must].tolist(), o.col[must].tolist()))
    assert not (exact < t - C.BAND).any()
    assert np.abs(sim.astype(np.float64) - exact).max(initial=0.0) <= C.BAND
    assert counts["pairs"] == len(rows) and abs(len(rows) - hits) <= band


def test_threshold_zero_is_every_pair_that_shares_an_n_gram(ctx):
    rows, cols, sim, _, _ = C.join(ctx, "names300", 0.0)
    idx, val = C.existing_table(ctx, "names300", 300)
    assert idx.shape == (300, 300)
    _assert_same_pairs((rows, cols, sim), C.threshold_table(idx, val, 0.0, True), "t=0")
    assert len(rows) > 300 and (sim > 0).all()                    # "no match" is never a pair, also at 0


def test_threshold_one_equals_the_existing_path(ctx):
    """whatever that says about equal strings: a copy is a hit only where its truncated sum still rounds to 1.0"""
    rows, cols, sim, _, _ = C.join(ctx, "spliced", 1.0)
    _assert_same_pairs((rows, cols, sim), C.existing_path(ctx, "spliced", 1.0), "t=1")
    assert (sim >= 1.0).all()                                     # (float32 weights: a row's norm may round just above 1)


def _raw_join(ctx, index, from_dev, self_join, t, cap, n):
    """pfz_cossim_join itself, into buffers pre-filled with -7 and one guard word longer than they need be"""
    row_ptr, idx, sim = np.full(n + 2, -7, np.int64), np.full(cap + 1, -7, np.int32), np.full(cap + 1, -7.0, np.float32)
    total, work = ctypes.c_int64(-7), np.full(3, -7, np.int64)
    rc = ctx.lib.pfz_cossim_join(ctx.h, index.h, from_dev.h, int(self_join), float(t), cap, row_ptr.ctypes.data, idx.ctypes.data,
                                 sim.ctypes.data, ctypes.byref(total), work.ctypes.data)
    return rc, total.value, row_ptr, idx, sim, work


@pytest.mark.parametrize("name", ["names2600", C.TWO_LIST_CASE])
def test_capacity_contract_and_determinism(ctx, name):
    from polyfuzz_amd import _lib
    _, f, index, self_join = C.fitted(ctx, name)
    rows, cols, sim, row_ptr, counts = C.join(ctx, name, 0.8)
    total, n = len(rows), f.n_rows
    assert total > 1
    rc, got, r_ptr, r_idx, r_sim, work = _raw_join(ctx, index, f, self_join, 0.8, total - 1, n)
    assert rc == 0 and got == total                                   # PFZ_OK, the exact total ...
    assert (r_ptr == -7).all() and (r_idx == -7).all() and (r_sim == -7.0).all()      # ... and nothing written
    assert work.tolist() == [counts[k] for k in _lib.SPARSE_JOIN_COUNTERS]
    rc, got, r_ptr, r_idx, r_sim, _ = _raw_join(ctx, index, f, self_join, 0.8, total, n)
    assert rc == 0 and got == total
    np.testing.assert_array_equal(r_ptr[:n + 1], row_ptr)
    np.testing.assert_array_equal(r_idx[:total], cols)
    np.testing.assert_array_equal(r_sim[:total].view(np.uint32), sim.view(np.uint32))
    assert r_ptr[n + 1] == -7 and r_idx[total] == -7 and r_sim[total] == -7.0       # not a word behind them
    again = _raw_join(ctx, index, f, self_join, 0.8, total, n)
    for a, b in zip(again[2:5], (r_ptr, r_idx, r_sim)):
        assert a.tobytes() == b.tobytes()                             # the same call gives the same bytes
    for cap in (0, 1, total - 1):                                     # the binding's one repeat returns the full result
        b_ptr, b_idx, b_sim, b_counts = _lib.sparse_join(ctx, index, f, 0.8, self_join=self_join, capacity=cap)
        assert b_counts == {"pairs": total}
        assert b_ptr.tobytes() == row_ptr.tobytes() and b_idx.tobytes() == cols.astype(np.int32).tobytes() and b_sim.tobytes() == sim.tobytes()


def test_one_list_as_two_handles_has_both_halves(ctx):
    """the two-list form on one list (a second handle of the same rows) reports (i, j), (j, i) and (i, i); its upper triangle is
    the self-join, bit for bit; the self-join refuses a matrix the index was not built from"""
    from polyfuzz_amd import _lib
    m, f, index, _ = C.fitted(ctx, "names2600")
    other = m._dev_vec.transform(m._upload(list(C.lists("names2600")[0])))
    row_ptr, idx, sim, counts = _lib.sparse_join(ctx, index, other, 0.8, counters=True)
    rows, cols = C.csr_pairs(row_ptr, idx)
    s_rows, s_cols, s_sim, _, s_counts = C.join(ctx, "names2600", 0.8)
    on_diag = int((rows == cols).sum())
    assert on_diag >= 2590                                            # every row with an n-gram meets itself
    up = cols > rows
    _assert_same_pairs((rows[up], cols[up], sim[up]), (s_rows, s_cols, s_sim), "upper triangle")
    low = cols < rows
    order = np.lexsort((rows[low], cols[low]))                        # the lower triangle, transposed: the same pairs and bits
    _assert_same_pairs((cols[low][order], rows[low][order], sim[low][order]), (s_rows, s_cols, s_sim), "lower triangle")
    assert counts["pairs"] == 2 * len(s_rows) + on_diag
    assert s_counts["visits"] < counts["visits"]                      # the self-join walks the blocks from its own on
    with pytest.raises(_lib.PfzError, match="self-join"):
        _lib.sparse_join(ctx, index, other, 0.8, self_join=True)
    with pytest.raises(_lib.PfzError, match="pfz_cossim_components"):
        _lib.sparse_components(ctx, index, other, 0.8)


@pytest.mark.parametrize("name", ALL_CASES)
def test_counters(ctx, name):
    _, f, index, self_join = C.fitted(ctx, name)
    info = index.info()
    block, n_blocks = info["block_cols"], info["n_blocks"]
    most = sum(n_blocks - i // block for i in range(f.n_rows)) if self_join else f.n_rows * n_blocks
    for t in C.THRESHOLDS:
        counts = C.join(ctx, name, t)[4]
        assert 0 <= counts["skipped"] <= counts["visits"] <= most, (name, t, counts)
        assert counts["hit_steps"] >= 1 and counts["hit_steps"] <= counts["pairs"], (name, t, counts)
    assert C.join(ctx, name, 0.9)[4]["skipped"] >= C.join(ctx, name, 0.6)[4]["skipped"]
    assert C.join(ctx, name, 0.9)[4]["visits"] == C.join(ctx, name, 0.6)[4]["visits"]       # what has postings does not depend on t
    if name == "names2600":
        assert C.join(ctx, name, 0.9)[4]["skipped"] > 0


def test_invalid_arguments_and_empty_sides(ctx):
    from polyfuzz_amd import _lib
    m, f, index, _ = C.fitted(ctx, "names300")
    n = f.n_rows
    for t in (float("nan"), 1.5, -0.25, float("inf"), np.nextafter(1.0, 2.0)):
        assert _raw_join(ctx, index, f, 1, t, 4, n)[0] == -1, t
    total = ctypes.c_int64(0)
    assert ctx.lib.pfz_cossim_join(ctx.h, index.h, f.h, 1, 0.5, -1, np.zeros(n + 1, np.int64).ctypes.data, None, None,
                                   ctypes.byref(total), None) == -1
    pairs, comps = ctypes.c_int64(0), ctypes.c_int64(0)
    label = np.zeros(n, np.int32)
    for t in (float("nan"), 1.5, -0.25):
        assert ctx.lib.pfz_cossim_components(ctx.h, index.h, f.h, t, label.ctypes.data, ctypes.byref(pairs), ctypes.byref(comps), None) == -1
    assert ctx.lib.pfz_cossim_components(ctx.h, index.h, f.h, 0.5, label.ctypes.data, None, ctypes.byref(comps), None) == -1
    assert ctx.lib.pfz_cossim_components(ctx.h, index.h, f.h, 0.5, label.ctypes.data, ctypes.byref(pairs), None, None) == -1
    narrow = _lib.DeviceCSR.upload(ctx, np.array([0, 1]), np.array([0]), np.array([1.0]), 7)
    with pytest.raises(_lib.PfzError, match="columns"):
        _lib.sparse_join(ctx, index, narrow, 0.5)


def test_an_empty_side_is_no_pairs(ctx):
    from polyfuzz_amd import _lib
    _, f, index, _ = C.fitted(ctx, "names300")
    n, n_cols = f.n_rows, index.info()["n_cols"]
    empty = _lib.DeviceCSR.upload(ctx, np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), n_cols)
    row_ptr, idx, sim, counts = _lib.sparse_join(ctx, index, empty, 0.5, counters=True)       # no from-rows
    assert row_ptr.tolist() == [0] and len(idx) == 0 and len(sim) == 0 and counts == {"pairs": 0, "visits": 0, "skipped": 0, "hit_steps": 0}
    empty_index = _lib.DeviceIndex.build(ctx, empty)
    row_ptr, idx, sim, counts = _lib.sparse_join(ctx, empty_index, f, 0.5)                    # no to-rows
    assert row_ptr.tolist() == [0] * (n + 1) and counts == {"pairs": 0}
    label, pairs, components = _lib.sparse_components(ctx, empty_index, empty, 0.5)
    assert len(label) == 0 and (pairs, components) == (0, 0)


def test_the_call_is_split_into_its_profiling_scopes(ctx):
    from polyfuzz_amd import _lib
    _, f, index, _ = C.fitted(ctx, "names2600")
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        _lib.sparse_join(ctx, index, f, 0.8, self_join=True, capacity=1 << 16)
        _lib.sparse_components(ctx, index, f, 0.8)
        ctx.sync()
        assert [ctx.prof_get(k)[1] for k in ("k15_join", "k15_sort_unpack", "k15_components")] == [1, 1, 1]
    finally:
        ctx.prof_enable(False)


def test_tfidf_join_frame(ctx):
    from polyfuzz_amd import linkage
    from polyfuzz_amd.models import TFIDF
    from_list, to_list = [list(x) for x in C.lists(C.TWO_LIST_CASE)]
    m = TFIDF(min_similarity=0.99, top_n=3, cosine_method="knn")        # (none of the three plays a part)
    frame = m.join(from_list, to_list, 0.8)
    rows, cols, sim = C.join(ctx, C.TWO_LIST_CASE, 0.8)[:3]
    assert list(frame.columns) == ["From", "To", "Similarity"] and len(frame) == len(rows)
    assert [str(d) for d in frame.dtypes] == ["object", "object", "float64"]
    assert frame["From"].tolist() == [from_list[i] for i in rows] and frame["To"].tolist() == [to_list[j] for j in cols]
    assert frame["Similarity"].to_numpy().tobytes() == sim.astype(np.float64).tobytes()       # unrounded
    assert m.last_counts == {"pairs": len(rows)} and set(m.last_timings) == {"device", "frame"}
    # re_train=False reuses the fitted to-side: a slice of the from-list gives the slice of the frame
    part = m.join(from_list[700:], to_list, 0.8, re_train=False)
    want = frame[np.asarray(rows) >= 700].reset_index(drop=True)
    assert len(part) > 0 and part.equals(want)
    # the self-join: From is the lower position of every pair; the scores are match's
    names = list(C.lists("names300")[0])
    own = TFIDF()
    self_frame = own.join(names, min_similarity=0.6)
    s_rows, s_cols, s_sim = C.join(ctx, "names300", 0.6)[:3]
    assert self_frame["From"].tolist() == [names[i] for i in s_rows] and self_frame["To"].tolist() == [names[j] for j in s_cols]
    assert self_frame["Similarity"].to_numpy().tobytes() == s_sim.astype(np.float64).tobytes()
    clusters, mapping, _ = linkage.single_linkage(self_frame, 0.6)      # the frame has the columns single_linkage reads
    assert clusters and set(mapping) <= set(names)


def test_tfidf_join_of_one_element_and_empty_lists(ctx):
    """a one-element list has no pair; an empty from-list has no row; an empty list alone cannot be fitted, as in match()"""
    from polyfuzz_amd.models import TFIDF
    to_list = list(C.lists(C.TWO_LIST_CASE)[1])
    one = TFIDF().join(["apple inc"], min_similarity=0.5)
    assert list(one.columns) == ["From", "To", "Similarity"] and len(one) == 0
    assert TFIDF().components(["apple inc"], 0.5).tolist() == [0]
    none = TFIDF().join([], to_list[:50], 0.5)
    assert list(none.columns) == ["From", "To", "Similarity"] and len(none) == 0
    hit = TFIDF().join([to_list[7]], to_list[:50], 0.99)
    assert to_list[7] in hit["To"].tolist() and set(hit["From"]) == {to_list[7]}
    with pytest.raises(ValueError, match="empty vocabulary"):
        TFIDF().join([], min_similarity=0.5)
