"""K14 on the GPU: pfz_dense_join (Embeddings.join) against the existing path -- pfz_dense_topn with ntop = every column and the
threshold as its lower bound, pairs and float32 score BITS equal -- and against the float64 cosines of oracle/dense.py; the
capacity contract, the counters that hold "the lower triangle is not computed", the edge inputs and the facade."""
import ctypes

import numpy as np
import pytest

from tests import dense_join_cases as C

pytestmark = pytest.mark.gpu
ALL_CASES = list(C.SELF_CASES) + [C.TWO_LIST_CASE]
_devs, _join, _existing_path = C.devs, C.join, C.existing_path


def _assert_same_pairs(got, want, what):
    (rows, cols, sim), (e_rows, e_cols, e_val) = got, want
    assert len(rows) == len(e_rows), (what, len(rows), len(e_rows))
    np.testing.assert_array_equal(rows, e_rows, err_msg=what)
    np.testing.assert_array_equal(cols, e_cols, err_msg=what)
    np.testing.assert_array_equal(sim.view(np.uint32), e_val.view(np.uint32), err_msg=what)


@pytest.mark.parametrize("panel_rows", [None, "128"])
@pytest.mark.parametrize("t", C.THRESHOLDS)
@pytest.mark.parametrize("name", ALL_CASES)
def test_pairs_and_score_bits_equal_the_existing_path(ctx, monkeypatch, name, t, panel_rows):
    if panel_rows:
        monkeypatch.setenv("PFZ_K5_PANEL_ROWS", panel_rows)      # the reference crosses panels
    f, to = _devs(ctx, name)
    rows, cols, sim, row_ptr, _ = _join(ctx, name, t)
    assert sim.dtype == np.float32 and row_ptr[0] == 0 and row_ptr[-1] == len(cols) and len(row_ptr) == f.n + 1
    _assert_same_pairs((rows, cols, sim), _existing_path(ctx, f, to, t), f"{name} t={t}")
    assert (np.diff(row_ptr) >= 0).all()
    same_row = rows[1:] == rows[:-1]
    assert (cols[1:][same_row] > cols[:-1][same_row]).all()      # ascending within a row
    if to is None:
        assert (cols > rows).all()


@pytest.mark.parametrize("t", C.THRESHOLDS)
@pytest.mark.parametrize("name", ALL_CASES)
def test_against_the_float64_oracle(ctx, oracle_mod, name, t):
    """every pair with cosine >= t + 1e-5 is present, none with cosine < t - 1e-5, every score within 1e-5 -- on inputs whose
    band (pairs within 1e-5 of t) is at most 0.5 % of the oracle's hits, which is asserted on the oracle alone first"""
    hits, band = C.oracle_counts(name, t)
    assert (hits, band) == C.ORACLE_HITS[name][t]
    assert band <= 0.005 * hits
    cos = C.cosines(name)
    rows, cols, sim, _, counts = _join(ctx, name, t)
    print(f"{name} t={t}: device {len(rows)} hits, oracle {hits} (band {band}), max |score - cosine| "
          f"{np.abs(sim - cos[rows, cols]).max(initial=0.0):.3g}")
    found = np.zeros(cos.shape, bool)
    found[rows, cols] = True
    assert found[cos >= t + C.BAND].all()
    assert not found[cos < t - C.BAND].any()
    assert np.abs(sim.astype(np.float64) - cos[rows, cols]).max(initial=0.0) <= C.BAND
    assert counts["pairs"] == len(rows) and abs(len(rows) - hits) <= band


def _raw_join(ctx, f, to, t, cap, n):
    """pfz_dense_join itself, into buffers pre-filled with -7 and one guard word longer than they need be"""
    row_ptr, idx, sim = np.full(n + 2, -7, np.int64), np.full(cap + 1, -7, np.int32), np.full(cap + 1, -7.0, np.float32)
    total, work = ctypes.c_int64(-7), np.full(2, -7, np.int64)
    rc = ctx.lib.pfz_dense_join(ctx.h, f.h, None if to is None else to.h, float(t), cap, row_ptr.ctypes.data, idx.ctypes.data,
                                sim.ctypes.data, ctypes.byref(total), work.ctypes.data)
    return rc, total.value, row_ptr, idx, sim, work


@pytest.mark.parametrize("name", ["300x96", C.TWO_LIST_CASE])
def test_capacity_contract_and_determinism(ctx, name):
    from polyfuzz_amd import _lib
    f, to = _devs(ctx, name)
    rows, cols, sim, row_ptr, counts = _join(ctx, name, 0.8)
    total, n = len(rows), f.n
    assert total > 1
    rc, got, r_ptr, r_idx, r_sim, work = _raw_join(ctx, f, to, 0.8, total - 1, n)
    assert rc == 0 and got == total                                   # PFZ_OK, the exact total ...
    assert (r_ptr == -7).all() and (r_idx == -7).all() and (r_sim == -7.0).all()      # ... and nothing written
    assert work.tolist() == [counts["tiles"], counts["hit_corners"]]
    rc, got, r_ptr, r_idx, r_sim, _ = _raw_join(ctx, f, to, 0.8, total, n)
    assert rc == 0 and got == total
    np.testing.assert_array_equal(r_ptr[:n + 1], row_ptr)
    np.testing.assert_array_equal(r_idx[:total], cols)
    np.testing.assert_array_equal(r_sim[:total].view(np.uint32), sim.view(np.uint32))
    assert r_ptr[n + 1] == -7 and r_idx[total] == -7 and r_sim[total] == -7.0       # not a word behind them
    again = _raw_join(ctx, f, to, 0.8, total, n)
    for a, b in zip(again[2:5], (r_ptr, r_idx, r_sim)):
        assert a.tobytes() == b.tobytes()                             # the same call gives the same bytes
    for cap in (0, 1, total - 1):                                     # the binding's one repeat returns the full result
        b_ptr, b_idx, b_sim, b_counts = _lib.dense_join(ctx, f, to, 0.8, capacity=cap)
        assert b_counts == {"pairs": total}
        assert b_ptr.tobytes() == row_ptr.tobytes() and b_idx.tobytes() == cols.astype(np.int32).tobytes() and b_sim.tobytes() == sim.tobytes()


@pytest.mark.parametrize("name", ALL_CASES)
def test_counters_hold_that_the_lower_triangle_is_not_computed(ctx, name):
    f, to = _devs(ctx, name)
    tiles = lambda n: -(-n // 128)
    want = tiles(f.n) * (tiles(f.n) + 1) // 2 if to is None else tiles(f.n) * tiles(to.n)
    for t in C.THRESHOLDS:
        counts = _join(ctx, name, t)[4]
        assert counts["tiles"] == want, (name, t, counts)
        assert 1 <= counts["hit_corners"] <= 4 * want, (name, t, counts)
    assert _join(ctx, name, 0.9)[4]["hit_corners"] <= _join(ctx, name, 0.6)[4]["hit_corners"]


def test_a_list_against_itself_as_two_lists_has_both_halves(ctx):
    """the two-list form on one list (two handles) computes all T^2 tiles and reports (i, j), (j, i) and (i, i); its upper
    triangle is the self-join, bit for bit"""
    from polyfuzz_amd import _lib
    x, _ = C.lists("300x96")
    f, _ = _devs(ctx, "300x96")
    other = _lib.DeviceDense.upload(ctx, x)
    row_ptr, idx, sim, counts = _lib.dense_join(ctx, f, other, 0.8, counters=True)
    rows, cols = C.csr_pairs(row_ptr, idx)
    assert counts["tiles"] == 9 and (rows == cols).sum() == 300
    s_rows, s_cols, s_sim = _join(ctx, "300x96", 0.8)[:3]
    up = cols > rows
    _assert_same_pairs((rows[up], cols[up], sim[up]), (s_rows, s_cols, s_sim), "upper triangle")
    # ([j][i] may differ from [i][j] in the last bit; no cosine of this case is within 1e-5 of 0.8, so the halves agree)
    assert counts["pairs"] == 2 * len(s_rows) + 300
    # the handle passed twice IS the self-join
    p2, i2, v2, c2 = _lib.dense_join(ctx, f, f, 0.8, counters=True)
    assert c2["tiles"] == 6 and i2.tobytes() == s_cols.astype(np.int32).tobytes() and v2.tobytes() == s_sim.tobytes()


def test_identical_rows_a_zero_row_and_tiny_lists(ctx):
    from polyfuzz_amd import _lib
    x = C.gen(257, 40, 20, 8).copy()
    x[200] = x[3]                                  # equal vectors at different positions are a pair ...
    x[100] = 0.0                                   # ... and a row of zeros scores 0 with everything
    f = _lib.DeviceDense.upload(ctx, x)
    for t in (0.6, 0.9, 1.0):
        row_ptr, idx, sim, _ = _lib.dense_join(ctx, f, None, t)
        rows, cols = C.csr_pairs(row_ptr, idx)
        assert (rows != cols).all() and (cols > rows).all()           # never (i, i)
        if t < 1.0:
            at = np.nonzero((rows == 3) & (cols == 200))[0]
            assert len(at) == 1 and abs(float(sim[at[0]]) - 1.0) <= C.BAND
        assert not ((rows == 100) | (cols == 100)).any()
        _assert_same_pairs((rows, cols, sim), _existing_path(ctx, f, None, t), f"edge rows t={t}")
    other = _lib.DeviceDense.upload(ctx, x[:50])
    row_ptr, idx, sim, _ = _lib.dense_join(ctx, f, other, 0.6)          # two lists: a row meets its own copy
    rows, cols = C.csr_pairs(row_ptr, idx)
    assert ((rows == 3) & (cols == 3)).any() and ((rows == 200) & (cols == 3)).any() and not (rows == 100).any()
    one = _lib.DeviceDense.upload(ctx, x[:1])
    row_ptr, idx, sim, counts = _lib.dense_join(ctx, one, None, 0.0, counters=True)
    assert row_ptr.tolist() == [0, 0] and len(idx) == 0 and counts == {"pairs": 0, "tiles": 1, "hit_corners": 0}
    row_ptr, idx, sim, counts = _lib.dense_join(ctx, one, one, 0.5)
    assert len(idx) == 0
    row_ptr, idx, sim, counts = _lib.dense_join(ctx, one, _lib.DeviceDense.upload(ctx, x[:1]), 0.5)
    assert row_ptr.tolist() == [0, 1] and idx.tolist() == [0]
    empty = _lib.DeviceDense.upload(ctx, np.zeros((0, 40), np.float32))
    row_ptr, idx, sim, counts = _lib.dense_join(ctx, empty, None, 0.5, counters=True)
    assert row_ptr.tolist() == [0] and len(idx) == 0 and len(sim) == 0 and counts == {"pairs": 0, "tiles": 0, "hit_corners": 0}
    row_ptr, idx, sim, counts = _lib.dense_join(ctx, f, empty, 0.5)
    assert row_ptr.tolist() == [0] * 258 and counts == {"pairs": 0}
    row_ptr, idx, sim, counts = _lib.dense_join(ctx, empty, f, 0.5)
    assert row_ptr.tolist() == [0] and counts == {"pairs": 0}


def test_a_deal_of_more_than_2_24_workgroups_goes_out_in_several_launches(ctx):
    """A launch takes fewer than 2^32 threads, 2^24 workgroups of 256; a fault of this kind shows only at that size.  741 000 rows
    of width 32 against themselves are T = 5 790 row tiles, 724 * 725 / 2 blocks of 8 x 8 tiles and 16 797 184 workgroups, so the
    call is two launches (k14_launch), the second of the last 320 blocks: rows from 419 840, columns from 740 352.  Random rows of
    width 32 have no cosine near 0.999, so the hits are exactly the planted copies -- in the first launch, in the second, and in
    the very last tile -- and every tile of the triangle is counted once."""
    from polyfuzz_amd import _lib
    n, d = 741_000, 32
    x = np.random.default_rng(24).standard_normal((n, d), dtype=np.float32)
    planted = sorted([(0, n - 1), (5, 700_000), (300_000, 300_001), (500_000, 740_500), (740_352, 740_998)])
    for i, j in planted:
        x[j] = x[i]
    dev = _lib.DeviceDense.upload(ctx, x)
    tiles = -(-n // 128)
    row_ptr, idx, sim, counts = _lib.dense_join(ctx, dev, None, 0.999, counters=True)
    rows, cols = C.csr_pairs(row_ptr, idx)
    assert list(zip(rows.tolist(), cols.tolist())) == planted
    assert np.abs(sim.astype(np.float64) - 1.0).max() <= C.BAND
    assert counts == {"pairs": 5, "tiles": tiles * (tiles + 1) // 2, "hit_corners": 5}
    label, pairs, components, counters = _lib.dense_components(ctx, dev, 0.999, counters=True)
    want = np.arange(n, dtype=np.int32)
    for i, j in planted:
        want[j] = i
    assert label.tobytes() == want.tobytes() and (pairs, components) == (5, n - 5)
    assert counters == {"tiles": tiles * (tiles + 1) // 2, "hit_corners": 5}


def test_invalid_arguments(ctx):
    from polyfuzz_amd import _lib
    f, _ = _devs(ctx, "130x32")
    n = f.n
    for t in (float("nan"), 1.5, -0.25, float("inf"), np.nextafter(1.0, 2.0)):
        assert _raw_join(ctx, f, None, t, 4, n)[0] == -1, t
    total = ctypes.c_int64(0)
    assert ctx.lib.pfz_dense_join(ctx.h, f.h, None, 0.5, -1, np.zeros(n + 1, np.int64).ctypes.data, None, None, ctypes.byref(total), None) == -1
    pairs, comps = ctypes.c_int64(0), ctypes.c_int64(0)
    for t in (float("nan"), 1.5, -0.25):
        assert ctx.lib.pfz_dense_components(ctx.h, f.h, t, np.zeros(n, np.int32).ctypes.data, ctypes.byref(pairs), ctypes.byref(comps), None) == -1
    x = C.lists("130x32")[0]
    narrow = _lib.DeviceDense.upload(ctx, x[:, :16])
    with pytest.raises(_lib.PfzError, match="columns"):
        _lib.dense_join(ctx, f, narrow, 0.5)
    raw = _lib.DeviceDense.upload(ctx, x, normalize=False)
    half = _lib.DeviceDense.upload(ctx, x, compute_dtype="float16")
    int8 = _lib.DeviceDense.upload_int8(ctx, x)
    bits = _lib.DeviceDense.upload_bits(ctx, x)
    for bad in (raw, half, int8, bits):
        with pytest.raises(ValueError, match="fp32"):                 # the binding refuses ...
            _lib.dense_join(ctx, bad, None, 0.5)
        with pytest.raises(ValueError, match="fp32"):
            _lib.dense_join(ctx, f, bad, 0.5)
        with pytest.raises(ValueError, match="fp32"):
            _lib.dense_components(ctx, bad, 0.5)
        total = ctypes.c_int64(0)                                     # ... and so does the library
        rc = ctx.lib.pfz_dense_join(ctx.h, bad.h, None, 0.5, 0, np.zeros(n + 1, np.int64).ctypes.data, None, None, ctypes.byref(total), None)
        assert rc == -1 and (bad is raw or b"fp32" in ctx.lib.pfz_last_error())


def test_the_call_is_split_into_its_profiling_scopes(ctx):
    from polyfuzz_amd import _lib
    f, to = _devs(ctx, C.TWO_LIST_CASE)
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        _lib.dense_join(ctx, f, to, 0.8, capacity=1 << 16)
        _lib.dense_components(ctx, _devs(ctx, "300x96")[0], 0.8)
        ctx.sync()
        assert [ctx.prof_get(k)[1] for k in ("k14_join", "k14_sort_unpack", "k14_components")] == [1, 1, 1]
    finally:
        ctx.prof_enable(False)


def test_embeddings_join_frame(ctx):
    from polyfuzz_amd import linkage
    from polyfuzz_amd.models import Embeddings
    x, y = C.lists(C.TWO_LIST_CASE)
    from_list, to_list = [f"f{i}" for i in range(len(x))], [f"t{i}" for i in range(len(y))]
    m = Embeddings(cosine_method="sparse", min_similarity=0.99, top_n=1)        # (none of the three plays a part)
    frame = m.join(from_list, to_list, 0.8, embeddings_from=x, embeddings_to=y)
    rows, cols, sim = _join(ctx, C.TWO_LIST_CASE, 0.8)[:3]
    assert list(frame.columns) == ["From", "To", "Similarity"] and len(frame) == len(rows)
    assert frame["From"].tolist() == [from_list[i] for i in rows] and frame["To"].tolist() == [to_list[j] for j in cols]
    assert frame["Similarity"].to_numpy().tobytes() == sim.tobytes()
    assert m.last_counts == {"pairs": len(rows)} and set(m.last_timings) == {"device", "frame"}
    # the self-join, embedded by the model's own callable: From is the lower position of every pair
    xs, _ = C.lists("130x32")
    names = [f"s{i}" for i in range(len(xs))]
    table = dict(zip(names, xs))
    own = Embeddings(embedding_method=lambda strings: np.stack([table[s] for s in strings]))
    frame = own.join(names, min_similarity=0.9)
    given = own.join(names, min_similarity=0.9, embeddings_from=own._embed(names))
    assert len(frame) > 0 and frame.equals(given)
    pos = {s: i for i, s in enumerate(names)}
    assert all(pos[a] < pos[b] for a, b in zip(frame["From"], frame["To"]))
    # (the callable's rows are normalised in float64 first, which moves a cosine by ~1e-7; none is within 1e-5 of 0.9)
    assert len(frame) == C.ORACLE_HITS["130x32"][0.9][0]
    clusters, mapping, name_map = linkage.single_linkage(frame, 0.9)    # the frame has the columns single_linkage reads
    assert clusters and set(mapping) <= set(names)
    with pytest.raises(ValueError, match="embeddings_to"):
        own.join(names, min_similarity=0.9, embeddings_to=xs)
