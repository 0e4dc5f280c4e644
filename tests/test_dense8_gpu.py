"""GPU parity of K5's int8 path (k5_gemm8_panel: int8 vectors on the integer matrix cores, int32 accumulation) against the
float64 oracle ON THE INT8 VECTORS widened to float64 -- which is exact: an integer dot product has no rounding and no order.
Cosines are held by the rule of the fp32 and 16-bit paths (tests/helpers.py::assert_dense_topn), raw dot products bit for bit.
The bit-exact cases are also the check of the MFMA's operand lane map that its guide asks for ("with exact integer data")."""
import concurrent.futures as cf
import pickle

import numpy as np
import pytest

from tests.helpers import assert_dense_topn as _check

pytestmark = pytest.mark.gpu


def _int8(rng, shape):
    return rng.integers(-128, 128, shape, dtype=np.int8)


def _quantize(x):
    """numpy restatement of k5_quantize8: q = rint((x / max|x|) * 127) in float32, row scale max|x| / 127"""
    x = np.ascontiguousarray(x, np.float32)
    m = np.abs(x).max(axis=1, keepdims=True)
    q = np.rint((x / np.where(m > 0, m, np.float32(1))).astype(np.float32) * np.float32(127)).astype(np.int8)
    return q, (m[:, 0] / np.float32(127)).astype(np.float32)


PARITY = [(1, 1, 1, 1),            # width far below one k-chunk; one tile, mostly clamped rows
          (6, 3, 300, 2),          # the reference's fixture shape; d not a multiple of the chunk
          (300, 1000, 33, 10),     # one value past an MFMA k-step: the padding columns must be zeros in both operands
          (513, 129, 128, 128),    # exactly one k-chunk: no steady-state loop; edge tiles on both sides
          (130, 257, 768, 5),      # 6 chunks: the pipelined steady state; one row / column beyond a tile
          (130, 257, 4096, 5),     # longest accumulation chain
          (200, 1500, 128, 5)]     # more than one tile block on the to-side (the XCD mapping)


@pytest.mark.parametrize("n_a,n_b,d,ntop", PARITY)
def test_random_int8_cosine_vs_oracle(ctx, oracle_mod, n_a, n_b, d, ntop):
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(n_a + n_b + d)
    a, b = _int8(rng, (n_a, d)), _int8(rng, (n_b, d))
    idx, val = _lib.dense_int8_topn_host(ctx, a, b, ntop, 0.0)
    wa, wb = a.astype(np.float64), b.astype(np.float64)
    e_idx, e_val = oracle_mod.dense_cossim_topn(wa, wb, ntop, 0.0)
    print((n_a, n_b, d, ntop), "max |score - oracle| =", float(np.abs(val - e_val).max()),
          "rows off the oracle's order:", int((idx != e_idx).any(axis=1).sum()))
    _check(idx, val, e_idx, e_val, oracle_mod.dense_cossim(wa, wb))


def test_raw_dot_products_of_small_integers_bit_for_bit(ctx, oracle_mod):
    """values in {-1, 0, 1}, d = 16: a row holds a handful of distinct scores, so the result is the tie rule (score
    descending, column ascending) and the strict > of the bound"""
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(2)
    a = rng.integers(-1, 2, (200, 16), dtype=np.int8)
    b = rng.integers(-1, 2, (900, 16), dtype=np.int8)
    idx, val = _lib.dense_int8_topn_host(ctx, a, b, 12, 0.5, normalize=False)
    e_idx, e_val = oracle_mod.dense_cossim_topn(a.astype(np.float64), b.astype(np.float64), 12, 0.5, normalize=False)
    np.testing.assert_array_equal(idx, e_idx)
    np.testing.assert_array_equal(val.astype(np.float64), e_val)
    assert len(np.unique(val[0])) <= 6 and (val[idx >= 0] >= 1.0).all()


def test_raw_dot_products_full_range_bit_for_bit(ctx, oracle_mod):
    """130 x 257 x 1024 over the whole range; rows of -128 on both sides meet in a dot product of exactly 2^24"""
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(24)
    a, b = _int8(rng, (130, 1024)), _int8(rng, (257, 1024))
    a[[3, 77, 129]] = -128
    b[[5, 100, 256]] = -128
    idx, val = _lib.dense_int8_topn_host(ctx, a, b, 5, 0.0, normalize=False)
    dots = a.astype(np.int64) @ b.astype(np.int64).T
    assert dots.max() == 1 << 24
    e_idx, _ = oracle_mod.dense_cossim_topn(a.astype(np.float64), b.astype(np.float64), 5, 0.0, normalize=False)
    np.testing.assert_array_equal(idx, e_idx)
    expect = np.where(idx >= 0, np.take_along_axis(dots, np.maximum(idx, 0).astype(np.int64), axis=1), 0).astype(np.float32)
    np.testing.assert_array_equal(val, expect)
    np.testing.assert_array_equal(idx[3], [5, 100, 256] + e_idx[3, 3:].tolist())
    assert (val[3, :3] == np.float32(1 << 24)).all()


def test_width_limit(ctx):
    """131071 columns of -128 against the same: 2^14 * 131071 = 2^31 - 2^14, the largest sum there is, still an int32 (and a
    float32: a multiple of 128 below 2^31).  One column more is refused at upload."""
    from polyfuzz_amd import _lib
    d = 131071
    a = np.full((4, d), -128, np.int8)
    b = np.full((64, d), -128, np.int8)
    idx, val = _lib.dense_int8_topn_host(ctx, a, b, 3, 0.0, normalize=False)
    dot = 128 * 128 * d
    assert float(np.float32(dot)) == dot
    np.testing.assert_array_equal(val, np.full((4, 3), np.float32(dot)))
    np.testing.assert_array_equal(idx, np.tile(np.arange(3, dtype=np.int32), (4, 1)))
    with pytest.raises(_lib.PfzUnsupported, match="131071"):
        _lib.DeviceDense.upload_int8(ctx, np.zeros((2, d + 1), np.int8))
    with pytest.raises(_lib.PfzUnsupported, match="131071"):
        _lib.DeviceDense.upload_int8(ctx, np.zeros((2, d + 1), np.float32))


def _float_rows(rng, n, d):
    x = (rng.standard_normal((n, d)) * rng.uniform(0.2, 3.0, (n, 1))).astype(np.float32)
    x[1] = 0                                              # a zero row: zeros, scale 0
    x[2, 7] = -1.5 * np.abs(x[2]).max()                   # the extreme of the row is negative
    x[3] = np.clip(x[3], -100, 100)
    x[3, :5] = [127.0, 0.5, 1.5, 2.5, -0.5]               # maximum 127: halves, ties to even
    return x


def test_quantiser_equals_the_numpy_restatement(ctx, oracle_mod):
    """float32 input quantised on the device == the numpy restatement's int8 array handed in, bit for bit (cosines and raw
    dot products); the raw dot products are those of the dequantised rows q * scale"""
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(8)
    for n_a, n_b, d in ((150, 257, 70), (77, 130, 300)):
        x, y = _float_rows(rng, n_a, d), _float_rows(rng, n_b, d)
        (qx, sx), (qy, sy) = _quantize(x), _quantize(y)
        assert (qx[1] == 0).all() and sx[1] == 0 and qx[2, 7] == -127 and np.abs(qx).max() == 127
        assert qx[3, :5].tolist() == [127, 0, 2, 2, 0]                              # halves go to the even neighbour
        dev = _lib.dense_int8_topn_host(ctx, x, y, 5, 0.0)
        given = _lib.dense_int8_topn_host(ctx, qx, qy, 5, 0.0)
        np.testing.assert_array_equal(dev[0], given[0])
        np.testing.assert_array_equal(dev[1], given[1])
        dev64 = _lib.dense_int8_topn_host(ctx, x.astype(np.float64), y.astype(np.float64), 5, 0.0)    # any float array
        np.testing.assert_array_equal(dev64[1], given[1])
        # raw dot products: the row scales come back in
        wx, wy = qx.astype(np.float64) * sx.astype(np.float64)[:, None], qy.astype(np.float64) * sy.astype(np.float64)[:, None]
        idx, val = _lib.dense_int8_topn_host(ctx, x, y, 6, 0.5, normalize=False)
        e_idx, e_val = oracle_mod.dense_cossim_topn(wx, wy, 6, 0.5, normalize=False)
        dots = oracle_mod.dense_cossim(wx, wy, normalize=False)
        print((n_a, n_b, d), "raw dots: max rel err", float((np.abs(val - e_val) / np.maximum(np.abs(e_val), 1.0)).max()))
        np.testing.assert_allclose(val, e_val, rtol=2e-6, atol=2e-5)
        bad = np.nonzero((idx != e_idx).any(axis=1))[0]
        for i in bad:                                    # only fp32-level near-ties may swap
            for r in range(idx.shape[1]):
                if idx[i, r] != e_idx[i, r]:
                    s_got = dots[i, idx[i, r]] if idx[i, r] >= 0 else 0.0
                    assert abs(s_got - e_val[i, r]) < 1e-4 * max(1.0, abs(e_val[i, r]))
        assert len(bad) <= 3
        h = _lib.DeviceDense.upload_int8(ctx, x)
        assert h.dtype == "int8" and (h.n, h.dim) == (n_a, d)


def test_quantisation_cost_on_unit_gaussian_vectors(ctx, oracle_mod):
    """What quantising float32 embeddings costs (the figure the documents quote): 300 x 2000 unit-Gaussian vectors at d = 768.
    Bound: a row x and its dequantised q * scale enclose an angle of at most asin(|x - q scale| / |x|), and the cosine of two
    vectors moves by at most the sum of the angles each of them moves by."""
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(768)
    a = rng.standard_normal((300, 768)).astype(np.float32)
    b = rng.standard_normal((2000, 768)).astype(np.float32)
    idx, val = _lib.dense_int8_topn_host(ctx, a, b, 1, 0.0)
    exact = oracle_mod.dense_cossim(a, b)

    def angle(x):
        q, s = _quantize(x)
        x = x.astype(np.float64)
        return np.arcsin(np.linalg.norm(x - q * s.astype(np.float64)[:, None], axis=1) / np.linalg.norm(x, axis=1)).max()
    qa, qb = _quantize(a)[0].astype(np.float64), _quantize(b)[0].astype(np.float64)
    worst = float(np.abs(oracle_mod.dense_cossim(qa, qb) - exact).max())
    top1_kept = int((idx[:, 0] == exact.argmax(axis=1)).sum())
    print(f"int8 quantisation: worst |cos_int8 - cos_fp32| = {worst:.3e}, bound {angle(a) + angle(b):.3e}; top-1 kept in "
          f"{top1_kept} of 300 rows")
    assert worst <= angle(a) + angle(b)
    got = np.abs(val[:, 0] - exact[np.arange(300), idx[:, 0]]).max()
    assert got <= angle(a) + angle(b) + 1e-5


def test_self_match_and_lower_bound(ctx, oracle_mod):
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(9)
    a = _int8(rng, (400, 96))
    a[100:110] = np.clip(a[:10].astype(np.int32) + rng.integers(-6, 7, (10, 96)), -128, 127).astype(np.int8)   # near-duplicates
    w = a.astype(np.float64)
    idx, val = _lib.dense_int8_topn_host(ctx, a, a, 3, 0.2, exclude_diag=True)
    e_idx, e_val = oracle_mod.dense_cossim_topn(w, w, 3, 0.2, exclude_diag=True)
    _check(idx, val, e_idx, e_val, oracle_mod.dense_cossim(w, w))
    assert (idx != np.arange(400)[:, None]).all()                                       # row i never comes back for row i
    assert (idx[:10, 0] == np.arange(100, 110)).all() and (idx[100:110, 0] == np.arange(10)).all()
    assert (idx < 0).any() and (val[idx >= 0] > 0.2).all()                              # the bound does cut
    a[200:203] = a[50]                                                                  # exact duplicates: lowest index first
    idx, _ = _lib.dense_int8_topn_host(ctx, a, a, 3, 0.2, exclude_diag=True)
    np.testing.assert_array_equal(idx[50], [200, 201, 202])
    np.testing.assert_array_equal(idx[201], [50, 200, 202])


def test_block_maxima_and_panels(ctx, oracle_mod, monkeypatch):
    """333 x 1500 x 64 with duplicates in four different 64-column blocks, three (bound, self) settings.
    PFZ_K5_NO_BLOCK_MAX, PFZ_K5_PANEL_ROWS=256 and neither: equal bit for bit, and the oracle's result.
    The five equal columns have ONE score here (integer sums, one pair of factors) and come out in ascending order; the
    oracle's float64 product may round them one ulp apart and order them otherwise.  The rule's row cap covers that whatever
    the oracle does: the rows that hold two or more of the five in their top ten are 2 of 333 (cap 3), 1 with the bound
    (cap 3) and 13 of 1500 in the self-match (cap 15) -- which is why only ONE from-row is made a near-duplicate."""
    from polyfuzz_amd import _lib
    ntop = 10
    rng = np.random.default_rng(77 + ntop)
    d = 64
    b = _int8(rng, (1500, d))
    for j in (70, 700, 1400, 1499):
        b[j] = b[5]
    a = _int8(rng, (333, d))
    a[0] = np.clip(b[5].astype(np.int32) + rng.integers(-40, 41, d), -128, 127).astype(np.int8)
    wa, wb = a.astype(np.float64), b.astype(np.float64)
    for lb, self_match in ((0.0, False), (0.35, False), (0.0, True)):
        (x, wx), (y, wy) = ((b, wb), (b, wb)) if self_match else ((a, wa), (b, wb))
        monkeypatch.setenv("PFZ_K5_NO_BLOCK_MAX", "1")
        full = _lib.dense_int8_topn_host(ctx, x, y, ntop, lb, exclude_diag=self_match)
        monkeypatch.delenv("PFZ_K5_NO_BLOCK_MAX")
        fast = _lib.dense_int8_topn_host(ctx, x, y, ntop, lb, exclude_diag=self_match)
        np.testing.assert_array_equal(fast[0], full[0])
        np.testing.assert_array_equal(fast[1], full[1])
        monkeypatch.setenv("PFZ_K5_PANEL_ROWS", "256")
        paneled = _lib.dense_int8_topn_host(ctx, x, y, ntop, lb, exclude_diag=self_match)
        monkeypatch.delenv("PFZ_K5_PANEL_ROWS")
        np.testing.assert_array_equal(paneled[0], full[0])
        np.testing.assert_array_equal(paneled[1], full[1])
        e_idx, e_val = oracle_mod.dense_cossim_topn(wx, wy, ntop, lb, exclude_diag=self_match)
        _check(fast[0], fast[1], e_idx, e_val, oracle_mod.dense_cossim(wx, wy))
        if self_match:
            assert (fast[0] != np.arange(len(x))[:, None]).all()
            assert fast[0][5, 0] == 70 and fast[0][70, 0] == 5          # duplicates find each other, lowest index first
        else:
            np.testing.assert_array_equal(fast[0][0, :5], [5, 70, 700, 1400, 1499])


def test_deep_top_n(ctx, oracle_mod, monkeypatch):
    """70 x 3000 x 24, top 2500 in passes of 1024 over 128-row panels, held as tests/test_dense16_gpu.py::test_deep_top_n
    holds it: scores within 1e-5; an index differs only where the oracle's score of the chosen column is within 4e-6 of the
    expected one, in at most 1 / 100 of the result entries; no column twice; forty duplicates in ascending order."""
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(70 + 2500)
    a = _int8(rng, (70, 24))
    b = _int8(rng, (3000, 24))
    # an integer dot product can be exactly 0, which is "no match" here and a rounding residue of either sign in the
    # oracle's float64 product of normalised rows: a's values are even except its first column, b's first column is odd, so
    # every dot product is odd
    a &= ~np.int8(1)
    a[:, 0] |= 1
    b[:, 0] |= 1
    b[100:140] = b[50]                             # forty exact duplicates: one score, forty columns in ascending order
    wa, wb = a.astype(np.float64), b.astype(np.float64)
    monkeypatch.setenv("PFZ_K5_PANEL_ROWS", "128")
    idx, val = _lib.dense_int8_topn_host(ctx, a, b, 2500, 0.0)
    e_idx, e_val = oracle_mod.dense_cossim_topn(wa, wb, 2500, 0.0, chunk_rows=64)
    dense = oracle_mod.dense_cossim(wa, wb)
    np.testing.assert_allclose(val, e_val, rtol=0, atol=1e-5)
    assert ((idx < 0) == (e_idx < 0)).all() and (idx < 0).any()
    rr, cc = np.nonzero(idx != e_idx)
    print("deep top-n: entries off the oracle's order:", len(rr), "of", idx.size)
    assert np.abs(dense[rr, idx[rr, cc]] - e_val[rr, cc]).max(initial=0.0) < 4e-6
    assert len(rr) <= max(1, idx.size // 100)
    for i in range(70):
        real = idx[i][idx[i] >= 0]
        assert len(set(real.tolist())) == len(real)
    dup_rows = np.nonzero((idx == 100).any(axis=1))[0]
    assert len(dup_rows) > 0
    for i in dup_rows[:10]:
        at = int(np.nonzero(idx[i] == 50)[0][0])
        np.testing.assert_array_equal(idx[i, at:at + 41], [50] + list(range(100, 140)))


def test_mixed_operand_types_raise(ctx):
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(3)
    a = rng.standard_normal((10, 64)).astype(np.float32)
    h8 = _lib.DeviceDense.upload_int8(ctx, a)
    others = {"float32": _lib.DeviceDense.upload(ctx, a, True), "float16": _lib.DeviceDense.upload(ctx, a, True, "float16"),
              "bfloat16": _lib.DeviceDense.upload(ctx, a, True, "bfloat16")}
    for name, h in others.items():
        with pytest.raises(_lib.PfzError, match=f"int8.*{name}"):
            _lib.dense_topn(ctx, h8, h, 2, 0.0)
        with pytest.raises(_lib.PfzError, match=f"{name}.*int8"):
            _lib.dense_topn(ctx, h, h8, 2, 0.0)
    with pytest.raises(ValueError, match="unsigned"):
        _lib.DeviceDense.upload_int8(ctx, np.zeros((3, 4), np.uint8))
    for h in [h8] + list(others.values()):                                     # the handles are still good
        idx, val = _lib.dense_topn(ctx, h, h, 1, 0.0).download()
        np.testing.assert_array_equal(idx[:, 0], np.arange(10))


def test_embeddings_with_int8_precision(ctx):
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import Embeddings
    rng = np.random.default_rng(21)
    a = rng.standard_normal((301, 96)).astype(np.float32)
    b = rng.standard_normal((530, 96)).astype(np.float32)
    qa, qb = _quantize(a)[0], _quantize(b)[0]
    fl, tl = [f"f{i}" for i in range(len(a))], [f"t{i}" for i in range(len(b))]
    ref_idx, ref_val = _lib.dense_int8_topn_host(ctx, qa, qb, 4, 0.0)
    m = Embeddings(min_similarity=0.0, top_n=4, cosine_method="hip")
    m.precision = "int8"
    df = m.match(fl, tl, embeddings_from=qa, embeddings_to=qb)                      # int8 arrays in
    assert df["To"].tolist() == [tl[j] for j in ref_idx[:, 0]]
    assert df["To_3"].tolist() == [tl[j] for j in ref_idx[:, 2]]
    np.testing.assert_array_equal(df["Similarity"].to_numpy(), np.round(ref_val[:, 0].astype(np.float64), 3))   # (the frame's rounding)
    assert m.match(fl, tl, embeddings_from=a, embeddings_to=b).equals(df)          # float arrays in: quantised per row
    resident = m._dev_to
    assert resident.dtype == "int8"
    df2 = m.match(fl[:50], tl, embeddings_from=a[:50], re_train=False)              # to-side: resident, not re-uploaded
    assert m._dev_to is resident
    assert df2["To_3"].tolist() == [tl[j] for j in ref_idx[:50, 2]]
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.precision == "int8"
    assert m2.match(fl[:50], tl, embeddings_from=a[:50], re_train=False).equals(df2)
    m.precision = None                                                              # the resident to-side follows the type
    f_idx, _ = _lib.dense_cossim_topn_host(ctx, a[:50], b, 4, 0.0)
    df3 = m.match(fl[:50], tl, embeddings_from=a[:50], re_train=False)
    assert m._dev_to is not resident and m._dev_to.dtype == "float32"
    assert df3["To"].tolist() == [tl[j] for j in f_idx[:, 0]]
    m.precision, m.compute_dtype = "int8", "float16"
    with pytest.raises(ValueError, match="precision.*compute_dtype"):
        m.match(fl[:50], tl, embeddings_from=a[:50], re_train=False)
    e = Embeddings(embedding_method=lambda strings: a[[int(s[1:]) for s in strings]], min_similarity=0.0, top_n=4,
                   cosine_method="hip")
    e.precision = "int8"                                                            # what an embedding_method returns
    assert e.match(fl[:50], fl)["To"].tolist() == fl[:50] and e._dev_to.dtype == "int8"


def test_sharded_dense_job_int8(ctx):
    """DenseMatchJob on two contexts of one device with uneven shards and resident int8 handles == the one-shot call, bit
    for bit."""
    import polyfuzz_amd
    from polyfuzz_amd import _lib, pipeline
    rng = np.random.default_rng(21)
    a, b = _int8(rng, (301, 96)), _int8(rng, (530, 96))
    ctxs = [polyfuzz_amd.Context(0), polyfuzz_amd.Context(0)]
    comms = _lib.Comm.local_group(ctxs)
    bounds = [pipeline.shard_bounds(len(a), 2, r) for r in range(2)]
    sizes = [e - s for s, e in bounds]

    def rank_fn(r, self_match):
        s, e = bounds[r]
        job = pipeline.DenseMatchJob(ctxs[r], _lib.DeviceDense.upload_int8(ctxs[r], a[s:e]),
                                     _lib.DeviceDense.upload_int8(ctxs[r], a if self_match else b), top_n=4, comm=comms[r],
                                     rows_per_rank=max(sizes), self_match=self_match, shard_offset=s if self_match else 0)
        assert job.from_dev.dtype == "int8" and job.to_dev.dtype == "int8" and (job.n_from, job.n_to) == (e - s, job.to_dev.n)
        idx, val = job.step().download()
        return pipeline.TfidfMatchJob.unpad(idx, val, sizes, max(sizes))

    for self_match in (False, True):
        exp = _lib.dense_int8_topn_host(ctx, a, a if self_match else b, 4, 0.0, exclude_diag=self_match)
        with cf.ThreadPoolExecutor(2) as ex:
            outs = [f.result(timeout=120) for f in [ex.submit(rank_fn, r, self_match) for r in range(2)]]
        for idx, val in outs:
            np.testing.assert_array_equal(idx, exp[0])
            np.testing.assert_array_equal(val, exp[1])
    for c in comms:
        c.free()
