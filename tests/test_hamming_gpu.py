"""GPU tests of the 1-bit dense path: k5_pack_signs, k5_hamming_panel under K5's row top-n, pfz_dense_upload1 and the doors
above it.  Everything is held BIT FOR BIT to the numpy oracle of tests/test_hamming_cpu.py: Hamming scores are exact
functions of an integer, so the indices must be equal and the values equal as float32 bits -- no tolerance.  Scores take
only d + 1 values: ties are everywhere, and the column-ascending rule decides most rows."""
import pickle

import numpy as np
import pytest

from tests.test_hamming_cpu import hamming_topn, pack, scores, topn

pytestmark = pytest.mark.gpu


def _bits(rng, n, d):
    """n random packed rows of d bits (d a multiple of 8)"""
    return rng.integers(0, 256, (n, d // 8), dtype=np.uint8)


def _same(got, want, what=""):
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"indices {what}")
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32), err_msg=f"score bits {what}")


def _run(ctx, a, b, ntop, lower_bound=0.0, exclude_diag=False, normalize=True):
    from polyfuzz_amd import _lib
    return _lib.dense_hamming_topn_host(ctx, a, b, ntop, lower_bound, exclude_diag, normalize)


SHAPES = [(1, 1, 8),
          (3, 5, 64),
          (63, 129, 96),            # a pitch with padding (96 bits in 128), edges that are no tile multiples
          (129, 257, 768),          # one row and one column beyond a tile
          (300, 2000, 768),         # several tiles each way, a partly filled last 256-column step
          (70, 300, 4104)]          # 513 bytes: a row wider than one LDS stage (five chunks, the last one 16 bytes)


@pytest.mark.parametrize("n_from,n_to,d", SHAPES)
def test_shapes_and_options(ctx, n_from, n_to, d):
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(n_from + n_to + d)
    a, b = _bits(rng, n_from, d), _bits(rng, n_to, d)
    s = scores(a, b, d)
    ha, hb = _lib.DeviceDense.upload_bits(ctx, a), _lib.DeviceDense.upload_bits(ctx, b)
    assert (ha.dtype, ha.n, ha.dim, hb.n, hb.dim) == ("binary", n_from, d, n_to, d)
    for ntop in (1, 5, 130, n_to + 3):                  # 130: the wide candidate buffer; beyond n_to: the tail is (-1, 0)
        got = _lib.dense_topn(ctx, ha, hb, ntop, 0.0).download()
        _same(got, topn(s, ntop), f"top_n {ntop}")
        assert ((got[0] < 0) == (got[1] == 0)).all()
    # a lower bound that cuts: ON a score the data has (strict: that score is dropped) and between two
    positive = np.unique(s[s > 0])
    for bound in ([float(positive[len(positive) // 2]), float(positive[len(positive) // 2]) + 1e-4] if len(positive) else [0.5]):
        _same(_lib.dense_topn(ctx, ha, hb, 5, bound).download(), topn(s, 5, bound), f"bound {bound}")
    raw = scores(a, b, d, normalize=False)
    _same(_run(ctx, a, b, 5, 0.0, normalize=False), topn(raw, 5), "dot products")
    _same(_run(ctx, a, b, 5, 2.0, normalize=False), topn(raw, 5, 2.0), "dot products above 2")


def test_self_match_excludes_the_diagonal(ctx):
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(7)
    a = _bits(rng, 300, 96)
    a[200:210] = a[5]                                    # copies: score 1.0 off the diagonal, in column order
    s = scores(a, a, 96)
    h = _lib.DeviceDense.upload_bits(ctx, a)
    for ntop in (1, 4, 130):
        got = _lib.dense_topn(ctx, h, h, ntop, 0.0, exclude_diag=True).download()
        _same(got, topn(s, ntop, exclude_diag=True), f"self-match top_n {ntop}")
        assert (got[0] != np.arange(300)[:, None]).all()
    got = _lib.dense_topn(ctx, h, h, 3, 0.0, exclude_diag=True).download()
    assert got[0][5].tolist() == [200, 201, 202] and got[1][5].tolist() == [1.0, 1.0, 1.0]
    assert got[0][203].tolist() == [5, 200, 201]
    _same(_run(ctx, a, a, 4, 0.0, exclude_diag=True), topn(s, 4, exclude_diag=True), "one handle for both sides")
    # a shard of the rows: the diagonal sits at an offset
    part = _lib.DeviceDense.upload_bits(ctx, a[100:])
    got = _lib.dense_topn(ctx, part, h, 4, 0.0, exclude_diag=True, diag_offset=100).download()
    _same(got, topn(s[100:], 4, exclude_diag=True, diag_offset=100), "diag_offset")


def _clustered(rng, n_from, n_to, d):
    """rows around one base row: every pair scores positive, with few distinct values -- long runs of ties"""
    base = rng.integers(0, 2, d, dtype=np.uint8)
    a = np.packbits(base ^ (rng.random((n_from, d)) < 0.1), axis=1)
    b = np.packbits(base ^ (rng.random((n_to, d)) < 0.2), axis=1)
    return a, b


def test_deep_top_n(ctx, monkeypatch):
    """top_n = 1100 of 1500 to-rows: two passes of the deep top-n over the Hamming panel, the second continuing below the
    last key of the first -- in the middle of a run of equal scores."""
    rng = np.random.default_rng(11)
    a, b = _clustered(rng, 40, 1500, 256)
    s = scores(a, b, 256)
    assert (s > 0).sum(axis=1).min() >= 1100 and len(np.unique(s)) < 200
    want = topn(s, 1100)
    assert (want[1][:, 1023] == want[1][:, 1024]).any()                # a tie across the pass boundary
    _same(_run(ctx, a, b, 1100, 0.0), want, "deep")
    monkeypatch.setenv("PFZ_K5_PANEL_ROWS", "128")
    a3 = np.concatenate([a] * 7)                                       # 280 rows: three panels
    _same(_run(ctx, a3, b, 1100, 0.0), tuple(np.concatenate([w] * 7) for w in want), "deep, three panels")


def test_panels_and_block_maxima(ctx, monkeypatch):
    """The same search in one panel, in panels of 128 rows (two buffers, the side stream) and without the block maxima
    (M == nullptr: the row top-n streams the panel): one result, the oracle's."""
    rng = np.random.default_rng(12)
    a, b = _bits(rng, 300, 768), _bits(rng, 2000, 768)
    a2, b2 = _clustered(rng, 300, 700, 200)
    for x, y, d in ((a, b, 768), (a2, b2, 200)):
        for ntop in (5, 130):
            want = hamming_topn(x, y, d, ntop)
            _same(_run(ctx, x, y, ntop), want, "plain")
            monkeypatch.setenv("PFZ_K5_PANEL_ROWS", "128")
            _same(_run(ctx, x, y, ntop), want, "panels of 128 rows")
            monkeypatch.delenv("PFZ_K5_PANEL_ROWS")
            monkeypatch.setenv("PFZ_K5_NO_BLOCK_MAX", "1")
            _same(_run(ctx, x, y, ntop), want, "no block maxima")
            monkeypatch.setenv("PFZ_K5_PANEL_ROWS", "128")
            _same(_run(ctx, x, y, ntop), want, "no block maxima, panels of 128 rows")
            monkeypatch.delenv("PFZ_K5_PANEL_ROWS")
            monkeypatch.delenv("PFZ_K5_NO_BLOCK_MAX")


def test_degenerate_rows(ctx):
    rng = np.random.default_rng(13)
    d = 200
    a = _bits(rng, 70, d)
    # all to-rows equal: one score per from-row, columns 0, 1, 2, ... in order
    b = np.repeat(a[3:4], 300, axis=0)
    idx, val = _run(ctx, a, b, 7, 0.0)
    _same((idx, val), hamming_topn(a, b, d, 7), "equal to-rows")
    hit = val[:, 0] > 0
    assert hit.sum() > 10 and (idx[hit] == np.arange(7)).all() and (idx[~hit] == -1).all()
    assert val[3].tolist() == [1.0] * 7                                 # an exact copy scores 1.0
    # a complemented row never matches; the copy beside it does, at 1.0
    b = _bits(rng, 300, d)
    b[17], b[18], b[250] = ~a[0], a[0], ~a[0]
    idx, val = _run(ctx, a, b, 300, 0.0)
    _same((idx, val), hamming_topn(a, b, d, 300), "complement")
    assert idx[0, 0] == 18 and val[0, 0] == 1.0 and 17 not in idx[0] and 250 not in idx[0]
    assert _run(ctx, a[:1], np.stack([~a[0]] * 5), 2, 0.0)[0].tolist() == [[-1, -1]]
    # all-zero rows: equal to each other (score 1.0), and against random rows d - 2 popcount
    z = np.zeros((5, d // 8), np.uint8)
    idx, val = _run(ctx, z, z, 3, 0.0)
    assert idx.tolist() == [[0, 1, 2]] * 5 and (val == 1.0).all()
    zb = np.concatenate([b[:100], z, b[100:]])
    _same(_run(ctx, z, zb, 9, 0.0), hamming_topn(z, zb, d, 9), "zero from-rows")
    _same(_run(ctx, a, zb, 9, 0.0), hamming_topn(a, zb, d, 9), "zero rows among the to-rows")
    _same(_run(ctx, zb, zb, 6, 0.0, exclude_diag=True), hamming_topn(zb, zb, d, 6, exclude_diag=True), "zero rows, self-match")


def _floats(rng, n, dim):
    """unit Gaussians with NaN, -0.0, 0.0, infinities and denormals sprinkled in: x > 0 is False for the first three"""
    x = rng.standard_normal((n, dim)).astype(np.float32)
    for value in (np.nan, -0.0, 0.0, np.inf, -np.inf, 1e-45, -1e-45):
        x[rng.random((n, dim)) < 0.02] = value
    head = np.array([np.nan, -0.0, 0.0, 1.0, -1.0, np.inf, -np.inf, 1e-45], np.float32)[:dim]
    x[0, :len(head)] = head
    x[-1, -3:] = [np.nan, 0.0, 2.0]
    return x


@pytest.mark.parametrize("dim", [768, 1000, 1003, 5])
def test_device_packing_equals_packbits(ctx, dim):
    """float rows packed by k5_pack_signs give the result of np.packbits(x > 0, axis=1) uploaded as it is -- which can only be
    said where the two forms have one d, dim % 8 == 0 -- and always the oracle's with d = dim."""
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(dim)
    a, b = _floats(rng, 65, dim), _floats(rng, 300, dim)
    pa, pb = pack(a), pack(b)
    ha = _lib.DeviceDense.upload_bits(ctx, a)
    assert (ha.dtype, ha.dim) == ("binary", dim)
    for ntop, normalize in ((5, True), (130, True), (5, False)):
        got = _run(ctx, a, b, ntop, 0.0, normalize=normalize)
        _same(got, topn(scores(pa, pb, dim, normalize), ntop), f"device-packed, d = {dim}")
        if dim % 8 == 0:
            _same(got, _run(ctx, pa, pb, ntop, 0.0, normalize=normalize), "device-packed against host-packed")
            _same(got, _run(ctx, a.astype(np.float64), pb, ntop, 0.0, normalize=normalize), "one side each")
    if dim % 8:
        # host-packed rows count 8 bits per byte: the two forms have different d and are refused, with the reason
        with pytest.raises(ValueError, match="not a multiple of 8"):
            _run(ctx, a, pb, 5, 0.0)
        with pytest.raises(_lib.PfzError, match="not a multiple of 8"):
            _lib.dense_topn(ctx, ha, _lib.DeviceDense.upload_bits(ctx, pb), 5, 0.0)


def test_refusals_on_the_device(ctx):
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(3)
    bits = _lib.DeviceDense.upload_bits(ctx, _bits(rng, 4, 64))
    for other in (_lib.DeviceDense.upload(ctx, np.ones((4, 64), np.float32)), _lib.DeviceDense.upload_int8(ctx, np.ones((4, 64), np.int8))):
        with pytest.raises(_lib.PfzError, match="binary"):              # pfz_dense_topn still refuses operands of two types
            _lib.dense_topn(ctx, bits, other, 1, 0.0)
        with pytest.raises(_lib.PfzError, match="binary"):
            _lib.dense_topn(ctx, other, bits, 1, 0.0)
    raw = _lib.DeviceDense.upload_bits(ctx, _bits(rng, 4, 64), normalize=False)
    with pytest.raises(_lib.PfzError, match="normalize"):
        _lib.dense_topn(ctx, bits, raw, 1, 0.0)
    with pytest.raises(_lib.PfzError, match="float32"):                 # a bit handle is no exact operand of the rescoring
        _lib.dense_rescore(ctx, bits, bits, _lib.DeviceTopN.alloc(ctx, 4, 2), 1, 0.0)
    with pytest.raises(_lib.PfzError, match="exceed"):                  # d < 2^24
        _lib.DeviceDense.upload_bits(ctx, np.zeros((1, 1 << 21), np.uint8))
    empty = _lib.DeviceDense.upload_bits(ctx, np.zeros((0, 8), np.uint8))
    assert (empty.n, empty.dim) == (0, 64)
    idx, val = _lib.dense_topn(ctx, bits, empty, 2, 0.0).download()
    assert (idx == -1).all() and (val == 0).all()


def test_binary_and_ubinary_arrays_are_one_operand(ctx):
    """sentence-transformers' int8 "binary" is ubinary - 128: the same rows, whichever side carries which form"""
    rng = np.random.default_rng(14)
    ua, ub = _bits(rng, 129, 768), _bits(rng, 257, 768)
    ba, bb = ((u.astype(np.int16) - 128).astype(np.int8) for u in (ua, ub))
    want = hamming_topn(ua, ub, 768, 6)
    _same(hamming_topn(ba, bb, 768, 6), want, "the oracle's own two forms")
    for x, y in ((ua, ub), (ba, bb), (ua, bb), (ba, ub)):
        _same(_run(ctx, x, y, 6), want, f"{x.dtype} x {y.dtype}")


def test_embeddings_binary_attribute(ctx):
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import Embeddings
    rng = np.random.default_rng(21)
    a = rng.standard_normal((301, 96)).astype(np.float32)
    b = rng.standard_normal((530, 96)).astype(np.float32)
    pa, pb = pack(a), pack(b)
    fl, tl = [f"f{i}" for i in range(len(a))], [f"t{i}" for i in range(len(b))]
    ref_idx, ref_val = _lib.dense_hamming_topn_host(ctx, pa, pb, 4, 0.0)
    _same((ref_idx, ref_val), hamming_topn(pa, pb, 96, 4))
    assert (ref_idx >= 0).all()
    m = Embeddings(min_similarity=0.0, top_n=4, cosine_method="hip")
    m.binary = "ubinary"
    df = m.match(fl, tl, embeddings_from=pa, embeddings_to=pb)                      # packed uint8 rows in
    assert df["To"].tolist() == [tl[j] for j in ref_idx[:, 0]]
    assert df["To_3"].tolist() == [tl[j] for j in ref_idx[:, 2]]
    np.testing.assert_array_equal(df["Similarity"].to_numpy(), np.round(ref_val[:, 0].astype(np.float64), 3))   # (the frame's rounding)
    assert m.match(fl, tl, embeddings_from=a, embeddings_to=b).equals(df)          # float arrays in: packed on the device
    m.binary = "binary"                                                             # the other spelling: the same path
    assert m.match(fl, tl, embeddings_from=(pa.astype(np.int16) - 128).astype(np.int8), embeddings_to=pb).equals(df)
    resident = m._dev_to
    assert resident.dtype == "binary" and resident.dim == 96
    df2 = m.match(fl[:50], tl, embeddings_from=a[:50], re_train=False)              # to-side: resident, not re-uploaded
    assert m._dev_to is resident
    assert df2["To_3"].tolist() == [tl[j] for j in ref_idx[:50, 2]]
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.binary == "binary"
    assert m2.match(fl[:50], tl, embeddings_from=a[:50], re_train=False).equals(df2)
    # "sparse": the dot product d - 2 h, min_similarity honoured
    sp = Embeddings(min_similarity=20.0, top_n=2, cosine_method="sparse")
    sp.binary = "ubinary"
    d_idx, d_val = hamming_topn(pa, pb, 96, 2, lower_bound=20.0, normalize=False)
    dfs = sp.match(fl, tl, embeddings_from=pa, embeddings_to=pb)
    assert dfs["To"].tolist() == [tl[j] if j >= 0 else None for j in d_idx[:, 0]]
    np.testing.assert_array_equal(dfs["Similarity"].to_numpy(), d_val[:, 0].astype(np.float64))
    # self-match through an embedding_method; a width mismatch names its reason
    e = Embeddings(embedding_method=lambda strings: a[[int(s[1:]) for s in strings]], min_similarity=0.0, top_n=2, cosine_method="hip")
    e.binary = "ubinary"
    s_idx, _ = hamming_topn(pa[:50], pa[:50], 96, 2, exclude_diag=True)
    assert e.match(fl[:50])["To"].tolist() == [fl[j] for j in s_idx[:, 0]] and e._dev_to.dtype == "binary"
    with pytest.raises(ValueError, match="not a multiple of 8"):
        m.match(fl[:5], tl, embeddings_from=a[:5, :93], embeddings_to=pb)
    m.binary = None                                                                 # the resident to-side follows the type
    f_idx, _ = _lib.dense_cossim_topn_host(ctx, a[:50], b, 4, 0.0)
    df3 = m.match(fl[:50], tl, embeddings_from=a[:50], embeddings_to=b)
    assert m._dev_to.dtype == "float32" and df3["To"].tolist() == [tl[j] for j in f_idx[:, 0]]


def test_dense_match_job_on_bit_handles(ctx):
    from polyfuzz_amd import _lib, pipeline
    rng = np.random.default_rng(22)
    a = rng.standard_normal((130, 96)).astype(np.float32)
    b = rng.standard_normal((530, 96)).astype(np.float32)
    ha, hb = _lib.DeviceDense.upload_bits(ctx, pack(a)), _lib.DeviceDense.upload_bits(ctx, b)
    job = pipeline.DenseMatchJob(ctx, ha, hb, top_n=4)
    _same(job.step().download(), hamming_topn(pack(a), pack(b), 96, 4), "resident bit handles")
    _same(job.step().download(), hamming_topn(pack(a), pack(b), 96, 4), "a second step")
    own = pipeline.DenseMatchJob(ctx, hb, None, top_n=3, self_match=True)
    _same(own.step().download(), hamming_topn(pack(b), pack(b), 96, 3, exclude_diag=True), "self-match")
    rescored = pipeline.DenseMatchJob(ctx, ha, hb, top_n=4, min_similarity=0.05, rescore_multiplier=4, rescore_from=a, rescore_to=b)
    _same(rescored.step().download(), _lib.dense_rescored_topn_host(ctx, a, b, 4, 0.05, coarse="binary", multiplier=4), "rescored")
    with pytest.raises(ValueError, match="float32 form"):
        pipeline.DenseMatchJob(ctx, ha, hb, top_n=4, rescore_multiplier=4, rescore_from=ha, rescore_to=hb)


def test_binary_search_with_exact_rescoring(ctx, oracle_mod):
    """How such embeddings are normally used: an oversampled Hamming search, then the exact scores of those candidates.
    300 x 2000 unit-Gaussian vectors of width 768 (the generator call of tests/test_dense_rescore_gpu.py), top-5.  Hamming is
    exact, so the candidate set is known: the result must be that of a numpy simulation -- Hamming top-(5 m) by the tie rule,
    float64 scores of those columns, their top-5.  Columns may differ only where the float64 scores of the two columns are
    within 1e-6 of each other; every score is within the project's 1e-5 of the float64 value.
    Measured on an MI355X (printed below; a measurement, not a condition): the result is the plain float64 top-5 in 0 / 0 / 21 of
    300 rows at multipliers 1 / 4 / 16, the candidates holding 222 / 492 / 907 of its 1 500 entries."""
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import Embeddings
    rng = np.random.default_rng(768)
    a = rng.standard_normal((300, 768)).astype(np.float32)
    b = rng.standard_normal((2000, 768)).astype(np.float32)
    dense = oracle_mod.dense_cossim(a, b)
    e_idx, _ = oracle_mod.dense_cossim_topn(a, b, 5, 0.0)
    pa, pb = pack(a), pack(b)
    fl, tl = [f"f{i}" for i in range(300)], [f"t{i}" for i in range(2000)]
    rows = np.arange(300)[:, None]
    for mult in (1, 4, 16):
        cand, _ = hamming_topn(pa, pb, 768, 5 * mult)
        w_idx = np.full((300, 5), -1, np.int32)
        w_val = np.zeros((300, 5))
        for i in range(300):
            cols = cand[i][cand[i] >= 0].astype(np.int64)
            sc = dense[i, cols]
            order = np.lexsort((cols, -sc))
            order = order[sc[order] > 0.0][:5]
            w_idx[i, :len(order)], w_val[i, :len(order)] = cols[order], sc[order]
        idx, val = _lib.dense_rescored_topn_host(ctx, a, b, 5, 0.0, coarse="binary", multiplier=mult)
        agree = int((idx == e_idx).all(axis=1).sum())
        print(f"binary x{mult}: rows whose top-5 is the float64 oracle's: {agree} of 300; exact top-5 entries among the candidates: "
              f"{int(sum(len(np.intersect1d(e_idx[i], cand[i])) for i in range(300)))} of 1500; "
              f"max |score - float64| = {float(np.abs(val - w_val).max()):.2e}")
        assert ((idx < 0) == (w_idx < 0)).all()
        assert np.abs(val - w_val).max() <= 1e-5
        off = (idx != w_idx) & (idx >= 0)
        got_score = np.where(idx >= 0, dense[rows, np.maximum(idx, 0)], 0.0)
        assert (np.abs(got_score - w_val)[off] <= 1e-6).all(), "columns differ where the float64 scores are further than 1e-6 apart"
        if mult == 4:                                   # the same through the matcher
            m = Embeddings(min_similarity=0.0, top_n=5, cosine_method="hip")
            m.binary, m.rescore_multiplier = "ubinary", 4
            df = m.match(fl, tl, embeddings_from=a, embeddings_to=b)
            assert df["To"].tolist() == [tl[j] for j in idx[:, 0]] and df["To_5"].tolist() == [tl[j] for j in idx[:, 4]]
            assert m._dev_to.dtype == "binary" and m._dev_to_exact.dtype == "float32"
