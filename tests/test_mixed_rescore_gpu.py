"""GPU tests of the mixed rescoring (k5_mixed_rescore, pfz_dense_rescore_topn_mixed and the doors above it): the float32
from-vectors scored against an int8 or a 1-bit to-operand itself, so that no float32 to-side has to exist.
The expected values are built here from numpy float64: for int8 rows q the cosine (a / ||a||) . (q / ||q||) or the dot product
a . q (times the row's scale for rows quantised on the device); for bit rows, with s = +-1 as the bit says, the cosine
(a / ||a||) . (s / sqrt(d)) or a . s.  The expected result of a candidate-restricted search is those scores over the row's
candidate columns by (score descending, column ascending), strict > on the bound.  The acceptance rule is the dense tests' own
(tests/helpers.py::assert_dense_topn): 1e-5 absolute on the scores; an index may differ only where the float64 score of the
chosen column is within 4e-6 of the expected one, in at most max(1, n / 100) rows.  Raw scores: rtol 2e-7, atol 1e-6 (one fp32
rounding of a float64 sum).  The float64 expectation differs from the device by the fp32 rounding of the row factors and of the
final score only, so a swap needs a gap of about 1e-8."""
import concurrent.futures as cf
import pickle

import numpy as np
import pytest

from tests.helpers import assert_dense_topn as _check
from tests.test_dense8_gpu import _quantize
from tests.test_dense_rescore_gpu import _candidates, _restricted
from tests.test_hamming_cpu import hamming_topn, pack

pytestmark = pytest.mark.gpu


class _OtherShape:
    """a to-operand of one row more, as dense_topn_rescored reads it before the first device call"""
    def __init__(self, h):
        self.n, self.dim, self.dtype = h.n + 1, h.dim, h.dtype


def _unit(x):
    x = np.asarray(x, np.float64)
    n = np.sqrt((x * x).sum(axis=1, keepdims=True))
    return x / np.where(n > 0, n, 1.0)


def _signs(b):
    """the +-1 vectors of float rows (bit = x > 0) or of packed uint8 rows"""
    b = np.asarray(b)
    bits = np.unpackbits(b, axis=1) if b.dtype == np.uint8 else b > 0
    return np.where(bits, 1.0, -1.0)


def _dense8(a, q, normalize=True, scale=None):
    """float64 scores of float rows a against int8 rows q: the cosine, or the dot product with q (times the row scale)"""
    q = q.astype(np.float64)
    if normalize:
        return _unit(a) @ _unit(q).T
    return a.astype(np.float64) @ (q if scale is None else q * scale.astype(np.float64)[:, None]).T


def _dense1(a, s, normalize=True):
    """float64 scores of float rows a against the +-1 rows s"""
    return _unit(a) @ (s / np.sqrt(s.shape[1])).T if normalize else a.astype(np.float64) @ s.T


def _mixed(ctx, a, hb, cand, ntop, lower_bound, normalize=True):
    from polyfuzz_amd import _lib
    ha = _lib.DeviceDense.upload(ctx, a, normalize)
    table = _lib.DeviceTopN.from_host(ctx, cand, np.full(cand.shape, np.nan, np.float32))      # the val half is ignored
    return _lib.dense_rescore_mixed(ctx, ha, hb, table, ntop, lower_bound).download()


def _hold(ctx, a, upload, cand, ntop, dense, dots):
    """bounds 0 and 0.02, normalised (`dense`) and raw (`dots`), against the restricted float64 top-n"""
    n_from = len(a)
    for lb in (0.0, 0.02):
        idx, val = _mixed(ctx, a, upload(True), cand, ntop, lb)
        e_idx, e_val = _restricted(dense, cand, ntop, lb)
        print(a.shape, cand.shape, "bound", lb, "max |score - float64| =", float(np.abs(val - e_val).max()),
              "rows off the float64 order:", int((idx != e_idx).any(axis=1).sum()))
        _check(idx, val, e_idx, e_val, dense)
        assert ((idx < 0) == (val == 0)).all()
        idx, val = _mixed(ctx, a, upload(False), cand, ntop, lb, normalize=False)
        e_idx, e_val = _restricted(dots, cand, ntop, lb)
        np.testing.assert_allclose(val, e_val, rtol=2e-7, atol=1e-6)
        assert (idx == e_idx).all(axis=1).sum() >= n_from - max(1, n_from // 100)


KERNEL8 = [(1, 1, 1, 1, 1),
           (6, 3, 300, 3, 2),              # pitches: 320 floats against 384 int8
           (130, 257, 33, 64, 5),
           (70, 3000, 768, 1024, 128),     # the largest m
           (40, 1500, 4096, 20, 5),        # the longest from-row in LDS
           (5, 40, 4100, 8, 3)]            # one chunk beyond the LDS limit, pitches 4 128 against 4 224


@pytest.mark.parametrize("n_from,n_to,d,m,ntop", KERNEL8)
def test_kernel_alone_int8(ctx, n_from, n_to, d, m, ntop):
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(n_from + n_to + d + m)
    a = rng.standard_normal((n_from, d)).astype(np.float32)
    q = rng.integers(-127, 128, (n_to, d)).astype(np.int8)          # np.int8 is taken as it is: the test knows the stored values
    cand = _candidates(rng, n_from, n_to, m)
    if n_from >= 40:
        assert (cand < 0).all(axis=1).any() and ((cand[:, :-1] < 0) & (cand[:, 1:] >= 0)).any()
    _hold(ctx, a, lambda nrm: _lib.DeviceDense.upload_int8(ctx, q, nrm), cand, ntop, _dense8(a, q), _dense8(a, q, False))


def test_kernel_alone_int8_quantised_on_the_device(ctx):
    """float to-rows: the handle holds k5_quantize8's values and, raw, the row scales"""
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(8)
    a = rng.standard_normal((50, 300)).astype(np.float32)
    b = rng.standard_normal((400, 300)).astype(np.float32)
    q, scale = _quantize(b)
    cand = _candidates(rng, 50, 400, 32)
    _hold(ctx, a, lambda nrm: _lib.DeviceDense.upload_int8(ctx, b, nrm), cand, 5, _dense8(a, q), _dense8(a, q, False, scale))


KERNEL1 = [(3, 5, 1, 4, 2),
           (130, 257, 33, 64, 5),
           (20, 300, 96, 24, 5),           # a 12-byte row inside a 16-byte piece
           (40, 500, 300, 32, 5),
           (70, 3000, 768, 1024, 128),     # the largest m
           (10, 100, 1032, 16, 4),         # one byte past 128 B
           (5, 40, 4104, 8, 3)]            # past the LDS limit


@pytest.mark.parametrize("n_from,n_to,d,m,ntop", KERNEL1)
def test_kernel_alone_bits(ctx, n_from, n_to, d, m, ntop):
    """float to-rows packed on the device"""
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(n_from + n_to + d + m + 1)
    a = rng.standard_normal((n_from, d)).astype(np.float32)
    b = rng.standard_normal((n_to, d)).astype(np.float32)
    cand = _candidates(rng, n_from, n_to, m)
    s = _signs(b)
    _hold(ctx, a, lambda nrm: _lib.DeviceDense.upload_bits(ctx, b, nrm), cand, ntop, _dense1(a, s), _dense1(a, s, False))


def test_kernel_alone_bits_packed_on_the_host(ctx):
    """np.uint8 "ubinary" rows and np.int8 "binary" rows of the same bits: one result, that of the float rows packed on the device"""
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(77)
    a = rng.standard_normal((60, 768)).astype(np.float32)
    b = rng.standard_normal((900, 768)).astype(np.float32)
    u = pack(b)
    i8 = (u.astype(np.int16) - 128).astype(np.int8)
    cand = _candidates(rng, 60, 900, 40)
    s = _signs(u)
    assert u.dtype == np.uint8 and u.shape == (900, 96) and (s == _signs(b)).all()
    _hold(ctx, a, lambda nrm: _lib.DeviceDense.upload_bits(ctx, u, nrm), cand, 5, _dense1(a, s), _dense1(a, s, False))
    outs = [_mixed(ctx, a, _lib.DeviceDense.upload_bits(ctx, rows), cand, 5, 0.0) for rows in (u, i8, b)]
    for idx, val in outs[1:]:
        np.testing.assert_array_equal(idx, outs[0][0])
        np.testing.assert_array_equal(val.view(np.uint32), outs[0][1].view(np.uint32))


def _operands(ctx, rng, n_to, d):
    """(name, handle, float64 score function of float rows a) of an int8 and a bit to-side of n_to rows"""
    from polyfuzz_amd import _lib
    q = rng.integers(-127, 128, (n_to, d)).astype(np.int8)
    b = rng.standard_normal((n_to, d)).astype(np.float32)
    return q, b, [("int8", lambda rows: _lib.DeviceDense.upload_int8(ctx, q[rows]), lambda a, rows: _dense8(a, q[rows])),
                  ("binary", lambda rows: _lib.DeviceDense.upload_bits(ctx, b[rows]), lambda a, rows: _dense1(a, _signs(b[rows])))]


def test_the_order_of_the_candidates_does_not_matter(ctx):
    rng = np.random.default_rng(64)
    for d in (300, 4100):
        n_from, n_to, m = (130, 257, 64) if d == 300 else (9, 60, 24)
        a = rng.standard_normal((n_from, d)).astype(np.float32)
        cand = _candidates(rng, n_from, n_to, m)
        shuffled = np.stack([row[rng.permutation(m)] for row in cand])
        assert (shuffled != cand).any()
        for name, upload, _ in _operands(ctx, rng, n_to, d)[2]:
            hb = upload(slice(None))
            first = _mixed(ctx, a, hb, cand, 5, 0.0)
            second = _mixed(ctx, a, hb, shuffled, 5, 0.0)
            assert (first[0] >= 0).any(), name
            np.testing.assert_array_equal(first[0], second[0])
            np.testing.assert_array_equal(first[1].view(np.uint32), second[1].view(np.uint32))


def test_tie_rule_and_strict_bound(ctx):
    """five exact duplicates among the to-rows, all in every row's candidate list: one score, ascending columns.  A bound set ON
    a returned score drops it (strict >).  A zero from-row and a zero int8 to-row match nothing."""
    rng = np.random.default_rng(5)
    d, m, n_to = 96, 24, 600
    dups = np.array([7, 130, 131, 402, 599])
    rows = np.arange(n_to)
    rows[dups] = 7                                                        # to-row j is a copy of row 7 for j in dups
    q, b, operands = _operands(ctx, rng, n_to, d)
    for name, upload, score in operands:
        base = q[7].astype(np.float32) if name == "int8" else b[7]
        a = (base + 0.8 * np.abs(base).mean() * rng.standard_normal((20, d))).astype(np.float32)      # close to the duplicates
        a[19] = 0.0
        cand = np.full((20, m), -1, np.int32)
        others = np.setdiff1d(np.arange(n_to), dups)
        for i in range(20):
            row = np.concatenate([dups, rng.permutation(others)[:15]])
            cand[i, rng.permutation(m)[:20]] = rng.permutation(row)
        dense = score(a, rows)                                            # (columns of equal rows: equal float64 scores)
        hb = upload(rows)
        idx, val = _mixed(ctx, a, hb, cand, m, 0.0)
        e_idx, e_val = _restricted(dense, cand, m, 0.0)
        _check(idx, val, e_idx, e_val, dense)
        assert (idx[19] == -1).all() and (val[19] == 0).all(), name       # the zero from-row
        for i in range(19):
            at = int(np.nonzero(idx[i] == 7)[0][0])
            np.testing.assert_array_equal(idx[i, at:at + 5], dups)
            assert len(set(val[i, at:at + 5].view(np.uint32).tolist())) == 1
        at = int(np.nonzero(idx[0] == 7)[0][0])
        assert at + 5 < m and idx[0, at + 5] >= 0 and val[0, at + 4] > val[0, at + 5]
        on = float(val[0, at])
        b_idx, b_val = _mixed(ctx, a, hb, cand, m, on)
        keep = val > np.float32(on)                                       # of the first run's (sorted) rows: a prefix
        np.testing.assert_array_equal(b_idx, np.where(keep, idx, -1))
        np.testing.assert_array_equal(b_val.view(np.uint32), np.where(keep, val, np.float32(0)).view(np.uint32))
        assert not np.isin(b_idx[0], dups).any() and (b_idx[0] >= 0).sum() == at      # equal to the bound: dropped
    from polyfuzz_amd import _lib
    z = rng.integers(1, 128, (50, d)).astype(np.int8)                     # positive values on both sides: every pair scores > 0 ...
    z[3] = 0                                                              # ... but a zero int8 to-row: factor 0 normalised, sum 0 raw
    a = (np.abs(rng.standard_normal((4, d))) + 0.1).astype(np.float32)
    cand = np.tile(np.arange(50, dtype=np.int32), (4, 1))
    for nrm in (True, False):
        idx, _ = _mixed(ctx, a, _lib.DeviceDense.upload_int8(ctx, z, nrm), cand, 50, 0.0, normalize=nrm)
        assert (idx[:, :49] >= 0).all() and (idx[:, 49] == -1).all() and not (idx == 3).any()


@pytest.mark.parametrize("d", [33, 100])
def test_padding_contributes_nothing(ctx, d):
    """from-rows of all 1.0 (and of all -1.0, to see the other sign above the bound) against bit rows of all ones and of all
    zeros: the raw scores are exactly +d or -d -- a pad bit counted as -a[k], or a value read beyond a row's own pitch, would
    show.  The three pitches at d = 33: 64 floats, 128 bits; at d = 100: 128 floats, 128 bits."""
    from polyfuzz_amd import _lib
    a = np.stack([np.ones(d, np.float32), -np.ones(d, np.float32)])
    b = np.stack([np.ones(d, np.float32), -np.ones(d, np.float32)])      # packed on the device: all ones, all zeros
    cand = np.array([[1, 0], [0, 1]], np.int32)
    idx, val = _mixed(ctx, a, _lib.DeviceDense.upload_bits(ctx, b, False), cand, 2, 0.0, normalize=False)
    np.testing.assert_array_equal(idx, [[0, -1], [1, -1]])               # the pair of opposite signs scores -d: no match
    np.testing.assert_array_equal(val.view(np.uint32), np.array([[d, 0], [d, 0]], np.float32).view(np.uint32))
    idx, val = _mixed(ctx, a, _lib.DeviceDense.upload_bits(ctx, b, True), cand, 2, 0.0)
    np.testing.assert_array_equal(idx, [[0, -1], [1, -1]])
    np.testing.assert_allclose(val[:, 0], 1.0, rtol=0, atol=1e-6)
    # the same through int8 rows of all 1 / all -1: exactly +-d as well
    q = np.stack([np.ones(d, np.int8), -np.ones(d, np.int8)])
    idx, val = _mixed(ctx, a, _lib.DeviceDense.upload_int8(ctx, q, False), cand, 2, 0.0, normalize=False)
    np.testing.assert_array_equal(idx, [[0, -1], [1, -1]])
    np.testing.assert_array_equal(val.view(np.uint32), np.array([[d, 0], [d, 0]], np.float32).view(np.uint32))


def _gaussian():
    rng = np.random.default_rng(768)
    return rng.standard_normal((300, 768)).astype(np.float32), rng.standard_normal((2000, 768)).astype(np.float32)


def _clustered():
    """2 000 to-vectors in 400 clusters of 5, 300 queries near a cluster centre each: the median 5th-best cosine is 0.59, the 6th 0.12"""
    rng = np.random.default_rng(22)
    c = rng.standard_normal((400, 768))
    b = (np.repeat(c, 5, axis=0) + 0.8 * rng.standard_normal((2000, 768))).astype(np.float32)
    a = (c[rng.integers(0, 400, 300)] + 0.8 * rng.standard_normal((300, 768))).astype(np.float32)
    return a, b


@pytest.mark.parametrize("data", ["gaussian", "clustered"])
def test_two_stage_search_end_to_end(ctx, data):
    """dense_rescored_topn_host(..., rescore_to=...) for the three pairs at 300 x 2 000 x 768, top-5: the result is the restricted
    float64 top-5 of the coarse stage's candidates -- for bits the numpy Hamming top-m by the tie rule (the stage is exact), for
    int8 the device's own dense_topn with m columns and bound 0.  Printed, as measurements: the rows whose result equals the
    plain float64 top-5 of the ORIGINAL vectors, beside the float32 rescoring's."""
    from polyfuzz_amd import _lib
    a, b = _gaussian() if data == "gaussian" else _clustered()
    q, _ = _quantize(b)
    exact = _unit(a) @ _unit(b).T
    full, _ = _restricted(exact, np.tile(np.arange(2000, dtype=np.int32), (300, 1)), 5, 0.0)
    to_side = {"int8": _dense8(a, q), "binary": _dense1(a, _signs(b))}
    pa, pb = pack(a), pack(b)
    q_a, q_b = _lib.DeviceDense.upload_int8(ctx, a), _lib.DeviceDense.upload_int8(ctx, b)
    for coarse, rescore_to, mult in (("int8", "int8", 4), ("binary", "binary", 16), ("binary", "int8", 16)):
        m = 5 * mult
        if coarse == "binary":
            c_idx, _ = hamming_topn(pa, pb, 768, m)
        else:
            c_idx, _ = _lib.dense_topn(ctx, q_a, q_b, m, 0.0).download()
        idx, val = _lib.dense_rescored_topn_host(ctx, a, b, 5, 0.0, coarse=coarse, multiplier=mult, rescore_to=rescore_to)
        dense = to_side[rescore_to]
        e_idx, e_val = _restricted(dense, c_idx, 5, 0.0)
        print(f"{data} {coarse} x{mult} -> {rescore_to}: max |score - float64| = {float(np.abs(val - e_val).max()):.2e}, "
              f"worst |score - float32 cosine| = {float(np.abs(dense - exact).max()):.2e}")
        _check(idx, val, e_idx, e_val, dense)
        if rescore_to == coarse:                                          # a to-side given in that form is the same search
            given = q if coarse == "int8" else pb
            g_idx, g_val = _lib.dense_rescored_topn_host(ctx, a, given, 5, 0.0, coarse=coarse, multiplier=mult, rescore_to=rescore_to)
            np.testing.assert_array_equal(g_idx, idx)
            np.testing.assert_array_equal(g_val.view(np.uint32), val.view(np.uint32))
    # measurements, not conditions
    for coarse, forms in (("int8", ("int8", None)), ("binary", ("binary", "int8", None))):
        for mult in (4, 16, 64):
            rows = []
            for form in forms:
                idx, _ = _lib.dense_rescored_topn_host(ctx, a, b, 5, 0.0, coarse=coarse, multiplier=mult, rescore_to=form)
                rows.append(f"{form or 'float32'} to-side {int((idx == full).all(axis=1).sum())}")
            print(f"{data}: {coarse} search x{mult}, rows of 300 equal to the float64 top-5: " + ", ".join(rows))


def test_no_float32_to_side_is_created(ctx):
    from polyfuzz_amd import _lib, pipeline
    from polyfuzz_amd.models import Embeddings
    rng = np.random.default_rng(4000)
    a = rng.standard_normal((50, 768)).astype(np.float32)
    b = rng.standard_normal((4000, 768)).astype(np.float32)
    fp32_to_side = b.nbytes
    ctx.sync()
    before = ctx.pool_stats()[0]
    h_bits, h_int8 = _lib.DeviceDense.upload_bits(ctx, b), _lib.DeviceDense.upload_int8(ctx, b)
    job = pipeline.DenseMatchJob(ctx, _lib.DeviceDense.upload_bits(ctx, a), h_bits, top_n=5, rescore_multiplier=16, rescore_from=a,
                                 rescore_to=h_int8)
    assert job.to_exact is h_int8 and job.from_exact.dtype == "float32"
    idx, val = job.step().download()
    ctx.sync()
    live = ctx.pool_stats()[0] - before
    print("binary + int8 to-side, 4000 x 768: live bytes", live, "a float32 to-side alone:", fp32_to_side)
    assert 0 < live < fp32_to_side
    ref = _lib.dense_rescored_topn_host(ctx, a, b, 5, 0.0, coarse="binary", multiplier=16, rescore_to="int8")
    np.testing.assert_array_equal(idx, ref[0])
    np.testing.assert_array_equal(val.view(np.uint32), ref[1].view(np.uint32))
    del job, h_bits, h_int8
    fl, tl = [f"f{i}" for i in range(50)], [f"t{i}" for i in range(4000)]
    for to, binary, precision, rescore_to in ((pack(b), "ubinary", None, "ubinary"), (b, "binary", None, "int8"), (b, None, "int8", "int8")):
        before = ctx.pool_stats()[0]
        m = Embeddings(min_similarity=0.0, top_n=5, cosine_method="hip")
        m.binary, m.precision, m.rescore_multiplier, m.rescore_to = binary, precision, 4, rescore_to
        df = m.match(fl, tl, embeddings_from=a, embeddings_to=to)
        ctx.sync()
        live = ctx.pool_stats()[0] - before
        print(f"Embeddings binary={binary} precision={precision} rescore_to={rescore_to}: live bytes", live)
        assert len(df) == 50 and 0 < live < fp32_to_side
        assert m._dev_to_exact.dtype != "float32" and (m._dev_to_exact is m._dev_to) == (rescore_to != "int8" or precision == "int8")
        del m


def _same_frame(df, expect):
    assert list(df.columns) == list(expect.columns)
    for col in df.columns:
        assert df[col].tolist() == expect[col].tolist(), col


def test_embeddings_with_rescore_to(ctx):
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import Embeddings
    from polyfuzz_amd.models._utils import topn_to_frame
    rng = np.random.default_rng(21)
    a = rng.standard_normal((301, 96)).astype(np.float32)
    b = rng.standard_normal((530, 96)).astype(np.float32)
    u = pack(b)
    fl, tl = [f"f{i}" for i in range(len(a))], [f"t{i}" for i in range(len(b))]
    # a corpus that exists only as packed bits
    m = Embeddings(min_similarity=0.0, top_n=4, cosine_method="hip")
    m.binary, m.rescore_multiplier = "ubinary", 4
    with pytest.raises(ValueError, match="no full-precision vectors"):       # today's refusal, while rescore_to is None
        m.match(fl, tl, embeddings_from=a, embeddings_to=u)
    m.rescore_to = "ubinary"
    df = m.match(fl, tl, embeddings_from=a, embeddings_to=u)
    ref = _lib.dense_rescored_topn_host(ctx, a, u, 4, 0.0, coarse="binary", multiplier=4, rescore_to="binary")
    _same_frame(df, topn_to_frame(ref[0], ref[1], fl, tl, 4))
    assert len(df.columns) == 9 and m._dev_to_exact is m._dev_to and m._dev_to.dtype == "binary"
    resident = m._dev_to
    df2 = m.match(fl[:50], tl, embeddings_from=a[:50], re_train=False)      # the to-side stays resident
    assert m._dev_to is resident and m._dev_to_exact is resident
    assert df2.equals(df.iloc[:50].reset_index(drop=True))
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.rescore_to == "ubinary" and m2.binary == "ubinary" and m2._dev_to is None and m2._dev_to_exact is None
    assert m2.match(fl[:50], tl, embeddings_from=a[:50], re_train=False).equals(df2)
    with pytest.raises(ValueError, match="embeddings_from.*no full-precision vectors"):
        m.match(fl, tl, embeddings_from=pack(a), embeddings_to=u)
    # binary search, int8 rescoring, on float to-vectors: the int8 form comes beside the bits and follows rescore_to
    m.rescore_to = "int8"
    df8 = m.match(fl, tl, embeddings_from=a, embeddings_to=b)
    ref = _lib.dense_rescored_topn_host(ctx, a, b, 4, 0.0, coarse="binary", multiplier=4, rescore_to="int8")
    _same_frame(df8, topn_to_frame(ref[0], ref[1], fl, tl, 4))
    coarse, fine = m._dev_to, m._dev_to_exact
    assert coarse.dtype == "binary" and fine.dtype == "int8"
    m.match(fl[:50], tl, embeddings_from=a[:50], re_train=False)
    assert m._dev_to is coarse and m._dev_to_exact is fine
    m.rescore_to = "binary"                                                    # re-made when rescore_to changes; the bits stay
    m.match(fl[:50], tl, embeddings_from=a[:50], re_train=False)
    assert m._dev_to is coarse and m._dev_to_exact is coarse
    with pytest.raises(ValueError, match="same form"):
        m.rescore_to = "int8"
        m.match(fl, tl, embeddings_from=a, embeddings_to=u)
    # rescore_to = None afterwards: today's frame and today's refusals
    m.rescore_to = None
    today = m.match(fl, tl, embeddings_from=a, embeddings_to=b)
    assert m._dev_to_exact.dtype == "float32"
    ref = _lib.dense_rescored_topn_host(ctx, a, b, 4, 0.0, coarse="binary", multiplier=4)
    _same_frame(today, topn_to_frame(ref[0], ref[1], fl, tl, 4))
    with pytest.raises(ValueError, match="no full-precision vectors"):
        m.match(fl, tl, embeddings_from=a, embeddings_to=u)
    # an np.int8 to-side
    q = np.clip(np.rint(b * 40), -127, 127).astype(np.int8)
    m8 = Embeddings(min_similarity=0.0, top_n=4, cosine_method="hip")
    m8.precision, m8.rescore_multiplier, m8.rescore_to = "int8", 4, "int8"
    dfq = m8.match(fl, tl, embeddings_from=a, embeddings_to=q)
    ref = _lib.dense_rescored_topn_host(ctx, a, q, 4, 0.0, coarse="int8", multiplier=4, rescore_to="int8")
    _same_frame(dfq, topn_to_frame(ref[0], ref[1], fl, tl, 4))
    assert m8._dev_to_exact is m8._dev_to and m8._dev_to.dtype == "int8"
    # self-match through an embedding_method
    e = Embeddings(embedding_method=lambda strings: a[[int(s[1:]) for s in strings]], min_similarity=0.0, top_n=4, cosine_method="hip")
    e.binary, e.rescore_multiplier, e.rescore_to = "binary", 8, "int8"
    own = e.match(fl[:50])
    assert (own["To"] != own["From"]).all() and own["To"].notna().all() and e._dev_to_exact.dtype == "int8"


def test_sharded_dense_job_against_the_to_handle(ctx):
    """DenseMatchJob on two contexts of one device with uneven shards, as
    tests/test_dense_rescore_gpu.py::test_sharded_dense_job_with_rescoring, with rescore_to = the to handle itself: the one-shot
    call bit for bit, self-match included; the candidate table is allocated once."""
    import polyfuzz_amd
    from polyfuzz_amd import _lib, pipeline
    rng = np.random.default_rng(21)
    a = rng.standard_normal((301, 96)).astype(np.float32)
    b = rng.standard_normal((530, 96)).astype(np.float32)
    ctxs = [polyfuzz_amd.Context(0), polyfuzz_amd.Context(0)]
    comms = _lib.Comm.local_group(ctxs)
    bounds = [pipeline.shard_bounds(len(a), 2, r) for r in range(2)]
    sizes = [e - s for s, e in bounds]

    def rank_fn(r, self_match, coarse):
        s, e = bounds[r]
        up = _lib.DeviceDense.upload_int8 if coarse == "int8" else _lib.DeviceDense.upload_bits
        to = up(ctxs[r], a if self_match else b)
        job = pipeline.DenseMatchJob(ctxs[r], up(ctxs[r], a[s:e]), to, top_n=4, comm=comms[r], rows_per_rank=max(sizes),
                                     self_match=self_match, shard_offset=s if self_match else 0, rescore_multiplier=4,
                                     rescore_from=a[s:e] if r else _lib.DeviceDense.upload(ctxs[r], a[s:e]), rescore_to=to)
        assert job.to_exact is to and job.from_exact.dtype == "float32" and job.candidates.ntop == 16
        table = job.candidates
        job.step()
        idx, val = job.step().download()
        assert job.candidates is table                                # allocated once, at construction
        return pipeline.TfidfMatchJob.unpad(idx, val, sizes, max(sizes))

    for coarse in ("int8", "binary"):
        for self_match in (False, True):
            exp = _lib.dense_rescored_topn_host(ctx, a, a if self_match else b, 4, 0.0, coarse=coarse, multiplier=4,
                                                exclude_diag=self_match, rescore_to=coarse)
            with cf.ThreadPoolExecutor(2) as ex:
                outs = [f.result(timeout=120) for f in [ex.submit(rank_fn, r, self_match, coarse) for r in range(2)]]
            for idx, val in outs:
                np.testing.assert_array_equal(idx, exp[0])
                np.testing.assert_array_equal(val, exp[1])
    for c in comms:
        c.free()


def test_refusals_of_the_new_entry(ctx):
    from polyfuzz_amd import _lib, pipeline
    rng = np.random.default_rng(50)
    a = rng.standard_normal((20, 64)).astype(np.float32)
    b = rng.standard_normal((50, 64)).astype(np.float32)
    x_a, x_b = _lib.DeviceDense.upload(ctx, a), _lib.DeviceDense.upload(ctx, b)
    q_a, q_b = _lib.DeviceDense.upload_int8(ctx, a), _lib.DeviceDense.upload_int8(ctx, b)
    b_b, b_raw = _lib.DeviceDense.upload_bits(ctx, b), _lib.DeviceDense.upload_bits(ctx, b, normalize=False)
    h16 = _lib.DeviceDense.upload(ctx, b, True, "float16")
    table = _lib.dense_topn(ctx, q_a, q_b, 8, 0.0)
    for bad in (q_a, _lib.DeviceDense.upload_bits(ctx, a), _lib.DeviceDense.upload(ctx, a, True, "bfloat16")):
        with pytest.raises(_lib.PfzError, match="from-vectors must be float32"):
            _lib.dense_rescore_mixed(ctx, bad, q_b, table, 3, 0.0)
    for bad in (x_b, h16):
        with pytest.raises(_lib.PfzError, match=r"int8 or binary.*pfz_dense_rescore_topn is the entry for float32"):
            _lib.dense_rescore_mixed(ctx, x_a, bad, table, 3, 0.0)
    with pytest.raises(_lib.PfzError, match="64 columns.*63"):
        _lib.dense_rescore_mixed(ctx, x_a, _lib.DeviceDense.upload_int8(ctx, b[:, :63].copy()), table, 3, 0.0)
    with pytest.raises(_lib.PfzError, match="64 columns.*56 bits.*8 bits per byte"):
        _lib.dense_rescore_mixed(ctx, x_a, _lib.DeviceDense.upload_bits(ctx, pack(b)[:, :7].copy()), table, 3, 0.0)
    with pytest.raises(_lib.PfzError, match="without normalize.*one or the other"):
        _lib.dense_rescore_mixed(ctx, x_a, b_raw, table, 3, 0.0)
    with pytest.raises(_lib.PfzError, match="one buffer"):
        _lib.dense_rescore_mixed(ctx, x_a, q_b, table, 8, 0.0, out=table)
    with pytest.raises(_lib.PfzError, match="candidate table has 20 rows.*50"):
        _lib.dense_rescore_mixed(ctx, x_b, q_b, table, 3, 0.0)
    for ntop in (0, 9):
        with pytest.raises(_lib.PfzError, match=f"ntop {ntop}"):
            _lib.dense_rescore_mixed(ctx, x_a, q_b, table, ntop, 0.0, out=_lib.DeviceTopN.alloc(ctx, 20, max(ntop, 1)))
    with pytest.raises(_lib.PfzError, match="NaN"):
        _lib.dense_rescore_mixed(ctx, x_a, b_b, table, 3, float("nan"))
    with pytest.raises(_lib.PfzError, match="result buffer"):
        _lib.dense_rescore_mixed(ctx, x_a, q_b, table, 3, 0.0, out=_lib.DeviceTopN.alloc(ctx, 20, 4))
    wide = _lib.DeviceTopN.alloc(ctx, 20, 1025)
    wide.clear()
    with pytest.raises(_lib.PfzUnsupported, match="1024"):
        _lib.dense_rescore_mixed(ctx, x_a, q_b, wide, 5, 0.0)
    empty = _lib.dense_rescore_mixed(ctx, _lib.DeviceDense.upload(ctx, a[:0]), q_b, table, 3, 0.0)       # no from-rows: nothing to do
    assert empty.download()[0].shape == (0, 3)
    # the float32 entry keeps refusing what it refused
    with pytest.raises(_lib.PfzError, match="float32"):
        _lib.dense_rescore(ctx, x_a, q_b, table, 3, 0.0)
    # refusals raised in Python: nothing is allocated or enqueued
    ctx.sync()
    live = ctx.pool_stats()[0]
    with pytest.raises(ValueError, match=r"rescore_to.*cannot follow"):
        _lib.dense_rescored_topn_host(ctx, a, b, 3, 0.0, coarse="int8", multiplier=4, rescore_to="binary")
    with pytest.raises(ValueError, match=r"rescore_to.*cannot follow"):
        _lib.dense_rescored_topn_host(ctx, a, b, 3, 0.0, coarse="float16", multiplier=4, rescore_to="int8")
    with pytest.raises(ValueError, match="rescore_to must be"):
        _lib.dense_rescored_topn_host(ctx, a, b, 3, 0.0, coarse="int8", multiplier=4, rescore_to="float32")
    with pytest.raises(ValueError, match="needs coarse='int8'"):
        _lib.dense_rescored_topn_host(ctx, a, b.astype(np.int8), 3, 0.0, coarse="binary", multiplier=4, rescore_to="int8")
    with pytest.raises(ValueError, match="not the same vectors"):
        _lib.dense_topn_rescored(ctx, q_a, q_b, x_a, _OtherShape(q_b), 3, 0.0, 4)
    with pytest.raises(ValueError, match="float32 form"):
        pipeline.DenseMatchJob(ctx, q_a, q_b, top_n=4, rescore_multiplier=4, rescore_from=q_a, rescore_to=q_b)
    with pytest.raises(ValueError, match="float32 form"):
        pipeline.DenseMatchJob(ctx, q_a, q_b, top_n=4, rescore_multiplier=4, rescore_from=x_a, rescore_to=b_b)      # bits after int8
    with pytest.raises(ValueError, match="float32 form"):
        pipeline.DenseMatchJob(ctx, q_a, q_b, top_n=4, rescore_multiplier=4, rescore_from=x_a, rescore_to=q_a)      # another shape
    assert ctx.pool_stats()[0] == live
    # the handles are still good
    idx, val = _lib.dense_topn_rescored(ctx, q_a, q_b, x_a, q_b, 3, 0.0, 4).download()
    ref = _lib.dense_rescored_topn_host(ctx, a, b, 3, 0.0, coarse="int8", multiplier=4, rescore_to="int8")
    np.testing.assert_array_equal(idx, ref[0])
    np.testing.assert_array_equal(val, ref[1])
    idx, _ = _lib.dense_rescore_mixed(ctx, x_a, b_b, table, 8, 0.0).download()
    assert (idx[:, 0] >= 0).all()

