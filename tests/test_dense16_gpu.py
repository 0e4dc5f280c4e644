"""GPU parity of K5's 16-bit path (k5_gemm16_panel: float16 / bfloat16 vectors on the 16-bit matrix cores, fp32
accumulation) against the float64 oracle ON THE 16-BIT VECTORS: the inputs are rounded in numpy, widened back to float64
and handed to oracle.dense_cossim_topn / dense_cossim.  The acceptance rule is the fp32 path's (tests/test_dense_gpu.py)."""
import concurrent.futures as cf
import pickle

import numpy as np
import pytest

from tests.helpers import assert_dense_topn as _check

pytestmark = pytest.mark.gpu

DTYPES = ("float16", "bfloat16")


def _bf16_bits(a):
    """float32 -> bfloat16 bits, round to nearest even"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _rounded(a, dtype):
    """(the array to hand to the library: np.float16 values or raw bfloat16 bits, the same values as float64)"""
    if dtype == "float16":
        g = np.asarray(a, np.float32).astype(np.float16)
        return g, g.astype(np.float64)
    g = _bf16_bits(a)
    return g, (g.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


PARITY = [(1, 1, 1, 1),            # width far below one k-chunk; one tile, mostly clamped rows
          (6, 3, 300, 2),          # the reference's fixture shape; d not a multiple of the chunk
          (300, 1000, 33, 10),     # d just over a fragment; padding columns must be zeros in both operands
          (513, 129, 64, 128),     # exactly one k-chunk: no steady-state loop; edge tiles on both sides
          (130, 257, 768, 5),      # 12 chunks: the pipelined steady state; one row / column beyond a tile
          (130, 257, 4096, 5),     # longest accumulation chain
          (200, 1500, 128, 5)]     # more than one 8 x 8 tile block on the to-side (the XCD mapping)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_a,n_b,d,ntop", PARITY)
def test_random_dense16_vs_oracle(ctx, oracle_mod, dtype, n_a, n_b, d, ntop):
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(n_a + n_b + d)
    a = rng.standard_normal((n_a, d)).astype(np.float32)
    b = rng.standard_normal((n_b, d)).astype(np.float32)
    if n_b > 10:
        b[3] = 2 * a[0]              # an exact-direction duplicate (doubling is exact in both types): cosine 1
        b[7] = 0                     # zero row: cosine 0 with everything
    ga, wa = _rounded(a, dtype)
    gb, wb = _rounded(b, dtype)
    idx, val = _lib.dense_cossim_topn_host(ctx, ga, gb, ntop, 0.0, compute_dtype=dtype)
    e_idx, e_val = oracle_mod.dense_cossim_topn(wa, wb, ntop, 0.0)
    print(dtype, (n_a, n_b, d, ntop), "max |score - oracle| =", float(np.abs(val - e_val).max()))
    _check(idx, val, e_idx, e_val, oracle_mod.dense_cossim(wa, wb))
    if n_b > 10:
        assert idx[0, 0] == 3 and abs(val[0, 0] - 1.0) < 1e-5


@pytest.mark.parametrize("dtype", DTYPES)
def test_given_16bit_input_equals_rounding_on_the_device(ctx, dtype):
    """A np.float16 array (raw bfloat16 bits as np.uint16) gives, bit for bit, what the same values passed as float32
    give with compute_dtype: k5_round16 rounds to nearest even, as numpy does; widths with and without padding."""
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(16)
    for n_a, n_b, d in ((130, 257, 768), (77, 300, 33)):
        a = rng.standard_normal((n_a, d)).astype(np.float32)
        b = rng.standard_normal((n_b, d)).astype(np.float32)
        a[0, :8] = [1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0 - 2.0 ** -11, 3e-6, -4e-5,
                    1.0 + 2.0 ** -9]                                    # exact halves (ties to even both ways), f16 subnormals
        given = _lib.dense_cossim_topn_host(ctx, _rounded(a, dtype)[0], _rounded(b, dtype)[0], 5, 0.0, compute_dtype=dtype)
        dev = _lib.dense_cossim_topn_host(ctx, a, b, 5, 0.0, compute_dtype=dtype)
        np.testing.assert_array_equal(given[0], dev[0])
        np.testing.assert_array_equal(given[1], dev[1])
        h = _lib.DeviceDense.upload(ctx, a, True, dtype)
        assert h.dtype == dtype and (h.n, h.dim) == (n_a, d)
        assert _lib.DeviceDense.upload(ctx, a.astype(np.float16)).dtype == "float32"     # no keyword: fp32, also for float16


def test_subnormal_float16_inputs(ctx, oracle_mod):
    """2 % of the entries below float16's smallest normal (6.1e-5): the scores stay within the rule against the oracle on
    the inputs as given."""
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(61)
    a = rng.standard_normal((100, 96)).astype(np.float32)
    b = rng.standard_normal((300, 96)).astype(np.float32)
    for m in (a, b):
        sel = rng.random(m.shape) < 0.02
        m[sel] = (rng.uniform(1e-7, 6e-5, m.shape) * rng.choice([-1.0, 1.0], m.shape)).astype(np.float32)[sel]
    ga, wa = _rounded(a, "float16")
    gb, wb = _rounded(b, "float16")
    assert ((np.abs(wa) < 6e-5) & (wa != 0)).sum() > 100
    idx, val = _lib.dense_cossim_topn_host(ctx, ga, gb, 5, 0.0, compute_dtype="float16")
    e_idx, e_val = oracle_mod.dense_cossim_topn(wa, wb, 5, 0.0)
    print("subnormals: max |score - oracle| =", float(np.abs(val - e_val).max()))
    _check(idx, val, e_idx, e_val, oracle_mod.dense_cossim(wa, wb))


@pytest.mark.parametrize("dtype", DTYPES)
def test_self_match_and_lower_bound(ctx, oracle_mod, dtype):
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(9)
    a = rng.standard_normal((400, 96)).astype(np.float32)
    a[100:110] = a[:10] + 0.05 * rng.standard_normal((10, 96)).astype(np.float32)      # near-duplicates
    g, w = _rounded(a, dtype)
    idx, val = _lib.dense_cossim_topn_host(ctx, g, g, 3, 0.2, exclude_diag=True, compute_dtype=dtype)
    e_idx, e_val = oracle_mod.dense_cossim_topn(w, w, 3, 0.2, exclude_diag=True)
    _check(idx, val, e_idx, e_val, oracle_mod.dense_cossim(w, w))
    assert (idx != np.arange(400)[:, None]).all()                                       # row i never comes back for row i
    assert (idx[:10, 0] == np.arange(100, 110)).all() and (idx[100:110, 0] == np.arange(10)).all()
    a[200:203] = a[50]                                                                  # exact duplicates: lowest index first
    g, w = _rounded(a, dtype)
    idx, _ = _lib.dense_cossim_topn_host(ctx, g, g, 3, 0.2, exclude_diag=True, compute_dtype=dtype)
    np.testing.assert_array_equal(idx[50], [200, 201, 202])
    np.testing.assert_array_equal(idx[201], [50, 200, 202])


@pytest.mark.parametrize("dtype", DTYPES)
def test_raw_dot_products_of_unnormalised_vectors(ctx, oracle_mod, dtype):
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(21)
    a = (rng.standard_normal((150, 70)) * rng.uniform(0.2, 3.0, (150, 1))).astype(np.float32)
    b = (rng.standard_normal((900, 70)) * rng.uniform(0.2, 3.0, (900, 1))).astype(np.float32)
    ga, wa = _rounded(a, dtype)
    gb, wb = _rounded(b, dtype)
    idx, val = _lib.dense_cossim_topn_host(ctx, ga, gb, 6, 0.5, normalize=False, compute_dtype=dtype)
    e_idx, e_val = oracle_mod.dense_cossim_topn(wa, wb, 6, 0.5, normalize=False)
    dots = oracle_mod.dense_cossim(wa, wb, normalize=False)
    np.testing.assert_allclose(val, e_val, rtol=2e-6, atol=2e-5)
    bad = np.nonzero((idx != e_idx).any(axis=1))[0]
    for i in bad:                                    # only fp32-level near-ties may swap
        for r in range(idx.shape[1]):
            if idx[i, r] != e_idx[i, r]:
                s_got = dots[i, idx[i, r]] if idx[i, r] >= 0 else 0.0
                assert abs(s_got - e_val[i, r]) < 1e-4 * max(1.0, abs(e_val[i, r]))
    assert len(bad) <= 3
    c_idx, _ = _lib.dense_cossim_topn_host(ctx, ga, gb, 6, 0.0, compute_dtype=dtype)
    assert (c_idx[:, 0] != idx[:, 0]).any()           # cosine and dot product rank differently here


@pytest.mark.parametrize("dtype", DTYPES)
def test_block_maxima_and_panels(ctx, oracle_mod, monkeypatch, dtype):
    """The 1500 x 64 case of the fp32 test: duplicates in four different 64-column blocks, three (bound, self) settings.
    PFZ_K5_NO_BLOCK_MAX, PFZ_K5_PANEL_ROWS=256 and neither: equal bit for bit, and the oracle's result."""
    from polyfuzz_amd import _lib
    ntop = 10
    rng = np.random.default_rng(77 + ntop)
    d = 64
    b = rng.standard_normal((1500, d)).astype(np.float32)
    for j in (70, 700, 1400, 1499):
        b[j] = b[5]
    a = rng.standard_normal((333, d)).astype(np.float32)
    a[:40] = b[5] + 0.3 * rng.standard_normal((40, d)).astype(np.float32)
    ga, wa = _rounded(a, dtype)
    gb, wb = _rounded(b, dtype)
    for lb, self_match in ((0.0, False), (0.35, False), (0.0, True)):
        (x, wx), (y, wy) = ((gb, wb), (gb, wb)) if self_match else ((ga, wa), (gb, wb))
        monkeypatch.setenv("PFZ_K5_NO_BLOCK_MAX", "1")
        full = _lib.dense_cossim_topn_host(ctx, x, y, ntop, lb, exclude_diag=self_match, compute_dtype=dtype)
        monkeypatch.delenv("PFZ_K5_NO_BLOCK_MAX")
        fast = _lib.dense_cossim_topn_host(ctx, x, y, ntop, lb, exclude_diag=self_match, compute_dtype=dtype)
        np.testing.assert_array_equal(fast[0], full[0])
        np.testing.assert_array_equal(fast[1], full[1])
        monkeypatch.setenv("PFZ_K5_PANEL_ROWS", "256")
        paneled = _lib.dense_cossim_topn_host(ctx, x, y, ntop, lb, exclude_diag=self_match, compute_dtype=dtype)
        monkeypatch.delenv("PFZ_K5_PANEL_ROWS")
        np.testing.assert_array_equal(paneled[0], full[0])
        np.testing.assert_array_equal(paneled[1], full[1])
        e_idx, e_val = oracle_mod.dense_cossim_topn(wx, wy, ntop, lb, exclude_diag=self_match)
        _check(fast[0], fast[1], e_idx, e_val, oracle_mod.dense_cossim(wx, wy))
        if self_match:
            assert (fast[0] != np.arange(len(x))[:, None]).all()
            assert fast[0][5, 0] == 70 and fast[0][70, 0] == 5          # duplicates find each other, lowest index first


@pytest.mark.parametrize("dtype", DTYPES)
def test_deep_top_n(ctx, oracle_mod, monkeypatch, dtype):
    """70 x 3000 x 24, top 2500 in passes of 1024 over 128-row panels.  Scores within 1e-5; an index differs only where the
    oracle's score of the chosen column is within 4e-6 of the expected one; no column twice.  The rule's third part is a
    count of ROWS made for results of a few columns; a row here holds about 1500 positive scores 4e-4 apart on average, and
    the fp32 rounding of the final score alone (3e-8) swaps two float64 neighbours in about one row of five whatever computes
    them, so the same 1 / 100 is held per result ENTRY (as tests/test_dense_gpu.py::test_deep_top_n_in_passes holds the
    first two parts only)."""
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(70 + 2500)
    a = rng.standard_normal((70, 24)).astype(np.float32)
    b = rng.standard_normal((3000, 24)).astype(np.float32)
    b[100:140] = b[50]                             # forty exact duplicates: one score, forty columns in ascending order
    ga, wa = _rounded(a, dtype)
    gb, wb = _rounded(b, dtype)
    monkeypatch.setenv("PFZ_K5_PANEL_ROWS", "128")
    idx, val = _lib.dense_cossim_topn_host(ctx, ga, gb, 2500, 0.0, compute_dtype=dtype)
    e_idx, e_val = oracle_mod.dense_cossim_topn(wa, wb, 2500, 0.0, chunk_rows=64)
    dense = oracle_mod.dense_cossim(wa, wb)
    np.testing.assert_allclose(val, e_val, rtol=0, atol=1e-5)
    assert ((idx < 0) == (e_idx < 0)).all() and (idx < 0).any()
    rr, cc = np.nonzero(idx != e_idx)
    print(dtype, "deep top-n: entries off the oracle's order:", len(rr), "of", idx.size)
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
    h16 = _lib.DeviceDense.upload(ctx, a, True, "float16")
    h32 = _lib.DeviceDense.upload(ctx, a, True)
    hbf = _lib.DeviceDense.upload(ctx, a, True, "bfloat16")
    with pytest.raises(_lib.PfzError, match="float16.*float32"):
        _lib.dense_topn(ctx, h16, h32, 2, 0.0)
    with pytest.raises(_lib.PfzError, match="float16.*bfloat16"):
        _lib.dense_topn(ctx, h16, hbf, 2, 0.0)
    with pytest.raises(_lib.PfzError, match="float32.*float16"):
        _lib.dense_topn(ctx, h32, h16, 2, 0.0)
    with pytest.raises(ValueError, match="compute_dtype"):
        _lib.DeviceDense.upload(ctx, a, True, "int8")
    with pytest.raises(ValueError, match="float array"):
        _lib.DeviceDense.upload(ctx, np.arange(12, dtype=np.int32).reshape(3, 4), True, "float16")
    idx, val = _lib.dense_topn(ctx, h16, h16, 1, 0.0).download()              # the handles are still good
    np.testing.assert_array_equal(idx[:, 0], np.arange(10))


def test_embeddings_with_compute_dtype(ctx):
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import Embeddings
    rng = np.random.default_rng(21)
    a = rng.standard_normal((301, 96)).astype(np.float32)
    b = rng.standard_normal((530, 96)).astype(np.float32)
    fl, tl = [f"f{i}" for i in range(len(a))], [f"t{i}" for i in range(len(b))]
    ref_idx, ref_val = _lib.dense_cossim_topn_host(ctx, a, b, 4, 0.0, compute_dtype="float16")
    m = Embeddings(min_similarity=0.0, top_n=4, cosine_method="hip")
    m.compute_dtype = "float16"
    df = m.match(fl, tl, embeddings_from=a, embeddings_to=b)
    assert df["To"].tolist() == [tl[j] for j in ref_idx[:, 0]]
    assert df["To_3"].tolist() == [tl[j] for j in ref_idx[:, 2]]
    resident = m._dev_to
    assert resident.dtype == "float16"
    df2 = m.match(fl[:50], tl, embeddings_from=a[:50], re_train=False)            # to-side: resident, not re-uploaded
    assert m._dev_to is resident
    assert df2["To_3"].tolist() == [tl[j] for j in ref_idx[:50, 2]]
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.compute_dtype == "float16"
    assert m2.match(fl[:50], tl, embeddings_from=a[:50], re_train=False).equals(df2)
    m.compute_dtype = "bfloat16"                                                  # the resident to-side follows the type
    bf_idx, _ = _lib.dense_cossim_topn_host(ctx, a[:50], b, 4, 0.0, compute_dtype="bfloat16")
    df3 = m.match(fl[:50], tl, embeddings_from=a[:50], re_train=False)
    assert m._dev_to is not resident and m._dev_to.dtype == "bfloat16"
    assert df3["To"].tolist() == [tl[j] for j in bf_idx[:, 0]]


def test_sharded_dense_job_float16(ctx):
    """DenseMatchJob on two contexts of one device with uneven shards == the one-shot call, bit for bit."""
    import polyfuzz_amd
    from polyfuzz_amd import _lib, pipeline
    rng = np.random.default_rng(21)
    a = rng.standard_normal((301, 96)).astype(np.float32)
    b = rng.standard_normal((530, 96)).astype(np.float32)
    ctxs = [polyfuzz_amd.Context(0), polyfuzz_amd.Context(0)]
    comms = _lib.Comm.local_group(ctxs)
    bounds = [pipeline.shard_bounds(len(a), 2, r) for r in range(2)]
    sizes = [e - s for s, e in bounds]

    def rank_fn(r, self_match):
        s, e = bounds[r]
        job = pipeline.DenseMatchJob(ctxs[r], a[s:e], a if self_match else b, top_n=4, comm=comms[r],
                                     rows_per_rank=max(sizes), self_match=self_match, shard_offset=s if self_match else 0,
                                     compute_dtype="float16")
        assert job.from_dev.dtype == "float16" and job.to_dev.dtype == "float16"
        idx, val = job.step().download()
        return pipeline.TfidfMatchJob.unpad(idx, val, sizes, max(sizes))

    for self_match in (False, True):
        exp = _lib.dense_cossim_topn_host(ctx, a, a if self_match else b, 4, 0.0, exclude_diag=self_match, compute_dtype="float16")
        with cf.ThreadPoolExecutor(2) as ex:
            outs = [f.result(timeout=120) for f in [ex.submit(rank_fn, r, self_match) for r in range(2)]]
        for idx, val in outs:
            np.testing.assert_array_equal(idx, exp[0])
            np.testing.assert_array_equal(val, exp[1])
    for c in comms:
        c.free()


def test_fp32_path_unchanged(ctx):
    """compute_dtype=None and "float32" are the fp32 kernels: bit-identical to each other."""
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(130 + 257 + 768)
    a = rng.standard_normal((130, 768)).astype(np.float32)
    b = rng.standard_normal((257, 768)).astype(np.float32)
    r0 = _lib.dense_cossim_topn_host(ctx, a, b, 5, 0.0, compute_dtype=None)
    r1 = _lib.dense_cossim_topn_host(ctx, a, b, 5, 0.0, compute_dtype="float32")
    np.testing.assert_array_equal(r0[0], r1[0])
    np.testing.assert_array_equal(r0[1], r1[1])
    r16 = _lib.dense_cossim_topn_host(ctx, a, b, 5, 0.0, compute_dtype="float16")
    assert not np.array_equal(r0[1], r16[1])                                   # (the keyword does select another computation)
