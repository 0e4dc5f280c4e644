"""GPU tests of the exact rescoring of a 16-bit / int8 top-n (k5_rescore_topn, pfz_dense_rescore_topn and the doors above it).
The expected result of a candidate-restricted search is built here from the float64 oracle: the row's candidate columns,
lexsorted by (score descending, column ascending), strict > on the bound.  Scores are held by the rule of the other dense
tests (tests/helpers.py::assert_dense_topn): 1e-5 absolute; an index may differ only where the oracle's score of the chosen
column is within 4e-6 of the expected one, in at most max(1, n / 100) rows."""
import concurrent.futures as cf
import pickle

import numpy as np
import pytest

from tests.helpers import assert_dense_topn as _check

pytestmark = pytest.mark.gpu


def _restricted(dense, cand, ntop, lower_bound):
    """the canonical top-n of every row of the float64 score matrix `dense` over the columns cand[row] (-1: none)"""
    n = len(cand)
    idx = np.full((n, ntop), -1, np.int32)
    val = np.zeros((n, ntop), np.float64)
    lb = max(lower_bound, 0.0)
    for i in range(n):
        cols = cand[i][cand[i] >= 0].astype(np.int64)
        s = dense[i, cols]
        order = np.lexsort((cols, -s))
        order = order[s[order] > lb][:ntop]
        idx[i, :len(order)] = cols[order]
        val[i, :len(order)] = s[order]
    return idx, val


def _candidates(rng, n_from, n_to, m):
    """random distinct columns, a random number of them per row (0 .. m), at random slots: the -1s are scattered; every
    seventh row has none at all"""
    cand = np.full((n_from, m), -1, np.int32)
    for i in range(n_from):
        count = min(n_to, m) if n_from == 1 else min(n_to, int(rng.integers(0, m + 1)))
        if n_from > 1 and i % 7 == 3:
            count = 0
        cand[i, rng.permutation(m)[:count]] = rng.permutation(n_to)[:count]
    return cand


def _rescore(ctx, a, b, cand, ntop, lower_bound, normalize=True):
    from polyfuzz_amd import _lib
    ha = _lib.DeviceDense.upload(ctx, a, normalize)
    hb = _lib.DeviceDense.upload(ctx, b, normalize)
    table = _lib.DeviceTopN.from_host(ctx, cand, np.full(cand.shape, np.nan, np.float32))      # the val half is ignored
    return _lib.dense_rescore(ctx, ha, hb, table, ntop, lower_bound).download()


KERNEL = [(1, 1, 1, 1, 1),
          (6, 3, 300, 3, 2),
          (130, 257, 33, 64, 5),          # width one past a chunk
          (70, 3000, 768, 1024, 128),     # the largest m: four keys per thread
          (40, 1500, 4096, 20, 5),        # the longest rows still shared through LDS
          (5, 40, 4100, 8, 3)]            # one chunk beyond that: the from-row is re-read from L2


@pytest.mark.parametrize("n_from,n_to,d,m,ntop", KERNEL)
def test_kernel_alone_on_hand_made_candidates(ctx, oracle_mod, n_from, n_to, d, m, ntop):
    rng = np.random.default_rng(n_from + n_to + d + m)
    a = rng.standard_normal((n_from, d)).astype(np.float32)
    b = rng.standard_normal((n_to, d)).astype(np.float32)
    cand = _candidates(rng, n_from, n_to, m)
    if n_from >= 40:
        assert (cand < 0).all(axis=1).any() and ((cand[:, :-1] < 0) & (cand[:, 1:] >= 0)).any()
    dense = oracle_mod.dense_cossim(a, b)
    for lb in (0.0, 0.02):
        idx, val = _rescore(ctx, a, b, cand, ntop, lb)
        e_idx, e_val = _restricted(dense, cand, ntop, lb)
        print((n_from, n_to, d, m, ntop), "bound", lb, "max |score - oracle| =", float(np.abs(val - e_val).max()),
              "rows off the oracle's order:", int((idx != e_idx).any(axis=1).sum()))
        _check(idx, val, e_idx, e_val, dense)
        assert ((idx < 0) == (val == 0)).all()
    # raw dot products: the operands' own factors are 1
    idx, val = _rescore(ctx, a, b, cand, ntop, 0.0, normalize=False)
    dots = oracle_mod.dense_cossim(a, b, normalize=False)
    e_idx, e_val = _restricted(dots, cand, ntop, 0.0)
    np.testing.assert_allclose(val, e_val, rtol=2e-7, atol=1e-6)      # one fp32 rounding of a float64 sum
    assert (idx == e_idx).all(axis=1).sum() >= n_from - max(1, n_from // 100)


def test_the_order_of_the_candidates_does_not_matter(ctx):
    rng = np.random.default_rng(64)
    for d in (300, 4100):
        n_from, n_to, m = (130, 257, 64) if d == 300 else (9, 60, 24)
        a = rng.standard_normal((n_from, d)).astype(np.float32)
        b = rng.standard_normal((n_to, d)).astype(np.float32)
        cand = _candidates(rng, n_from, n_to, m)
        shuffled = np.stack([row[rng.permutation(m)] for row in cand])
        assert (shuffled != cand).any()
        first = _rescore(ctx, a, b, cand, 5, 0.0)
        second = _rescore(ctx, a, b, shuffled, 5, 0.0)
        np.testing.assert_array_equal(first[0], second[0])
        np.testing.assert_array_equal(first[1].view(np.uint32), second[1].view(np.uint32))


def test_tie_rule_and_strict_bound(ctx, oracle_mod):
    """five exact duplicates among the to-rows, all in every row's candidate list: one score, ascending columns.  The bound is
    then set ON a known score (dropped: the comparison is strict) and between two known scores."""
    rng = np.random.default_rng(5)
    d, m = 96, 24
    b = rng.standard_normal((600, d)).astype(np.float32)
    dups = np.array([7, 130, 131, 402, 599])
    b[dups] = b[7]
    a = (b[7] + 0.8 * rng.standard_normal((20, d))).astype(np.float32)          # cosines of about 0.78 with the duplicates
    cand = np.full((20, m), -1, np.int32)
    others = np.setdiff1d(np.arange(600), dups)
    for i in range(20):
        row = np.concatenate([dups, rng.permutation(others)[:15]])
        cand[i, rng.permutation(m)[:20]] = rng.permutation(row)
    dense = oracle_mod.dense_cossim(a, b)
    idx, val = _rescore(ctx, a, b, cand, m, 0.0)
    # the duplicates' one score is rounded from float64 once, the oracle's five may differ in the last bits of a double:
    # expected order = the oracle's with the five columns given their common (first) score
    tied = dense.copy()
    tied[:, dups] = dense[:, [7]]
    e_idx, e_val = _restricted(tied, cand, m, 0.0)
    _check(idx, val, e_idx, e_val, tied)
    for i in range(20):
        at = int(np.nonzero(idx[i] == 7)[0][0])
        np.testing.assert_array_equal(idx[i, at:at + 5], dups)
        assert len(set(val[i, at:at + 5].view(np.uint32).tolist())) == 1
    at = int(np.nonzero(idx[0] == 7)[0][0])
    assert at + 6 < m and idx[0, at + 6] >= 0 and val[0, at + 5] > val[0, at + 6]
    on, between = float(val[0, at]), float(np.float32((np.float64(val[0, at + 5]) + np.float64(val[0, at + 6])) / 2))
    assert val[0, at + 5] > np.float32(between) > val[0, at + 6]
    for bound in (on, between):
        b_idx, b_val = _rescore(ctx, a, b, cand, m, bound)
        keep = val > np.float32(bound)                                            # of the first run's (sorted) rows: a prefix
        np.testing.assert_array_equal(b_idx, np.where(keep, idx, -1))
        np.testing.assert_array_equal(b_val.view(np.uint32), np.where(keep, val, np.float32(0)).view(np.uint32))
        assert (b_val[b_idx >= 0] > np.float32(bound)).all()
    b_idx, _ = _rescore(ctx, a, b, cand, m, on)
    assert not np.isin(b_idx[0], dups).any() and (b_idx[0] >= 0).sum() == at          # equal to the bound: dropped
    b_idx, _ = _rescore(ctx, a, b, cand, m, between)
    assert (b_idx[0] >= 0).sum() == at + 6


def test_rescoring_restores_the_fp32_ranking(ctx, oracle_mod):
    """What the feature is for: 300 x 2000 unit-Gaussian vectors of width 768 (the shape of
    tests/test_dense8_gpu.py::test_quantisation_cost_on_unit_gaussian_vectors), top-5.  A float64 simulation of the two
    roundings says: plain int8 differs from the exact top-5 in 75 rows, plain bfloat16 in 15, and the exact entries missing
    from the int8 candidates are 26 / 0 / 0 at multipliers 1 / 2 / 4.  An implementation that only re-ordered the coarse
    result, without reading the fp32 vectors, fails here."""
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(768)
    a = rng.standard_normal((300, 768)).astype(np.float32)
    b = rng.standard_normal((2000, 768)).astype(np.float32)
    dense = oracle_mod.dense_cossim(a, b)
    e_idx, e_val = oracle_mod.dense_cossim_topn(a, b, 5, 0.0)
    plain = {"int8": lambda n: _lib.dense_int8_topn_host(ctx, a, b, n, 0.0),
             "bfloat16": lambda n: _lib.dense_cossim_topn_host(ctx, a, b, n, 0.0, compute_dtype="bfloat16")}
    for coarse, least in (("int8", 30), ("bfloat16", 5)):
        idx, val = _lib.dense_rescored_topn_host(ctx, a, b, 5, 0.0, coarse=coarse, multiplier=4)
        p_idx, _ = plain[coarse](5)
        off_plain = int((p_idx != e_idx).any(axis=1).sum())
        off_rescored = int((idx != e_idx).any(axis=1).sum())
        missing = []
        for mult in (1, 2, 4):
            c_idx, _ = plain[coarse](5 * mult)
            missing.append(int(sum(len(np.setdiff1d(e_idx[i], c_idx[i])) for i in range(300))))
        print(f"{coarse}: rows whose top-5 differs from the float64 oracle's: plain {off_plain}, rescored (x4) {off_rescored} of 300; "
              f"exact top-5 entries missing from the candidates at multipliers 1 / 2 / 4: {missing} of 1500; "
              f"max |score - oracle| = {float(np.abs(val - e_val).max()):.2e}")
        _check(idx, val, e_idx, e_val, dense)
        assert off_plain >= least


def test_multiplier_one_keeps_the_coarse_columns(ctx, oracle_mod):
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(5)
    a = rng.standard_normal((130, 96)).astype(np.float32)
    b = rng.standard_normal((1500, 96)).astype(np.float32)
    dense = oracle_mod.dense_cossim(a, b)
    for coarse in ("int8", "float16"):
        if coarse == "int8":
            c_idx, _ = _lib.dense_int8_topn_host(ctx, a, b, 5, 0.0)
        else:
            c_idx, _ = _lib.dense_cossim_topn_host(ctx, a, b, 5, 0.0, compute_dtype=coarse)
        idx, val = _lib.dense_rescored_topn_host(ctx, a, b, 5, 0.0, coarse=coarse, multiplier=1)
        np.testing.assert_array_equal(np.sort(idx, axis=1), np.sort(c_idx, axis=1))
        e_idx, e_val = _restricted(dense, c_idx, 5, 0.0)
        _check(idx, val, e_idx, e_val, dense)


def test_self_match_and_lower_bound(ctx, oracle_mod):
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(9)
    a = rng.standard_normal((400, 96)).astype(np.float32)
    a[100:110] = a[:10] + 0.05 * rng.standard_normal((10, 96)).astype(np.float32)        # near-duplicates
    dense = oracle_mod.dense_cossim(a, a)
    bound = 0.25
    idx, val = _lib.dense_rescored_topn_host(ctx, a, a, 3, bound, coarse="int8", multiplier=4, exclude_diag=True)
    c_idx, c_val = _lib.dense_int8_topn_host(ctx, a, a, 12, 0.0, exclude_diag=True)
    assert (c_idx != np.arange(400)[:, None]).all()
    e_idx, e_val = _restricted(dense, c_idx, 3, bound)
    _check(idx, val, e_idx, e_val, dense)
    assert (idx != np.arange(400)[:, None]).all()                                       # row i never comes back for row i
    assert (idx[:10, 0] == np.arange(100, 110)).all() and (idx[100:110, 0] == np.arange(10)).all()
    assert (idx < 0).any() and (val[idx >= 0] > bound).all()                            # the bound does cut
    # ... on the exact score: a candidate whose int8 score is on the other side of the bound than its exact score goes by the latter
    exact_of = np.take_along_axis(dense, np.maximum(c_idx, 0).astype(np.int64), axis=1)
    crossed = (c_idx >= 0) & ((c_val > bound) != (exact_of > bound)) & (np.abs(exact_of - bound) > 1e-5)
    print("self-match: candidates whose int8 and exact scores lie on different sides of the bound:", int(crossed.sum()))
    for i, r in zip(*np.nonzero(crossed)):
        rank = int((exact_of[i][c_idx[i] >= 0] > exact_of[i, r]).sum())
        assert (c_idx[i, r] in idx[i]) == (exact_of[i, r] > bound and rank < 3)
    # and the unrestricted float64 top-3 is what comes out
    u_idx, u_val = oracle_mod.dense_cossim_topn(a, a, 3, bound, exclude_diag=True)
    _check(idx, val, u_idx, u_val, dense)


def test_clipping_and_refusals(ctx, oracle_mod):
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(50)
    a = rng.standard_normal((20, 64)).astype(np.float32)
    b = rng.standard_normal((50, 64)).astype(np.float32)
    assert _lib.rescore_candidates(10, 8, 50) == 50 and _lib.rescore_candidates(10, 8, 50, True) == 49
    assert _lib.rescore_candidates(10, 2, 50) == 20 and _lib.rescore_candidates(10, 8, 4) == 10
    idx, val = _lib.dense_rescored_topn_host(ctx, a, b, 10, 0.0, coarse="int8", multiplier=8)      # 80 candidates of 50 rows
    e_idx, e_val = oracle_mod.dense_cossim_topn(a, b, 10, 0.0)
    _check(idx, val, e_idx, e_val, oracle_mod.dense_cossim(a, b))
    idx, val = _lib.dense_rescored_topn_host(ctx, b, b, 10, 0.0, coarse="bfloat16", multiplier=8, exclude_diag=True)
    e_idx, e_val = oracle_mod.dense_cossim_topn(b, b, 10, 0.0, exclude_diag=True)
    _check(idx, val, e_idx, e_val, oracle_mod.dense_cossim(b, b))
    idx, val = _lib.dense_rescored_topn_host(ctx, a, b[:4], 10, 0.0, coarse="int8", multiplier=8)  # fewer to-rows than top_n
    e_idx, e_val = oracle_mod.dense_cossim_topn(a, b[:4], 10, 0.0)
    _check(idx, val, e_idx, e_val, oracle_mod.dense_cossim(a, b[:4]))

    big = rng.standard_normal((1100, 64)).astype(np.float32)
    x_a, x_b, x_big = (_lib.DeviceDense.upload(ctx, v) for v in (a, b, big))
    q_a, q_b, q_big = (_lib.DeviceDense.upload_int8(ctx, v) for v in (a, b, big))
    live = ctx.pool_stats()[0]
    with pytest.raises(ValueError, match=r"top_n=300.*rescore_multiplier=4.*1024"):
        _lib.dense_topn_rescored(ctx, q_a, q_big, x_a, x_big, 300, 0.0, 4)
    assert ctx.pool_stats()[0] == live                                  # refused before anything was allocated or enqueued
    with pytest.raises(ValueError, match="1024"):
        _lib.dense_rescored_topn_host(ctx, a, big, 300, 0.0, coarse="int8", multiplier=4)
    with pytest.raises(ValueError, match="coarse"):
        _lib.dense_rescored_topn_host(ctx, a, b, 3, 0.0, coarse="float32", multiplier=4)
    wide = _lib.DeviceTopN.alloc(ctx, 20, 1025)
    wide.clear()
    with pytest.raises(_lib.PfzUnsupported, match="1024"):
        _lib.dense_rescore(ctx, x_a, x_big, wide, 5, 0.0)
    table = _lib.dense_topn(ctx, q_a, q_b, 8, 0.0)
    h16 = _lib.DeviceDense.upload(ctx, a, True, "float16")
    for bad_a, bad_b in ((h16, x_b), (x_a, q_b), (q_a, q_b)):
        with pytest.raises(_lib.PfzError, match="float32"):
            _lib.dense_rescore(ctx, bad_a, bad_b, table, 3, 0.0)
    narrow = _lib.DeviceDense.upload(ctx, b[:, :63].copy())
    with pytest.raises(_lib.PfzError, match="64 columns.*63"):
        _lib.dense_rescore(ctx, x_a, narrow, table, 3, 0.0)
    with pytest.raises(_lib.PfzError, match="candidate table has 20 rows.*50"):
        _lib.dense_rescore(ctx, x_b, x_b, table, 3, 0.0)
    with pytest.raises(_lib.PfzError, match="ntop 9"):
        _lib.dense_rescore(ctx, x_a, x_b, table, 9, 0.0)
    with pytest.raises(_lib.PfzError, match="result buffer"):
        _lib.dense_rescore(ctx, x_a, x_b, table, 3, 0.0, out=_lib.DeviceTopN.alloc(ctx, 20, 4))
    # the handles are still good
    idx, val = _lib.dense_topn_rescored(ctx, q_a, q_b, x_a, x_b, 3, 0.0, 4).download()
    ref = _lib.dense_rescored_topn_host(ctx, a, b, 3, 0.0, coarse="int8", multiplier=4)
    np.testing.assert_array_equal(idx, ref[0])
    np.testing.assert_array_equal(val, ref[1])
    idx, val = _lib.dense_rescore(ctx, x_a, x_b, table, 8, 0.0).download()
    assert (idx[:, 0] >= 0).all()
    empty = _lib.dense_rescore(ctx, _lib.DeviceDense.upload(ctx, a[:0]), x_b, table, 3, 0.0)       # no from-rows: nothing to do
    assert empty.download()[0].shape == (0, 3)


def test_embeddings_with_a_rescore_multiplier(ctx):
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import Embeddings
    from polyfuzz_amd.models._utils import topn_to_frame
    rng = np.random.default_rng(21)
    a = rng.standard_normal((301, 96)).astype(np.float32)
    b = rng.standard_normal((530, 96)).astype(np.float32)
    fl, tl = [f"f{i}" for i in range(len(a))], [f"t{i}" for i in range(len(b))]
    ref_idx, ref_val = _lib.dense_rescored_topn_host(ctx, a, b, 4, 0.0, coarse="int8", multiplier=4)
    m = Embeddings(min_similarity=0.0, top_n=4, cosine_method="hip")
    m.precision = "int8"
    plain = m.match(fl, tl, embeddings_from=a, embeddings_to=b)
    coarse_handle = m._dev_to
    assert m._dev_to_exact is None
    m.rescore_multiplier = 4
    df = m.match(fl, tl, embeddings_from=a, embeddings_to=b, re_train=False)       # the multiplier alone re-uploads nothing ...
    assert m._dev_to is coarse_handle and m._dev_to_exact.dtype == "float32"       # ... the float32 to-side comes beside it
    expect = topn_to_frame(ref_idx, ref_val, fl, tl, 4)
    assert list(df.columns) == list(expect.columns) and len(df.columns) == 9
    for col in df.columns:
        assert df[col].tolist() == expect[col].tolist(), col
    np.testing.assert_array_equal(df["Similarity_3"].to_numpy(), np.round(ref_val[:, 2].astype(np.float64), 3))
    assert not df.equals(plain)
    coarse, exact = m._dev_to, m._dev_to_exact
    df2 = m.match(fl[:50], tl, embeddings_from=a[:50], re_train=False)              # both to-sides: resident, not re-uploaded
    assert m._dev_to is coarse and m._dev_to_exact is exact
    assert df2.equals(df.iloc[:50].reset_index(drop=True))
    m.rescore_multiplier = 8
    m.match(fl[:50], tl, embeddings_from=a[:50], re_train=False)
    assert m._dev_to is coarse and m._dev_to_exact is exact
    m.rescore_multiplier = 4
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.rescore_multiplier == 4 and m2.precision == "int8" and m2._dev_to is None and m2._dev_to_exact is None
    assert m2.match(fl[:50], tl, embeddings_from=a[:50], re_train=False).equals(df2)
    m.match(fl, tl, embeddings_from=a, embeddings_to=b)                             # re_train: both follow
    assert m._dev_to is not coarse and m._dev_to_exact is not exact and m._dev_to_exact is not None
    m.rescore_multiplier = None
    assert m.match(fl, tl, embeddings_from=a, embeddings_to=b).equals(plain)
    m.rescore_multiplier = 4
    m.precision = None
    with pytest.raises(ValueError, match="nothing to rescore"):
        m.match(fl, tl, embeddings_from=a, embeddings_to=b)
    m.precision = "int8"
    q = np.clip(np.rint(a * 40), -127, 127).astype(np.int8)
    with pytest.raises(ValueError, match="no full-precision vectors"):
        m.match(fl, tl, embeddings_from=q, embeddings_to=b)
    m.precision, m.compute_dtype = None, "float16"
    with pytest.raises(ValueError, match="no full-precision vectors"):
        m.match(fl, tl, embeddings_from=a, embeddings_to=b.astype(np.float16))
    ref16 = _lib.dense_rescored_topn_host(ctx, a, b, 4, 0.0, coarse="float16", multiplier=4)
    df16 = m.match(fl, tl, embeddings_from=a, embeddings_to=b)
    assert df16["To_4"].tolist() == [tl[j] for j in ref16[0][:, 3]]
    e = Embeddings(embedding_method=lambda strings: a[[int(s[1:]) for s in strings]], min_similarity=0.0, top_n=4,
                   cosine_method="hip")
    e.precision, e.rescore_multiplier = "int8", 2                                   # what an embedding_method returns; self-match
    own = e.match(fl[:50])
    assert (own["To"] != own["From"]).all() and e._dev_to_exact.dtype == "float32"


def test_sharded_dense_job_with_rescoring(ctx):
    """DenseMatchJob on two contexts of one device with uneven shards, as tests/test_dense8_gpu.py::test_sharded_dense_job_int8,
    with rescoring == the one-shot call, bit for bit."""
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
        to = a if self_match else b
        job = pipeline.DenseMatchJob(ctxs[r], _lib.DeviceDense.upload_int8(ctxs[r], a[s:e]), _lib.DeviceDense.upload_int8(ctxs[r], to),
                                     top_n=4, comm=comms[r], rows_per_rank=max(sizes), self_match=self_match,
                                     shard_offset=s if self_match else 0, rescore_multiplier=4,
                                     rescore_from=a[s:e], rescore_to=_lib.DeviceDense.upload(ctxs[r], to) if r else to)
        assert job.from_exact.dtype == "float32" and job.candidates.ntop == 16 and job.candidates.n_rows == e - s
        table = job.candidates
        job.step()
        idx, val = job.step().download()
        assert job.candidates is table                                # allocated once, at construction
        return pipeline.TfidfMatchJob.unpad(idx, val, sizes, max(sizes))

    for self_match in (False, True):
        exp = _lib.dense_rescored_topn_host(ctx, a, a if self_match else b, 4, 0.0, coarse="int8", multiplier=4,
                                            exclude_diag=self_match)
        with cf.ThreadPoolExecutor(2) as ex:
            outs = [f.result(timeout=120) for f in [ex.submit(rank_fn, r, self_match) for r in range(2)]]
        for idx, val in outs:
            np.testing.assert_array_equal(idx, exp[0])
            np.testing.assert_array_equal(val, exp[1])
    with pytest.raises(ValueError, match="nothing to rescore"):
        pipeline.DenseMatchJob(ctx, a, b, top_n=4, rescore_multiplier=4, rescore_from=a, rescore_to=b)
    with pytest.raises(ValueError, match="rescore_from and rescore_to"):
        pipeline.DenseMatchJob(ctx, a, b, top_n=4, compute_dtype="bfloat16", rescore_multiplier=4, rescore_from=a)
    with pytest.raises(ValueError, match="1024"):
        pipeline.DenseMatchJob(ctx, a, np.tile(b, (3, 1)), top_n=300, compute_dtype="bfloat16", rescore_multiplier=4, rescore_from=a,
                               rescore_to=np.tile(b, (3, 1)))
    for c in comms:
        c.free()
