"""Shared helpers of the parity tests (test infrastructure; may use oracle/)."""
import contextlib

import numpy as np

SCORE_TOL = 1e-5      # north-star tolerance for fp32 cosine scores
NEAR_TIE = 2e-6       # float64 oracle scores closer than this may swap ranks in fp32

_cache = {}


def vectorize_pair(oracle, from_list, to_list, cache_key=None, **kw):
    """TF-IDF CSR triples (float64) of from/to with the oracle's vectoriser
    (fit on to+from, reference _tfidf.py:109)."""
    if cache_key is not None and cache_key in _cache:
        return _cache[cache_key]
    v = oracle.TfidfOracle(**kw)
    if to_list is None:
        v.fit(from_list)
        a3 = v.transform(from_list)
        out = (a3, a3, len(v.vocabulary))
    else:
        v.fit(list(to_list) + list(from_list))
        out = (v.transform(from_list), v.transform(to_list), len(v.vocabulary))
    if cache_key is not None:
        _cache[cache_key] = out
    return out


def random_csr(rng, n_rows, n_cols, density, empty_rows=()):
    """Random non-negative CSR with L2-normalised rows, sorted indices."""
    indptr = [0]
    indices, data = [], []
    for r in range(n_rows):
        if r in empty_rows:
            indptr.append(len(indices))
            continue
        k = max(1, int(rng.binomial(n_cols, density)))
        cols = np.sort(rng.choice(n_cols, size=min(k, n_cols), replace=False))
        vals = rng.random(len(cols)) + 0.05
        vals /= np.sqrt((vals * vals).sum())
        indices.extend(cols.tolist())
        data.extend(vals.tolist())
        indptr.append(len(indices))
    return (np.array(indptr, np.int64), np.array(indices, np.int32), np.array(data, np.float64))


def assert_topn_parity(idx, val, exp_idx, exp_val, oracle, a3, b3, n_col, exclude_diag=False,
                       max_near_tie_frac=0.01, rows=None):
    """idx/val: engine output (int32, fp32); exp_*: oracle (canonical order, float64).
    rows: the from-rows of a3 that idx / val / exp_* hold, position by position (default: all of them, in order)."""
    idx = np.asarray(idx)
    val = np.asarray(val, np.float64)
    exp_idx = np.asarray(exp_idx)
    exp_val = np.asarray(exp_val, np.float64)
    assert idx.shape == exp_idx.shape, (idx.shape, exp_idx.shape)
    if idx.size == 0:
        return
    np.testing.assert_allclose(val, exp_val, rtol=0, atol=SCORE_TOL)
    bad_rows = np.nonzero((idx != exp_idx).any(axis=1))[0]
    assert len(bad_rows) <= max(1, int(max_near_tie_frac * len(idx))), \
        f"{len(bad_rows)} of {len(idx)} rows differ from the oracle's indices"
    for i in bad_rows:
        row = int(i) if rows is None else int(rows[i])
        dense = oracle.cossim_dense(a3, b3, n_col, rows=(row, row + 1))[0]
        got = idx[i]
        real = got[got >= 0]
        assert len(set(real.tolist())) == len(real), f"row {row}: duplicate indices {got}"
        if exclude_diag:
            assert row not in real.tolist()
        for r in range(idx.shape[1]):
            if got[r] == exp_idx[i, r]:
                continue
            # a swap is only acceptable between candidates the float64 oracle itself
            # separates by less than NEAR_TIE
            s_got = dense[got[r]] if got[r] >= 0 else 0.0
            assert abs(s_got - exp_val[i, r]) < NEAR_TIE, \
                f"row {row} rank {r}: got col {got[r]} (oracle score {s_got!r}), expected col " \
                f"{exp_idx[i, r]} (score {exp_val[i, r]!r})"


def assert_dense_topn(idx, val, e_idx, e_val, dense, tol=1e-5):
    """The dense (K5) tests' acceptance rule, e_idx / e_val / dense being the float64 oracle's top-n and score matrix: scores
    within `tol` absolute; an index may differ from the oracle's only where the oracle's score of the chosen column is within
    4e-6 of the expected one (only float64 near-ties may swap); such rows are at most max(1, n / 100)"""
    np.testing.assert_allclose(val, e_val, rtol=0, atol=tol)
    bad = np.nonzero((idx != e_idx).any(axis=1))[0]
    for i in bad:
        for r in range(idx.shape[1]):
            if idx[i, r] != e_idx[i, r]:
                s = dense[i, idx[i, r]] if idx[i, r] >= 0 else 0.0
                assert abs(s - e_val[i, r]) < 4e-6, (i, r, idx[i], e_idx[i])
    assert len(bad) <= max(1, len(idx) // 100)


# ---- the headline held to the REFERENCE's own run (tests/golden/headline_knn_golden_*.npz, make_golden_headline.py) ---------

HEADLINE_GOLDEN_PARTS = 4          # consecutive row blocks of 25 000 rows: each file stays well below 1 MiB


def load_headline_golden():
    import os
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    parts = [np.load(os.path.join(d, f"headline_knn_golden_{p}.npz")) for p in range(HEADLINE_GOLDEN_PARTS)]
    return {k: np.concatenate([g[k] for g in parts]) for k in ("idx", "sim", "sim3", "to_none")}


def assert_topn_equals_reference_knn(idx, val, golden, true_score, rows=None, score_tol=SCORE_TOL):
    """idx / val: an engine's (or the oracle's) self-match top-5 of the 100 000 company names, rows `rows` (default: all), canonical
    order; golden: what `polyfuzz.models.TFIDF(min_similarity=0, top_n=5, cosine_method="knn").match(names)` -- the REFERENCE, run in the
    build container -- returned for them.  true_score(r, j) -> float64 cosine of the pairs (r[i], j[i]) from the oracle-built matrix.

    The rule (SURVEY section 7 "Ties"): the scores agree rank by rank within the north-star's 1e-5 on EVERY cell; wherever the index
    at a rank differs, the reference's choice must score the same as ours at that rank (NEAR_TIE: an exact tie, resolved by
    sklearn's unspecified argpartition order there and by ascending index here) -- or be the row itself, `_utils.py:61-65`'s quirk:
    neighbour column 0 is dropped as "self", which keeps the row's own index wherever an exact duplicate took column 0; such a
    row must have a perfect match here.  Empty cells (score 0 / index -1 here) must be the frame's None cells."""
    idx, val = np.asarray(idx), np.asarray(val, np.float64)
    if rows is None:
        rows = np.arange(len(idx))
    rows = np.asarray(rows)
    r_idx, r_sim, r_none = golden["idx"][rows], golden["sim"][rows].astype(np.float64), golden["to_none"][rows]
    assert idx.shape == r_idx.shape
    err = np.abs(val - r_sim)
    assert err.max() <= score_tol, f"max |score - reference| = {err.max()} at {np.unravel_index(err.argmax(), err.shape)}"
    empty = idx < 0
    assert np.array_equal(empty, val == 0)
    # the reference's None cells are its cells below 0.001 after rounding: ours that round the same way
    mine_none = np.round(val, 3) < 0.001
    edge = np.abs(r_sim - 0.0005) < 2 * score_tol
    assert np.array_equal(mine_none | edge, r_none | edge)
    rr, kk = np.nonzero((idx != r_idx) & ~r_none & ~empty)
    jj = r_idx[rr, kk]
    is_self = jj == rows[rr]
    ts = true_score(rows[rr[~is_self]], jj[~is_self])
    not_tie = np.abs(ts - val[rr[~is_self], kk[~is_self]]) > NEAR_TIE
    assert not not_tie.any(), (f"{int(not_tie.sum())} cells where the reference chose a column that is no tie of ours; first: row "
                               f"{rows[rr[~is_self]][not_tie][:3]}, reference column {jj[~is_self][not_tie][:3]}")
    assert (val[rr[is_self], 0] >= 1.0 - NEAR_TIE).all() and (val[rr[is_self], kk[is_self]] >= 1.0 - NEAR_TIE).all()
    # an empty cell of ours facing a real cell of the reference (or the other way round) was caught by the None test above
    return {"cells": int(idx.size), "cells_index_differs": int(len(rr)), "of_them_reference_kept_self": int(is_self.sum()),
            "max_abs_score_err": float(err.max())}


# ---- config 3's lists under all ten fuzz scorers, the C oracle's answers (tests/golden/c3_fuzz_oracle_*.npz, make_golden_c3_fuzz.py) ----

# scorer -> row stride of its fixture: every row for seven, every 10th row (0, 10, 20, ...) for the three partial_token_* scorers
# (0.27 - 0.54 s per row on one core of the oracle: 46 minutes of eight cores for all rows)
C3_FUZZ_SCORERS = {"ratio": 1, "QRatio": 1, "token_sort_ratio": 1, "token_set_ratio": 1, "token_ratio": 1, "partial_ratio": 1,
                   "WRatio": 1, "partial_token_sort_ratio": 10, "partial_token_set_ratio": 10, "partial_token_ratio": 10}


def c3_fuzz_lists():
    """the one place the fixture's generator, its self-check and the GPU tests take the two lists from"""
    from polyfuzz_amd import datasets
    fl, tl = datasets.c3_lists()
    assert len(fl) == len(tl) == 20_000 and fl[0] == "Polly Blue Eyes"
    return fl, tl


def lists_sha256(from_list, to_list):
    import hashlib
    h = hashlib.sha256()
    for lst in (from_list, to_list):
        h.update("\0".join(lst).encode("utf-8", "surrogatepass"))
        h.update(b"\0\0")
    return h.hexdigest()


def c3_fuzz_golden_path(scorer):
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"c3_fuzz_oracle_{scorer}.npz")


def load_c3_fuzz_golden(scorer):
    """-> (rows int64, idx int32, score float64) of the fixture; a missing file raises (a test fails on it, it does not skip)"""
    g = np.load(c3_fuzz_golden_path(scorer))
    stride = C3_FUZZ_SCORERS[scorer]
    assert str(g["scorer"]) == scorer and int(g["stride"]) == stride and str(g["source"]) == "oracle"
    rows = np.arange(0, 20_000, stride)
    idx, score = g["idx"], g["score"]
    assert idx.dtype == np.int32 and score.dtype == np.float64 and idx.shape == score.shape == rows.shape
    return rows, idx, score


# ---- K8 held to the C oracle (oracle/jaro.c); config 3's lists at full size (tests/golden/c3_jaro_oracle_*.npz, make_golden_c3_jaro.py) ----

JARO_SCORERS = ("jaro", "jaro_winkler")


def _row_shards(n_rows, workers):
    cuts = np.linspace(0, n_rows, min(workers, max(n_rows, 1)) * 4 + 1).astype(np.int64)
    return [(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


def jaro_oracle_matrix(oracle, from_list, to_list, scorer, workers=8):
    """oracle.jaro_matrix with the from-rows cut over a thread pool (ctypes releases the GIL for the C call)"""
    import concurrent.futures as cf
    out = np.empty((len(from_list), len(to_list)), np.float64)
    with cf.ThreadPoolExecutor(workers) as ex:
        for (a, b), part in zip(_row_shards(len(from_list), workers),
                                ex.map(lambda r: oracle.jaro_matrix(from_list, to_list, scorer, rows=r), _row_shards(len(from_list), workers))):
            out[a:b] = part
    return out


def jaro_oracle_argmax(oracle, from_list, to_list, scorer, skip=None, workers=8):
    """oracle.jaro_argmax with the from-rows cut over a thread pool: (int32 idx, float64 score) of every from-row"""
    import concurrent.futures as cf
    with cf.ThreadPoolExecutor(workers) as ex:
        parts = list(ex.map(lambda r: oracle.jaro_argmax(from_list, to_list, scorer, skip, rows=r), _row_shards(len(from_list), workers)))
    if not parts:
        return np.empty(0, np.int32), np.empty(0, np.float64)
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def c3_jaro_golden_path(scorer):
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"c3_jaro_oracle_{scorer}.npz")


def load_c3_jaro_golden(scorer):
    """-> (idx int32[20 000], score float64[20 000]) of the fixture; a missing file raises (a test fails on it, it does not skip)"""
    g = np.load(c3_jaro_golden_path(scorer))
    assert str(g["scorer"]) == scorer and str(g["source"]) == "oracle"
    idx, score = g["idx"], g["score"]
    assert idx.dtype == np.int32 and score.dtype == np.float64 and idx.shape == score.shape == (20_000,)
    return idx, score


# ---- which form of K3 served a call ---------------------------------------------------------------------------------------------

@contextlib.contextmanager
def lockstep_launches(ctx):
    """with lockstep_launches(ctx) as box: ...calls...  ->  box["launches"] = how many of them k3_lockstep.hip served (every form of
    K3 is timed as `k3_cossim_topn`; the lock-step launch counts itself as `k3_lockstep` beside it while profiling is on) and
    box["k3"] = (ms, launches) of `k3_cossim_topn` over the same calls."""
    box = {}
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        yield box
        ctx.sync()
        ms, n = ctx.prof_get("k3_lockstep")
        assert ms == 0.0                          # a count, not a second timer inside the timed scope
        box["launches"], box["k3"] = n, ctx.prof_get("k3_cossim_topn")
    finally:
        ctx.prof_enable(False)
