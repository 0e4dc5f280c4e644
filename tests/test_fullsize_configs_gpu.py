"""Configs 3 (RapidFuzz; and the same lists under K8's Jaro / Jaro-Winkler), 4 and 5 of BASELINE.json held to the CPU oracle AT THEIR REAL SIZE inside the suite -- until now three of the
five benchmark configurations met the oracle at full size only in `bench.py --full`:

* K7: the whole 20 000 x 20 000 IMDB-title configuration under all ten rapidfuzz.fuzz scorers, bit for bit against
  tests/golden/c3_fuzz_oracle_*.npz (the C oracle's answers, make_golden_c3_fuzz.py; tests/test_fuzz_golden_cpu.py keeps the files
  equal to the committed oracle), the matchers' frames and K7's schedule knobs on the same rows;
* K3 lock-step on its natural dispatch: config 4's shard (125 000 x 1 000 000 synthetic names, top-10), no PFZ_* variable set,
  against the oracle chain (numpy vectoriser -> float64 product) on 2 176 rows, properties and lock-step == row-major on all rows;
* K5 at config 5's width: 4 352 x 500 000 x 768 (two whole 4 GiB score panels and a short third), natural panels.
"""
import concurrent.futures as cf
import gc
import os

import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu


# ---- 1. config 3's lists, all ten scorers --------------------------------------------------------------------------------------------

K3_ENV = ("PFZ_K3_LOCKSTEP", "PFZ_K3_BLOCK", "PFZ_K3_SYM")


def _assert_rows_equal(what, fl, tl, rows, idx, score, e_idx, e_score):
    """idx / score: the device's answer for the fixture rows `rows`; a mismatch names its rows before numpy's report"""
    bad = np.nonzero((idx != e_idx) | (score != e_score))[0]
    if len(bad):
        lines = [f"row {int(rows[k])} {fl[int(rows[k])]!r}: got choice {int(idx[k])} ({tl[int(idx[k])]!r}) score {float(score[k])!r}, "
                 f"fixture choice {int(e_idx[k])} ({tl[int(e_idx[k])]!r}) score {float(e_score[k])!r}" for k in bad[:5]]
        raise AssertionError(f"{what}: {len(bad)} of {len(rows)} rows differ from the oracle fixture\n" + "\n".join(lines))
    np.testing.assert_array_equal(score, e_score, err_msg=what)
    np.testing.assert_array_equal(idx, e_idx, err_msg=what)


@pytest.fixture(scope="module")
def c3():
    fl, tl = helpers.c3_fuzz_lists()
    return fl, tl


@pytest.mark.parametrize("scorer", sorted(helpers.C3_FUZZ_SCORERS))
def test_config_3_lists_every_scorer_equals_the_oracle_fixture(ctx, c3, scorer):
    """`best_choice` (K7 for seven scorers, K4 for ratio / QRatio / token_sort_ratio) on the full lists: first best choice and float64
    score equal the fixture on EVERY fixture row -- 20 000 rows, every 10th (2 000) for the three partial_token_* scorers.  No
    tolerance and no allowance for ties: the oracle's rule is "first best", the kernels claim the same."""
    from polyfuzz_amd.models._rapidfuzz import best_choice
    fl, tl = c3
    rows, e_idx, e_score = helpers.load_c3_fuzz_golden(scorer)
    assert len(rows) == (2_000 if scorer.startswith("partial_token") else 20_000)
    idx, score = best_choice(ctx, scorer, fl, tl, None, False)
    assert idx.shape == score.shape == (20_000,) and idx.dtype == np.int32 and score.dtype == np.float64
    _assert_rows_equal(scorer, fl, tl, rows, idx[rows], score[rows], e_idx, e_score)


@pytest.mark.parametrize("scorer", ["WRatio", "partial_ratio", "token_set_ratio", "token_ratio", "partial_token_sort_ratio",
                                    "partial_token_set_ratio", "partial_token_ratio"])
def test_config_3_lists_resident_k7_equals_the_oracle_fixture(ctx, c3, scorer):
    """... and what bench.py times: `_lib.fuzz_extract_one` on RESIDENT lists (forms and plan cached on the handles), a second call on
    the same handles included"""
    from polyfuzz_amd import _lib
    fl, tl = c3
    rows, e_idx, e_score = helpers.load_c3_fuzz_golden(scorer)
    f_dev, t_dev = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for call in ("first call", "second call"):
        idx, score = _lib.fuzz_extract_one(ctx, f_dev, t_dev, scorer)
        _assert_rows_equal(f"{scorer}, resident lists, {call}", fl, tl, rows, idx[rows], score[rows], e_idx, e_score)


@pytest.mark.parametrize("knob,value", [("PFZ_K7_NO_HANDOVER", "1"), ("PFZ_K7_NO_SIDE_STREAM", "1"), ("PFZ_K7_PARTS", "3")])
def test_config_3_wratio_under_the_schedule_knobs_equals_the_oracle_fixture(ctx, c3, monkeypatch, knob, value):
    """K7's schedule knobs (no heavy-row hand-over, no side stream for the long classes, every class in three parts) against the
    ORACLE on all 20 000 rows, not against another run of the kernel"""
    from polyfuzz_amd.models._rapidfuzz import best_choice
    fl, tl = c3
    rows, e_idx, e_score = helpers.load_c3_fuzz_golden("WRatio")
    assert len(rows) == 20_000
    monkeypatch.setenv(knob, value)
    idx, score = best_choice(ctx, "WRatio", fl, tl, None, False)
    _assert_rows_equal(f"WRatio under {knob}={value}", fl, tl, rows, idx[rows], score[rows], e_idx, e_score)


def test_config_3_matcher_frames_equal_the_oracle_fixture(ctx, c3):
    """The user-level calls at this size: `RapidFuzz().match(from, to)` (WRatio), `RapidFuzz(score_cutoff=0.9)`, and
    `EditDistance(scorer="token_set_ratio", normalize=False)` -- From, To and Similarity of all 20 000 rows derived from the fixture"""
    from polyfuzz_amd.models import EditDistance, RapidFuzz
    fl, tl = c3
    rows, e_idx, e_score = helpers.load_c3_fuzz_golden("WRatio")
    assert len(rows) == 20_000 and (e_idx >= 0).all()
    df = RapidFuzz().match(fl, tl)
    assert len(df) == 20_000 and df["From"].tolist() == fl
    assert df["To"].tolist() == [tl[j] for j in e_idx.tolist()]
    np.testing.assert_array_equal(df["Similarity"].to_numpy(), e_score / 100)
    dc = RapidFuzz(score_cutoff=0.9).match(fl, tl)
    hit = e_score >= 0.9 * 100                # (test_rapidfuzz_matcher_default_scorer's expression; 0.9 * 100 is 90.0 in float64)
    assert 0 < hit.sum() < len(hit) and ((e_score == 90.0) & hit).sum() > 1000       # 5 437 rows sit exactly ON the cut-off: kept
    assert dc["From"].tolist() == fl
    assert dc["To"].tolist() == [tl[j] if h else None for j, h in zip(e_idx.tolist(), hit.tolist())]
    np.testing.assert_array_equal(dc["Similarity"].to_numpy(), np.where(hit, e_score / 100, 0.0))
    rows, s_idx, s_score = helpers.load_c3_fuzz_golden("token_set_ratio")
    assert len(rows) == 20_000
    de = EditDistance(scorer="token_set_ratio", normalize=False).match(fl, tl)
    assert de["From"].tolist() == fl
    assert de["To"].tolist() == [tl[j] for j in s_idx.tolist()]
    np.testing.assert_array_equal(de["Similarity"].to_numpy(), s_score)


# ---- 1b. config 3's lists under Jaro / Jaro-Winkler (K8 at the size its timing is quoted at) ---------------------------------------

@pytest.mark.parametrize("scorer", helpers.JARO_SCORERS)
def test_config_3_lists_jaro_equals_the_oracle_fixture(ctx, c3, scorer):
    """K8 on the RESIDENT 20 000 x 20 000 titles (what tools/bench_jaro.py times): first arg-max and float64 score of all 20 000 rows ==
    tests/golden/c3_jaro_oracle_*.npz (oracle/jaro.c's answers; tests/test_jaro_golden_cpu.py keeps the files equal to the committed
    oracle), through the host entry and jaro_argmax_dev.  The share of the 4e8 pairs whose float64 score the arg-max computed is
    printed.  Measured on an MI355X: 43 382 896 (Jaro) / 43 383 985 (Jaro-Winkler) of 4e8 pairs, 10.85 %."""
    from polyfuzz_amd import _lib
    fl, tl = c3
    e_idx, e_score = helpers.load_c3_jaro_golden(scorer)
    rows = np.arange(20_000)
    f_dev, t_dev = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        idx, score = _lib.jaro_argmax(ctx, f_dev, t_dev, scorer)
        scored = ctx.prof_get("k8_pairs_scored")[1]
    finally:
        ctx.prof_enable(False)
    print(f"K8 {scorer}, 20 000 x 20 000 titles: {scored} of {len(fl) * len(tl)} pairs scored, share {scored / (len(fl) * len(tl)):.4f}")
    assert idx.shape == score.shape == (20_000,) and idx.dtype == np.int32 and score.dtype == np.float64
    _assert_rows_equal(f"{scorer}, resident lists", fl, tl, rows, idx, score, e_idx, e_score)
    assert 0 < scored < len(fl) * len(tl)
    out = _lib.DeviceTopN.alloc(ctx, 20_000, 2)
    _lib.jaro_argmax_dev(ctx, f_dev, t_dev, scorer, out)
    d_idx, d_score = _lib.best_from_topn(*out.download())
    _assert_rows_equal(f"{scorer}, resident lists, device entry", fl, tl, rows, d_idx[:20_000], d_score[:20_000], e_idx, e_score)


def test_config_3_jaro_winkler_matcher_frame_equals_the_oracle_fixture(ctx, c3):
    """`EditDistance(scorer="jaro_winkler", normalize=False).match(from, to)` at this size: From, To and Similarity of all 20 000 rows
    from the fixture"""
    from polyfuzz_amd.models import EditDistance
    fl, tl = c3
    e_idx, e_score = helpers.load_c3_jaro_golden("jaro_winkler")
    df = EditDistance(scorer="jaro_winkler", normalize=False).match(fl, tl)
    assert len(df) == 20_000 and df["From"].tolist() == fl
    assert df["To"].tolist() == [tl[j] for j in e_idx.tolist()]
    np.testing.assert_array_equal(df["Similarity"].to_numpy(), e_score)


# ---- 2. config 4's shard on the lock-step kernel's natural dispatch ------------------------------------------------------------------

C4_TO, C4_FROM, C4_TOP = 1_000_000, 125_000, 10


def _k3_env_set():
    return sorted(k for k in os.environ if k in K3_ENV or k.startswith("PFZ_K3_LS_"))


@pytest.fixture(scope="module")
def c4(ctx):
    """what bench.py's run_tfidf_1m builds: 125 000 synthetic from-names against 1 000 000 synthetic to-names, vectoriser fitted on
    to + from, top-10 -- with NO knob set: slice width, chunk size, grid and the kernel itself are the library's own choice"""
    from polyfuzz_amd import _lib, synth
    assert _k3_env_set() == [], "this module tests the natural dispatch"
    tl, fl = synth.company_names(C4_TO, 5678), synth.company_names(C4_FROM, 1234)
    t, f = _lib.DeviceStrings.upload(ctx, tl), _lib.DeviceStrings.upload(ctx, fl)
    vec = _lib.DeviceTfidf.fit(ctx, _lib.TfidfParams(3, 3, 1, 1), t, f)
    a, b = vec.transform(f), vec.transform(t)
    ix = _lib.DeviceIndex.build(ctx, b)
    with helpers.lockstep_launches(ctx) as served:
        idx, val = _lib.cossim_topn(ctx, ix, a, C4_TOP, 0.0).download()
    idx2, val2 = _lib.cossim_topn(ctx, ix, a, C4_TOP, 0.0).download()
    out = {"fl": fl, "tl": tl, "a": a, "b": b, "ix": ix, "idx": idx, "val": val, "idx2": idx2, "val2": val2, "served": served}
    yield out
    out.clear()
    gc.collect()


@pytest.fixture(scope="module")
def c4_oracle(c4, oracle_mod):
    """the two lists through the ORACLE vectoriser (oracle/tfidf_numpy.py == scikit-learn bit for bit): float64 CSR of both"""
    o = oracle_mod.TfidfNumpyOracle()
    o.fit(list(c4["tl"]) + list(c4["fl"]))
    b3, a3 = o.transform_fitted(0, C4_TO), o.transform_fitted(C4_TO, C4_TO + C4_FROM)
    out = {"a3": a3, "b3": b3, "n_col": len(o.codes)}
    del o
    yield out
    out.clear()
    gc.collect()


def test_config_4_the_lockstep_kernel_served_the_default_call(ctx, c4, monkeypatch):
    """1 000 000 to-rows and 125 000 from-rows: beyond both bars of k3_lockstep_wanted.  The launch counts itself (`k3_lockstep`,
    read through Context.prof_get) beside the one timed scope all forms of K3 share; the row-major run under PFZ_K3_LOCKSTEP=0
    counts none -- and returns the same 125 000 x 10 cells, bit for bit."""
    from polyfuzz_amd import _lib
    assert c4["served"]["launches"] == 1
    assert c4["served"]["k3"][1] == 1 and c4["served"]["k3"][0] > 0          # (timed as k3_cossim_topn, once, as before)
    info = c4["ix"].info()
    per_slice = 4 if info["block_cols"] == 4096 else 8                        # (k3_lockstep_launch's default slice width)
    assert info["n_rows"] == C4_TO and -(-info["n_blocks"] // per_slice) >= 60  # the kept keys travel through HBM 60+ times
    monkeypatch.setenv("PFZ_K3_LOCKSTEP", "0")
    with helpers.lockstep_launches(ctx) as served:
        r_idx, r_val = _lib.cossim_topn(ctx, c4["ix"], c4["a"], C4_TOP, 0.0).download()
    assert served["launches"] == 0 and served["k3"][1] == 1
    np.testing.assert_array_equal(c4["idx"], r_idx)
    np.testing.assert_array_equal(c4["val"], r_val)


def test_config_4_properties_on_all_rows(c4, c4_oracle, oracle_mod):
    """Two runs bit-identical; scores non-increasing and in [0, 1 + 1e-6]; -1 exactly where the score is 0; no column twice in a row;
    ties ordered by ascending column.  A tie is two equal SUMS: the kernels order keys (fixed-point sum, column) and print the sum as
    fp32, so two sums less than an fp32 spacing apart (6e-8 below 1.0; the sums carry 30 bits here) print equal while the larger one
    rightly comes first whatever its column.  Hence: equal printed scores with a DESCENDING column are accepted only where the float64
    oracle ranks the first candidate strictly above the second, by less than NEAR_TIE -- the kernel's order is then the true one.
    Measured: 556 484 tie cells, 2 of them descending (rows 29 893 and 84 219, oracle differences 4.1e-8 and 1.5e-8).  Their number is
    capped at 0.1 % of the rows: 0.39 % of the rows have unequal neighbours within 2e-6 at all (the figure under the sample test), an
    fp32 spacing is 3 % of that range."""
    idx, val = c4["idx"], c4["val"]
    assert idx.shape == val.shape == (C4_FROM, C4_TOP)
    np.testing.assert_array_equal(idx, c4["idx2"])                       # two runs, bit for bit
    np.testing.assert_array_equal(val, c4["val2"])
    assert (val <= 1.0 + 1e-6).all() and (val >= 0).all()
    assert (np.diff(val, axis=1) <= 0).all()                             # sorted by score
    assert ((idx == -1) == (val == 0)).all() and (idx >= -1).all() and (idx < C4_TO).all()
    valid = idx >= 0
    assert (valid[:, :-1] | ~valid[:, 1:]).all()                         # empty cells trail
    srt = np.sort(np.where(valid, idx, -np.arange(1, C4_TOP + 1)[None, :]), axis=1)
    assert (np.diff(srt, axis=1) != 0).all()                             # no column twice in a row
    tie = (np.diff(val, axis=1) == 0) & valid[:, 1:]
    assert tie.sum() > 100_000                                           # (synthetic names repeat: most rows have exact ties)
    rr, kk = np.nonzero(tie & (idx[:, 1:] < idx[:, :-1]))
    print(f"config 4: {int(tie.sum())} tie cells, {len(rr)} with a descending column in rows {np.unique(rr).tolist()[:20]}")
    assert len(np.unique(rr)) <= C4_FROM // 1000
    a3, b3, n_col = c4_oracle["a3"], c4_oracle["b3"], c4_oracle["n_col"]
    for r, k in zip(rr.tolist(), kk.tolist()):
        dense = oracle_mod.cossim_dense(a3, b3, n_col, rows=(r, r + 1))[0]
        first, second = float(dense[idx[r, k]]), float(dense[idx[r, k + 1]])
        assert 0 < first - second < helpers.NEAR_TIE, \
            f"row {r} ranks {k}, {k + 1}: columns {idx[r, k]} > {idx[r, k + 1]} at equal score {val[r, k]!r}, oracle {first!r} / {second!r}"


def test_config_4_vectoriser_vs_oracle(c4, c4_oracle):
    """K1 / K2 on 1 125 000 strings: the device CSR of both lists against the numpy oracle's -- vocabulary size, indptr and column
    ids equal, values within 2e-7 (one fp32 rounding of the float64 tf-idf)"""
    for dev, key in ((c4["a"], "a3"), (c4["b"], "b3")):
        ep, ei, ev = c4_oracle[key]
        ap, ai, av, ncol = dev.download()
        assert ncol == c4_oracle["n_col"]
        np.testing.assert_array_equal(ap, ep)
        np.testing.assert_array_equal(ai, ei)
        assert np.abs(av.astype(np.float64) - ev).max() <= 2e-7
        del ap, ai, av


def c4_sample_rows():
    rows = np.sort(np.random.default_rng(4).choice(C4_FROM, 2048, replace=False))
    return np.unique(np.concatenate([rows, np.arange(64), np.arange(C4_FROM - 64, C4_FROM)])).astype(np.int64)


def test_config_4_sample_vs_the_oracle_chain(c4, c4_oracle, oracle_mod):
    """K1 -> K2 -> index -> lock-step K3 against the oracle's cosine top-10 on the ORACLE-built float64 matrices: 2 048 seeded rows plus
    the first and last 64 of the shard (chunk edges).  tests.helpers.assert_topn_parity's rule as everywhere: scores within 1e-5; an
    index may differ only between candidates the float64 oracle separates by less than 2e-6; at most 1 % of the checked rows may
    differ at all.  The cap is a condition: on the oracle alone, 8 of the 2 048 seeded rows (0.39 %) have two unequal neighbouring
    scores among ranks 1 .. 11 closer than 2e-6 -- the only place fp32 may reorder (exact float64 ties, which 1 717 of the rows have,
    are equal fixed-point sums in the kernel and ordered by column on both sides).  Measured on an MI355X: 8 of the 2 175 checked rows
    (0.37 %) differ in an index, all of them such near-ties; largest score error 1.2e-7; 15 rows have fewer than ten matches; 5 s."""
    rows = c4_sample_rows()
    assert 2048 <= len(rows) <= 2048 + 128 and rows[0] == 0 and rows[-1] == C4_FROM - 1
    a3, b3, n_col = c4_oracle["a3"], c4_oracle["b3"], c4_oracle["n_col"]
    parts = np.array_split(rows, 64)
    with cf.ThreadPoolExecutor(16) as ex:
        got = list(ex.map(lambda r: oracle_mod.cossim_topn(a3, b3, n_col, C4_TOP, 0.0, rows=np.ascontiguousarray(r)), parts))
    e_idx, e_val = np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])
    n_diff = int((c4["idx"][rows] != e_idx).any(axis=1).sum())
    print(f"config 4 sample: {n_diff} of {len(rows)} rows differ in an index; max |score - oracle| = "
          f"{np.abs(c4['val'][rows].astype(np.float64) - e_val).max():.3e}; rows with fewer than {C4_TOP} matches: "
          f"{int((e_idx[:, -1] < 0).sum())}")
    helpers.assert_topn_parity(c4["idx"][rows], c4["val"][rows], e_idx, e_val, oracle_mod, a3, b3, n_col, rows=rows)


# ---- 3. a slice of config 5 at its real width, natural panels ------------------------------------------------------------------------

C5_TO, C5_DIM, C5_FROM, C5_TOP = 500_000, 768, 2 * 2048 + 256, 10


@pytest.fixture(scope="module")
def c5(ctx):
    """rank 0's operands of bench.py's run_dense, 4 352 from-rows: with 4 GiB score panels and ld = 500 224 a panel holds 2 048 rows --
    two whole panels and a short third, byte offsets beyond 2^32 inside each, 7 816 block maxima per row, 24 k-chunks"""
    from polyfuzz_amd import _lib, pipeline
    assert [k for k in os.environ if k.startswith("PFZ_K5_")] == [], "this module tests the natural panel split"
    assert (((4 << 30) // (((C5_TO + 255) // 256 * 256) * 4)) // 128) * 128 == 2048
    b = np.random.default_rng(7).standard_normal((C5_TO, C5_DIM), dtype=np.float32)
    rng = np.random.default_rng(70)
    a = rng.standard_normal((C5_FROM, C5_DIM), dtype=np.float32)
    pick = rng.choice(C5_TO, C5_FROM, replace=False)
    a += 2.0 * b[pick]
    job = pipeline.DenseMatchJob(ctx, a, b, top_n=C5_TOP)
    idx, val = job.step().download()
    idx2, val2 = job.step().download()
    del job
    h_idx, h_val = _lib.dense_cossim_topn_host(ctx, a, b, C5_TOP, 0.0)
    out = {"a": a, "b": b, "pick": pick, "idx": idx, "val": val, "idx2": idx2, "val2": val2, "h_idx": h_idx, "h_val": h_val}
    yield out
    out.clear()
    del a, b
    gc.collect()


def test_config_5_slice_planted_match_and_repeatability(c5):
    """the planted match (cosine 2 / sqrt 5 = 0.89; the best of 500 000 random columns stays below 0.2) is rank 1 of ALL 4 352 rows; a
    second step() and the one-shot host call return the same cells, bit for bit"""
    idx, val = c5["idx"], c5["val"]
    assert idx.shape == val.shape == (C5_FROM, C5_TOP)
    np.testing.assert_array_equal(idx[:, 0], c5["pick"])
    assert (np.abs(val[:, 0] - 2 / np.sqrt(5)) < 0.05).all() and (val[:, 1] < 0.25).all()
    assert (np.diff(val, axis=1) <= 0).all() and (idx >= 0).all() and (idx < C5_TO).all()
    np.testing.assert_array_equal(idx, c5["idx2"])
    np.testing.assert_array_equal(val, c5["val2"])
    np.testing.assert_array_equal(idx, c5["h_idx"])
    np.testing.assert_array_equal(val, c5["h_val"])


def c5_sample_rows():
    rows = np.random.default_rng(5).choice(C5_FROM, 256, replace=False)
    seams = np.concatenate([np.arange(2040, 2056), np.arange(4088, 4104), np.arange(C5_FROM - 8, C5_FROM)])
    return np.unique(np.concatenate([rows, seams])).astype(np.int64)


def test_config_5_slice_sample_vs_oracle(c5, oracle_mod):
    """256 seeded rows, the rows either side of both panel seams (2 040 .. 2 055, 4 088 .. 4 103) and the last 8, against the float64
    oracle (oracle/dense.py) over all 500 000 to-vectors: scores within 1e-5; an index may differ only between float64 near-ties
    (< 4e-6, the rule of tests/test_dense_gpu.py), in at most max(1, rows // 100) rows.  Measured on an MI355X: 0 of the 292 checked
    rows differ, largest score error 1.1e-6; 2 s for the oracle (3 s for the module's operands and device runs)."""
    rows = c5_sample_rows()
    assert 256 + 8 <= len(rows) <= 256 + 40 and {2047, 2048, 4095, 4096, C5_FROM - 1} <= set(rows.tolist())
    a, b = c5["a"], c5["b"]
    e_idx, e_val = oracle_mod.dense_cossim_topn(a[rows], b, C5_TOP, 0.0, chunk_rows=128)
    idx, val = c5["idx"][rows], c5["val"][rows]
    bad = np.nonzero((idx != e_idx).any(axis=1))[0]
    print(f"config 5 slice: {len(bad)} of {len(rows)} rows differ in an index; max |score - oracle| = "
          f"{np.abs(val.astype(np.float64) - e_val).max():.3e}")
    np.testing.assert_allclose(val, e_val, rtol=0, atol=1e-5)
    for i in bad:                       # only float64 near-ties may swap
        for r in range(C5_TOP):
            if idx[i, r] != e_idx[i, r]:
                s = float(oracle_mod.dense_cossim(a[rows[i]:rows[i] + 1], b[idx[i, r]:idx[i, r] + 1])[0, 0]) if idx[i, r] >= 0 else 0.0
                assert abs(s - e_val[i, r]) < 4e-6, (int(rows[i]), r, idx[i], e_idx[i])
    assert len(bad) <= max(1, len(rows) // 100)
