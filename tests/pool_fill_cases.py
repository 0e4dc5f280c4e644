"""The batteries of tests/test_pool_fill_gpu.py: one function per group of entry points that runs every listed form once and returns
what it computed, and one per group that holds such a run to the oracle the entry's own tests use.

A battery is run under Context.pool_fill(ZERO), then ONE64, then ONE32 (every block the allocator hands out pre-filled with the
mode's word), and the runs are compared on their bytes: a difference means a kernel or a host path read device memory nobody
wrote.  So a run
  * uploads its own DeviceStrings / DeviceDense / DeviceCSR / DeviceIndex and builds its own plans and handles -- a plan cached on a
    handle from an earlier fill would hide the plan's own allocations;
  * records results only (indices, scores, row pointers, labels, pair totals, exported vocabularies), and of the counters only the
    totals the header documents as exact (the hits of a join, the pairs and components of a components call);
  * asserts, through the counter or profiling scope the form's own tests use, that a form it forces with a knob did run.
The lists and references are the existing case modules'."""
import contextlib
import functools
import os

import numpy as np

from tests import dense_join_cases as DJ
from tests import sparse_join_cases as SJ

ZERO, ONE64, ONE32 = 1, 2, 3
FILLS = (("ZERO", ZERO), ("ONE64", ONE64), ("ONE32", ONE32))


@contextlib.contextmanager
def knobs(**env):
    """the environment knobs of a forced form, for the calls inside; None removes one"""
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@contextlib.contextmanager
def launches(ctx, *names):
    """with launches(ctx, "k4_indel_general") as box: ...  ->  box[name] = launches of that profiling scope inside"""
    box = {}
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        yield box
        ctx.sync()
        for n in names:
            box[n] = ctx.prof_get(n)[1]
    finally:
        ctx.prof_enable(False)


class Run(dict):
    """name -> array of one battery run, in the order recorded; .forms: name -> the counter that shows a forced form ran"""

    def __init__(self):
        super().__init__()
        self.forms = {}

    def put(self, name, *arrays):
        for k, a in enumerate(arrays):
            key = name if len(arrays) == 1 else f"{name}[{k}]"
            assert key not in self, key
            self[key] = np.ascontiguousarray(a)

    def get_all(self, name):
        out, k = [], 0
        while f"{name}[{k}]" in self:
            out.append(self[f"{name}[{k}]"])
            k += 1
        return out if out else [self[name]]


def differences(run, base):
    """the items of `run` whose bytes, dtype or shape differ from `base`'s (NaN and -0.0 count: the comparison is on bytes)"""
    assert list(run) == list(base), (sorted(set(run) ^ set(base)))
    return [k for k in base if run[k].dtype != base[k].dtype or run[k].shape != base[k].shape or run[k].tobytes() != base[k].tobytes()]


# ==== tfidf: K1, K2, K3, K15 =========================================================================================================

DOC_LONG = "ab" * 3000                       # 5 998 trigrams: beyond the 4 096 of one pass
WIDE_RANGE = (3, 6)


@functools.lru_cache(maxsize=None)
def tfidf_lists():
    rng = np.random.default_rng(52)
    names = list(SJ.lists("names2600")[0])
    doc_mid = "".join(chr(97 + int(c)) for c in rng.integers(0, 26, 102))      # 100 trigrams: the 65 .. 128 form
    docs = names[:300] + [DOC_LONG, doc_mid]
    from polyfuzz_amd import synth
    two = (synth.company_names(203, seed=521), synth.company_names(180, seed=522))
    return names, docs, two


def _csr(run, name, dev):
    indptr, indices, data, n_cols = dev.download()
    run.put(name, indptr, indices, data, np.array([n_cols], np.int64))


def _join_items(run, name, got):
    row_ptr, idx, sim, counts = got
    run.put(name, row_ptr, idx, sim, np.array([counts["pairs"]], np.int64))


def run_tfidf(ctx):
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models._tfidf import _SPLIT_EVENT
    run = Run()
    names, docs, (two_from, two_to) = tfidf_lists()
    p33 = _lib.TfidfParams(3, 3, 1, 1)
    # K1 / K2: a document beyond one pass and one of the two-keys-per-lane form, among 300 names
    d = _lib.DeviceStrings.upload(ctx, docs)
    vec = _lib.DeviceTfidf.fit(ctx, p33, d, None)
    run.put("docs.export", *vec.export())
    _csr(run, "docs.csr", vec.transform(d))
    # K1 / K2: two lists at n-gram range (3, 6) -- codes beyond 32 bits: the sorted vocabulary and its 64-bit sort
    f, t = _lib.DeviceStrings.upload(ctx, two_from), _lib.DeviceStrings.upload(ctx, two_to)
    wide = _lib.DeviceTfidf.fit(ctx, _lib.TfidfParams(WIDE_RANGE[0], WIDE_RANGE[1], 1, 1), t, f)
    run.forms["sorted_vocabulary.code_bits"] = wide.info()["code_bits"]
    assert run.forms["sorted_vocabulary.code_bits"] > 32
    run.put("two_list.export", *wide.export())
    _csr(run, "two_list.from", wide.transform(f))
    _csr(run, "two_list.to", wide.transform(t))
    # names2600, index blocks of 1024: three blocks, the last ragged, two empty rows
    s = _lib.DeviceStrings.upload(ctx, names)
    a = _lib.DeviceTfidf.fit(ctx, p33, s, None).transform(s)
    _csr(run, "names2600.csr", a)
    with knobs(PFZ_K3_BLOCK="1024", PFZ_K3_SYM=None, PFZ_K3_LOCKSTEP=None):
        index = _lib.DeviceIndex.build(ctx, a)
        assert (index.info()["block_cols"], index.info()["n_blocks"]) == (1024, 3)
        run.put("k3.row_major", *_lib.cossim_topn(ctx, index, a, 5, 0.0, exclude_diag=True).download())
        ends = [1024, len(names)]                       # one cut on a block boundary
        out = _lib.cossim_topn_ranges(ctx, index, a, 5, 0.0, True, ends, _SPLIT_EVENT)
        for i in range(len(ends)):
            ctx.event_wait(_SPLIT_EVENT + i)
        run.put("k3.ranges", *out.download())
        assert index.symmetric_launches()[0] == 0
        # K15 on the same index: room for every hit, and the repeat after a first call with room for one
        _join_items(run, "k15.join", _lib.sparse_join(ctx, index, a, 0.8, self_join=True, capacity=1 << 16))
        _join_items(run, "k15.join_repeat", _lib.sparse_join(ctx, index, a, 0.8, self_join=True, capacity=1))
        pairs = _lib.sparse_join_dev(ctx, index, a, 0.8, self_join=True, capacity_hint=1)
        run.put("k15.join_dev_repeat", *pairs.download())
        pairs = _lib.sparse_join_dev(ctx, index, a, 0.8, self_join=True)
        run.put("k15.join_dev", *pairs.download())
        label, n_pairs, n_comp = _lib.sparse_components(ctx, index, a, 0.8)
        run.put("k15.components", label, np.array([n_pairs, n_comp], np.int64))
    # the symmetric and the lock-step form take 2048-row blocks and at least two of them: the same list at the default block size
    with knobs(PFZ_K3_BLOCK=None, PFZ_K3_SYM="1", PFZ_K3_LOCKSTEP="0"):
        index = _lib.DeviceIndex.build(ctx, a)
        assert (index.info()["block_cols"], index.info()["n_blocks"]) == (2048, 2)
        run.put("k3.symmetric", *_lib.cossim_topn(ctx, index, a, 5, 0.0, exclude_diag=True).download())
        run.forms["symmetric_launches"] = index.symmetric_launches()
        assert run.forms["symmetric_launches"] == (1, len(names))
    with knobs(PFZ_K3_BLOCK=None, PFZ_K3_SYM="0", PFZ_K3_LOCKSTEP="1"):
        index = _lib.DeviceIndex.build(ctx, a)
        with launches(ctx, "k3_lockstep", "k3_cossim_topn") as box:
            run.put("k3.lockstep", *_lib.cossim_topn(ctx, index, a, 5, 0.0, exclude_diag=True).download())
        run.forms["k3_lockstep"] = box["k3_lockstep"]
        assert box["k3_lockstep"] == box["k3_cossim_topn"] == 1 and index.symmetric_launches()[0] == 0
    return run


def _check_csr(got, exp, n_col):
    """tests/test_vectorize_gpu.py's rule: structure exact, values within 2e-7"""
    indptr, indices, data, ncols = got
    assert int(ncols[0]) == n_col
    np.testing.assert_array_equal(indptr, exp[0])
    np.testing.assert_array_equal(indices, exp[1])
    np.testing.assert_allclose(data, exp[2], rtol=0, atol=2e-7)


def _check_export(got, o):
    ngrams, idf, df = got
    assert ["".join(chr(c) for c in row if c) for row in ngrams.tolist()] == o.vocabulary
    np.testing.assert_array_equal(df, o.df)
    np.testing.assert_allclose(idf, o.idf, rtol=1e-15)


def check_tfidf(run, oracle):
    from tests.helpers import assert_topn_parity
    names, docs, (two_from, two_to) = tfidf_lists()
    o = oracle.TfidfOracle().fit(docs)
    exp = o.transform(docs)
    per_row = np.diff(exp[0])
    assert 65 <= per_row[-1] <= 128 and len(DOC_LONG) - 2 > 4096
    _check_export(run.get_all("docs.export"), o)
    _check_csr(run.get_all("docs.csr"), exp, len(o.vocabulary))
    o = oracle.TfidfOracle(n_gram_range=WIDE_RANGE).fit(list(two_to) + list(two_from))
    _check_export(run.get_all("two_list.export"), o)
    _check_csr(run.get_all("two_list.from"), o.transform(list(two_from)), len(o.vocabulary))
    _check_csr(run.get_all("two_list.to"), o.transform(list(two_to)), len(o.vocabulary))
    o = oracle.TfidfOracle().fit(names)
    a3, n_col = o.transform(names), len(o.vocabulary)
    assert (np.diff(a3[0]) == 0).sum() >= 2                              # the strings too short for a trigram: empty rows
    _check_csr(run.get_all("names2600.csr"), a3, n_col)
    e_idx, e_val = oracle.cossim_topn(a3, a3, n_col, 5, 0.0, exclude_diag=True)
    for form in ("row_major", "ranges", "symmetric", "lockstep"):
        idx, val = run.get_all("k3." + form)
        assert_topn_parity(idx, val, e_idx, e_val, oracle, a3, a3, n_col, exclude_diag=True)
    # K15 against the float64 oracle as tests/test_sparse_join_gpu.py holds it: no pair of this list lies within 1e-5 of 0.8
    hits, band = SJ.oracle_counts("names2600", 0.8)
    assert (hits, band) == SJ.ORACLE_HITS["names2600"][0.8] and band == 0
    cos = SJ.oracle_pairs("names2600").tocoo()
    must = cos.data >= 0.8
    want = sorted(zip(cos.row[must].tolist(), cos.col[must].tolist()))
    row_ptr, idx, sim, total = run.get_all("k15.join")
    rows, cols = SJ.csr_pairs(row_ptr, idx)
    assert int(total[0]) == hits == len(idx) and list(zip(rows.tolist(), cols.tolist())) == want
    exact = np.asarray(SJ.oracle_pairs("names2600")[rows, cols]).ravel()
    assert np.abs(sim.astype(np.float64) - exact).max() <= SJ.BAND
    for other in ("k15.join_repeat", "k15.join_dev", "k15.join_dev_repeat"):      # the same bytes whatever the capacity, wherever the result is left
        for g, w in zip(run.get_all(other), (row_ptr, idx, sim)):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), other
    label, counts = run.get_all("k15.components")
    want_label = SJ.union_find_labels(len(names), rows, cols)
    assert label.tobytes() == want_label.tobytes() and counts.tolist() == [hits, len(np.unique(want_label))]


# ==== edit: K4, K8, K9, K11, K12, K13 ==================================================================================================

COMPONENTS_N = 100           # the components calls take the first 100 to-strings as their list (the reference is a 100 x 100 table)


@functools.lru_cache(maxsize=None)
def edit_lists(alpha):
    """tests/test_join_gpu.py's ~33 from-strings of lengths 0, 1, 31 .. 33, 63 .. 65 and 130 against its 300 to-strings; "wide": over
    300 code points, so the symbols are 16-bit"""
    from tests.test_join_gpu import _class_lists
    fl, tl = _class_lists(alpha)
    assert len({c for s in tl for c in s}) > 255 if alpha == "wide" else len({c for s in tl for c in s}) == 2
    return tuple(fl), tuple(tl)


def _run_edit_lists(ctx, run, alpha):
    from polyfuzz_amd import _lib
    fl, tl = edit_lists(alpha)
    f, t = _lib.DeviceStrings.upload(ctx, list(fl)), _lib.DeviceStrings.upload(ctx, list(tl))
    c = _lib.DeviceStrings.upload(ctx, list(tl[:COMPONENTS_N]))
    room = len(fl) * len(tl)
    tag = alpha + "."
    # K4
    run.put(tag + "indel_argmax", *_lib.indel_argmax(ctx, f, t))
    run.put(tag + "indel_topn", *_lib.indel_topn(ctx, f, t, 3))
    run.put(tag + "indel_matrix", _lib.indel_matrix(ctx, f, t))
    with knobs(PFZ_K4_FORCE_GENERAL="1"), launches(ctx, "k4_indel", "k4_general_rows") as box:
        run.put(tag + "general.indel_argmax", *_lib.indel_argmax(ctx, f, t))
        run.put(tag + "general.indel_topn", *_lib.indel_topn(ctx, f, t, 3))
        run.put(tag + "general.indel_matrix", _lib.indel_matrix(ctx, f, t))
    run.forms[tag + "k4_general_rows"] = box["k4_general_rows"]
    with_chars = sum(1 for s in fl if s)
    assert 3 * with_chars <= box["k4_general_rows"] <= 3 * len(fl) and box["k4_indel"] == 3      # every from-row of the three calls
    # K8
    for name in ("jaro", "jaro_winkler"):
        run.put(tag + name + "_argmax", *_lib.jaro_argmax(ctx, f, t, name))
        run.put(tag + name + "_matrix", _lib.jaro_matrix(ctx, f, t, name))
    # K9
    for name in ("levenshtein", "osa"):
        run.put(tag + name + "_argmax", *_lib.lev_argmax(ctx, f, t, name))
        run.put(tag + name + "_topn", *_lib.lev_topn(ctx, f, t, name, 3))
        run.put(tag + name + "_matrix", _lib.lev_matrix(ctx, f, t, name))
    # K11, K12, K13: room for every pair, and the repeat after a first call with room for one; the components of the to-list's first 100
    run.put(tag + "lev_join", *_lib.lev_join(ctx, f, t, "levenshtein", 0.8, capacity=room))
    run.put(tag + "lev_join_repeat", *_lib.lev_join(ctx, f, t, "levenshtein", 0.8, capacity=1))
    label, n_pairs, n_comp = _lib.lev_components(ctx, c, "levenshtein", 0.8)
    run.put(tag + "lev_components", label, np.array([n_pairs, n_comp], np.int64))
    run.put(tag + "indel_join", *_lib.indel_join(ctx, f, t, 0.8, capacity=room))
    run.put(tag + "indel_join_repeat", *_lib.indel_join(ctx, f, t, 0.8, capacity=1))
    label, n_pairs, n_comp = _lib.indel_components(ctx, c, 0.8)
    run.put(tag + "indel_components", label, np.array([n_pairs, n_comp], np.int64))


def _second_row_lists(ctx):
    """tests/second_row_cases.py's K4 lists: more from-strings than the general launch has workgroups, so that a workgroup walks a
    second row on its own match table"""
    from tests import second_row_cases as SR
    return SR.k4_lists(ctx.info()["n_cu"])


def run_edit(ctx):
    from polyfuzz_amd import _lib
    run = Run()
    _run_edit_lists(ctx, run, "ab")
    _run_edit_lists(ctx, run, "wide")
    fl, tl = _second_row_lists(ctx)
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    with knobs(PFZ_K4_FORCE_GENERAL="1"), launches(ctx, "k4_indel_general", "k4_general_rows") as box:
        run.put("second_row.indel_argmax", *_lib.indel_argmax(ctx, f, t))
    run.forms["second_row.k4_general_rows"] = box["k4_general_rows"]
    from tests import second_row_cases as SR
    assert box["k4_indel_general"] == 1 and box["k4_general_rows"] > SR.K4_GRID_PER_CU * ctx.info()["n_cu"]      # one launch, rows beyond its grid
    run.n_cu = ctx.info()["n_cu"]
    return run


def _equal(got, want, what):
    got, want = list(got), list(want)
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        w = np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=f"{what}[{k}]")


def _join_want(sim, value, thr, self_join=False):
    """(row_ptr, idx, value, sim) of the pairs with sim >= thr, row-major (tests/test_join_gpu.py's _want)"""
    keep = sim >= thr
    if self_join:
        keep &= np.triu(np.ones(keep.shape, bool), 1)
    i, j = np.nonzero(keep)
    row_ptr = np.zeros(sim.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(i, minlength=sim.shape[0]), out=row_ptr[1:])
    return row_ptr, j.astype(np.int32), value[i, j].astype(np.int32), sim[i, j]


def _components_want(sim):
    i, j = np.nonzero((sim >= 0.8) & np.triu(np.ones(sim.shape, bool), 1))
    label = DJ.union_find_labels(sim.shape[0], i, j)
    return label, np.array([len(i), len(np.unique(label))], np.int64)


def _check_edit_lists(run, oracle, alpha):
    from tests import indel_oracle, lev_oracle
    from tests.test_edit_topn_gpu import expected_topn
    fl, tl = [list(x) for x in edit_lists(alpha)]
    tag = alpha + "."
    # K4 against oracle/indel.c, every comparison exact
    e_idx, e_score, e_mat = oracle.indel_argmax(fl, tl, want_matrix=True)
    for form in ("", "general."):
        _equal(run.get_all(tag + form + "indel_argmax"), (e_idx, e_score), tag + form + "indel_argmax")
        _equal(run.get_all(tag + form + "indel_topn"), expected_topn(e_mat, 3), tag + form + "indel_topn")
        _equal(run.get_all(tag + form + "indel_matrix"), (e_mat,), tag + form + "indel_matrix")
    # K8 against oracle/jaro.c
    for name in ("jaro", "jaro_winkler"):
        mat = oracle.jaro_matrix(fl, tl, name)
        _equal(run.get_all(tag + name + "_matrix"), (mat,), tag + name + "_matrix")
        _equal(run.get_all(tag + name + "_argmax"), lev_oracle.argmax(mat), tag + name + "_argmax")
    # K9, K11, K12 against the Wagner-Fischer table
    for name in ("levenshtein", "osa"):
        d = lev_oracle.matrix(fl, tl, name)
        sim = lev_oracle.sim_matrix(fl, tl, d)
        _equal(run.get_all(tag + name + "_matrix"), (d,), tag + name + "_matrix")
        _equal(run.get_all(tag + name + "_argmax"), lev_oracle.argmax(sim), tag + name + "_argmax")
        _equal(run.get_all(tag + name + "_topn"), expected_topn(sim, 3), tag + name + "_topn")
        if name == "levenshtein":
            want = _join_want(sim, d, 0.8)
            assert len(want[1]) > 1                                     # (capacity 1 is too small: the repeat ran)
            _equal(run.get_all(tag + "lev_join"), want, tag + "lev_join")
            _equal(run.get_all(tag + "lev_join_repeat"), want, tag + "lev_join_repeat")
    cl = tl[:COMPONENTS_N]
    d = lev_oracle.matrix(cl, cl, "levenshtein")
    _equal(run.get_all(tag + "lev_components"), _components_want(lev_oracle.sim_matrix(cl, cl, d)), tag + "lev_components")
    # K13 against the LCS table
    lcs = indel_oracle.lcs_matrix(fl, tl)
    sim = indel_oracle.sim_matrix(fl, tl, lcs)
    want = _join_want(sim, indel_oracle.distance(lcs, lev_oracle.lengths(fl)[:, None], lev_oracle.lengths(tl)[None, :]), 0.8)
    assert len(want[1]) > 1
    _equal(run.get_all(tag + "indel_join"), want, tag + "indel_join")
    _equal(run.get_all(tag + "indel_join_repeat"), want, tag + "indel_join_repeat")
    sim = indel_oracle.sim_matrix(cl, cl, indel_oracle.lcs_matrix(cl, cl))
    _equal(run.get_all(tag + "indel_components"), _components_want(sim), tag + "indel_components")


def check_edit(run, oracle):
    from tests import second_row_cases as SR
    _check_edit_lists(run, oracle, "ab")
    _check_edit_lists(run, oracle, "wide")
    fl, tl = SR.k4_lists(run.n_cu)
    _equal(run.get_all("second_row.indel_argmax"), oracle.indel_argmax(fl, tl), "second_row.indel_argmax")


# ==== fuzz: K7 =======================================================================================================================

FUZZ_MODES = ("WRatio", "partial_ratio", "token_set_ratio", "token_ratio", "partial_token_sort_ratio", "partial_token_set_ratio",
              "partial_token_ratio")


@functools.lru_cache(maxsize=None)
def fuzz_lists():
    """name -> (from, to).  "": the lists of tests/test_fuzz_gpu.py's test_modes_bit_exact_vs_oracle.  "long_from.": the 400-character
    and the 40-token from-string of its test_strings_beyond_the_fast_kernel (the general kernel's rows) against short to-strings;
    "long_to.": short from-strings against that test's to-string of 35 tokens (a general to-string) and its 295 characters.  The
    long strings do not meet each other: one such pair alone takes partial_ratio seven seconds.  "hand_over.": 150 x 3 000 of
    config 3's lists"""
    from polyfuzz_amd import datasets
    from tests.test_fuzz_gpu import _lists
    fl, tl = _lists(3, 70, 150)
    fl += ["this is a test", "this is a word", "fuzzy was a bear", "", "a", "mets mets mets new"]
    tl += ["this is a new test!!!", "THIS IS A WORD", "fuzzy fuzzy was a bear", "", "this is a test!", "new mets"]
    rng = np.random.default_rng(5)
    words = ["alpha", "beta", "gamma", "delta", "of", "the", "inc", "llc", "new", "york", "mets", "braves"]
    long_from = " ".join(rng.choice(words, size=70))
    small = ["york new mets", "t1 t2 t3", "", "alpha beta of the mets", "t7 t8 gamma delta inc", "braves llc new york"]
    long_fl = [long_from[:400], " ".join(f"t{i}" for i in range(40)), "new york mets", ""]
    long_tl = [" ".join(f"t{i}" for i in range(3, 38)), long_from[5:300]] + small
    assert max(map(len, long_fl)) > 256 and max(len(set(s.split())) for s in long_fl) == 40 and max(len(set(s.split())) for s in long_tl) > 32
    hand_from, hand_to = datasets.c3_lists(3000)
    return {"": (tuple(fl), tuple(tl)), "long_from.": (tuple(long_fl), tuple(small)),
            "long_to.": (("new york mets", "", "t3 t4 t9 gamma", "of the alpha beta inc"), tuple(long_tl)),
            "hand_over.": (tuple(hand_from[:150]), tuple(hand_to))}


def run_fuzz(ctx):
    from polyfuzz_amd import _lib
    run = Run()
    lists = fuzz_lists()
    for tag, parts in (("", None), ("parts3.", "3")):                 # parts3: the to-groups of a from-string shared by three workgroups
        with knobs(PFZ_K7_PARTS=parts, PFZ_K7_HAND_BATCHES=None):
            for name in ("", "long_from.", "long_to."):
                f, t = [_lib.DeviceStrings.upload(ctx, list(x)) for x in lists[name]]
                if name == "long_to.":
                    run.forms[tag + "n_general_strings"] = _lib.fuzz_plan_info(ctx, t)["n_general_strings"]
                    assert run.forms[tag + "n_general_strings"] == 1
                for mode in FUZZ_MODES:
                    run.put(tag + name + mode, *_lib.fuzz_extract_one(ctx, f, t, mode))
    with knobs(PFZ_K7_PARTS="1", PFZ_K7_HAND_BATCHES="1"):            # the heavy rows hand their later to-groups to a second launch
        f, t = [_lib.DeviceStrings.upload(ctx, list(x)) for x in lists["hand_over."]]
        run.put("hand_over.WRatio", *_lib.fuzz_extract_one(ctx, f, t, "WRatio"))
    return run


def check_fuzz(run, oracle):
    import concurrent.futures as cf
    lists = {k: [list(x) for x in v] for k, v in fuzz_lists().items()}
    for name in ("", "long_from.", "long_to."):
        fl, tl = lists[name]
        for mode in FUZZ_MODES:
            want = oracle.fuzz_extract_one(fl, tl, mode)
            _equal(run.get_all(name + mode), want, name + mode)
            _equal(run.get_all("parts3." + name + mode), want, "parts3." + name + mode)
    hand_from, hand_to = lists["hand_over."]
    cuts = list(range(0, len(hand_from), 10))          # (the C oracle lets go of the interpreter lock: ten rows per task)
    with cf.ThreadPoolExecutor(8) as ex:
        parts = list(ex.map(lambda b: oracle.fuzz_extract_one(hand_from[b:b + 10], hand_to, "WRatio"), cuts))
    want = [np.concatenate([p[k] for p in parts]) for k in range(2)]
    _equal(run.get_all("hand_over.WRatio"), want, "hand_over.WRatio")


# ==== dense: K5, K14, K6 =============================================================================================================

DENSE_CASES = ("257x40", DJ.TWO_LIST_CASE)
DENSE_FORMS = ("float32", "float16", "bfloat16", "int8", "binary")
PANEL_ROWS = 64
RESCORE_M = 20                  # candidates per row of the two rescored searches: top 5 x 4


def _dense_upload(ctx, x, form):
    from polyfuzz_amd import _lib
    if form == "binary":
        return _lib.DeviceDense.upload_bits(ctx, x)
    return _lib.DeviceDense.upload_as(ctx, x, form)


@functools.lru_cache(maxsize=None)
def k6_inputs():
    rng = np.random.default_rng(6)
    v = rng.random(10_000)
    on = rng.random(len(v)) < 1 / 16
    v[on] = rng.choice(np.linspace(0, 1, 101), int(on.sum()))          # values ON thresholds
    v[rng.random(len(v)) < 0.01] = np.nan
    v.setflags(write=False)
    return v, np.linspace(0.0, 1.0, 101)


def run_dense(ctx):
    from polyfuzz_amd import _lib
    run = Run()
    for case in DENSE_CASES:
        x, y = DJ.lists(case)
        self_match = y is None
        for tag, env in (("", {"PFZ_K5_PANEL_ROWS": None}), ("panels.", {"PFZ_K5_PANEL_ROWS": str(PANEL_ROWS)})):
            with knobs(**env), launches(ctx, "k5_gemm_panel") as box:
                for form in DENSE_FORMS:
                    f = _dense_upload(ctx, x, form)
                    t = f if self_match else _dense_upload(ctx, y, form)
                    run.put(f"{case}.{tag}{form}", *_lib.dense_topn(ctx, f, t, 5, 0.0, exclude_diag=self_match).download())
            run.forms[f"{case}.{tag}k5_gemm_panel"] = box["k5_gemm_panel"]             # one launch per panel of from-rows
            assert box["k5_gemm_panel"] >= 2 * len(DENSE_FORMS) if tag else box["k5_gemm_panel"] == len(DENSE_FORMS), (case, tag, box)
        # exact fp32 scores of bfloat16 candidates, and float32 from-vectors against the int8 to-side itself
        f32 = _lib.DeviceDense.upload(ctx, x)
        t32 = f32 if self_match else _lib.DeviceDense.upload(ctx, y)
        f16 = _dense_upload(ctx, x, "bfloat16")
        t16 = f16 if self_match else _dense_upload(ctx, y, "bfloat16")
        cand = _lib.DeviceTopN.alloc(ctx, len(x), RESCORE_M)
        out = _lib.dense_topn_rescored(ctx, f16, t16, f32, t32, 5, 0.0, 4, exclude_diag=self_match, candidates=cand)
        run.put(f"{case}.rescore.candidates", cand.download()[0])
        run.put(f"{case}.rescore", *out.download())
        f8 = _dense_upload(ctx, x, "int8")
        t8 = f8 if self_match else _dense_upload(ctx, y, "int8")
        cand = _lib.DeviceTopN.alloc(ctx, len(x), RESCORE_M)
        out = _lib.dense_topn_rescored(ctx, f8, t8, f32, t8, 5, 0.0, 4, exclude_diag=self_match, candidates=cand)
        run.put(f"{case}.mixed.candidates", cand.download()[0])
        run.put(f"{case}.mixed", *out.download())
        # K14: one pass with room for every hit, and the repeat after a first call with room for one
        to = None if self_match else t32
        _join_items(run, f"{case}.join", _lib.dense_join(ctx, f32, to, 0.8, capacity=len(x) * (len(x) if self_match else len(y))))
        _join_items(run, f"{case}.join_repeat", _lib.dense_join(ctx, f32, to, 0.8, capacity=1))
        if self_match:
            label, n_pairs, n_comp = _lib.dense_components(ctx, f32, 0.8)
            run.put(f"{case}.components", label, np.array([n_pairs, n_comp], np.int64))
            # K6 on the self-match's best choices (rank 0 of the fp32 top-5 is what it reads)
            top = _lib.dense_topn(ctx, f32, f32, 5, 0.0, exclude_diag=True)
            cluster, key, info = _lib.linkage_top1(ctx, top, 0.8)
            run.put("linkage_top1", cluster, key, np.array([info["first_row"], info["clusters"]], np.int64))
    sims, thr = k6_inputs()
    run.put("pr_curve", *_lib.pr_curve(ctx, sims, thr))
    return run


def _rounded16(a, form):
    from tests.test_dense16_gpu import _rounded
    return _rounded(a, form)[1]


def _as_float64(x, form):
    """the values the device holds of float32 rows uploaded as `form`, as float64 (tests/test_dense16_gpu.py, test_dense8_gpu.py)"""
    from tests.test_dense8_gpu import _quantize
    if form == "float32":
        return x.astype(np.float64)
    if form == "int8":
        return _quantize(x)[0].astype(np.float64)
    return _rounded16(x, form)


def check_dense(run, oracle):
    import math
    from tests.helpers import assert_dense_topn
    from tests.test_dense8_gpu import _quantize
    from tests.test_dense_rescore_gpu import _restricted
    from tests.test_hamming_cpu import pack, scores, topn
    from tests.test_k6_core_cpu import check_against_walk, kept_oracle, pr_error_bound
    from tests.test_mixed_rescore_gpu import _dense8
    from polyfuzz_amd.linkage import greedy_assign
    for case in DENSE_CASES:
        x, y = DJ.lists(case)
        self_match = y is None
        yy = x if self_match else y
        for form in DENSE_FORMS:
            for tag in ("", "panels."):
                idx, val = run.get_all(f"{case}.{tag}{form}")
                if form == "binary":                  # Hamming scores are exact functions of an integer: bit for bit
                    e_idx, e_val = topn(scores(pack(x), pack(yy), x.shape[1]), 5, 0.0, exclude_diag=self_match)
                    assert idx.tobytes() == e_idx.tobytes() and val.tobytes() == e_val.tobytes(), (case, tag, form)
                    continue
                wa, wb = _as_float64(x, form), _as_float64(yy, form)
                e_idx, e_val = oracle.dense_cossim_topn(wa, wb, 5, 0.0, exclude_diag=self_match)
                assert_dense_topn(idx, val, e_idx, e_val, oracle.dense_cossim(wa, wb))
        dense = oracle.dense_cossim(x.astype(np.float64), yy.astype(np.float64))
        cand = run[f"{case}.rescore.candidates"]
        assert cand.shape == (len(x), RESCORE_M) and (cand >= 0).all()
        idx, val = run.get_all(f"{case}.rescore")
        assert_dense_topn(idx, val, *_restricted(dense, cand, 5, 0.0), dense)
        mixed = _dense8(x, _quantize(yy)[0])
        cand = run[f"{case}.mixed.candidates"]
        idx, val = run.get_all(f"{case}.mixed")
        assert_dense_topn(idx, val, *_restricted(mixed, cand, 5, 0.0), mixed)
        # K14 against the float64 cosines, as tests/test_dense_join_gpu.py holds it: no pair of these cases lies within 1e-5 of 0.8
        hits, band = DJ.oracle_counts(case, 0.8)
        assert (hits, band) == DJ.ORACLE_HITS[case][0.8] and band == 0
        cos = DJ.cosines(case)
        row_ptr, cols, sim, total = run.get_all(f"{case}.join")
        rows, cols = DJ.csr_pairs(row_ptr, cols)
        found = np.zeros(cos.shape, bool)
        found[rows, cols] = True
        assert int(total[0]) == hits == len(rows) and np.array_equal(found, cos >= 0.8)
        assert np.abs(sim.astype(np.float64) - cos[rows, cols]).max() <= DJ.BAND
        for g, w in zip(run.get_all(f"{case}.join_repeat"), run.get_all(f"{case}.join")):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), case
        if self_match:
            label, counts = run.get_all(f"{case}.components")
            want = DJ.union_find_labels(len(x), rows, cols)
            assert label.tobytes() == want.tobytes() and counts.tolist() == [hits, DJ.ORACLE_COMPONENTS[case][0.8]]
            g, v = run[f"{case}.float32[0]"][:, 0], run[f"{case}.float32[1]"][:, 0]
            cluster, key, info = run.get_all("linkage_top1")
            kept = kept_oracle(g, v, len(x), 0.8)
            assert kept.sum() > 100
            check_against_walk(g, kept, cluster, key, {"first_row": int(info[0]), "clusters": int(info[1]), "rounds": 1}, len(x), greedy_assign)
    # K6's curve: counts == numpy's, sums within the fixed point's bound of the exact sum (tests/test_k6_gpu.py)
    sims, thr = k6_inputs()
    count, ssum = run.get_all("pr_curve")
    v = np.sort(sims[~np.isnan(sims)])[::-1]
    np.testing.assert_array_equal(count, (v[:, None] >= thr[None, :]).sum(0))
    step, _ = pr_error_bound(len(sims), float(np.abs(v).max()))
    for k in range(len(thr)):
        exact = math.fsum(v[:int(count[k])].tolist())
        assert abs(float(ssum[k]) - exact) <= int(count[k]) * step + abs(exact) * 2.0 ** -52, k


# ==== blocked: K10, K16, K17 =========================================================================================================

FIVE = ("ratio", "levenshtein", "osa", "jaro", "jaro_winkler")


@functools.lru_cache(maxsize=None)
def blocked_cases():
    """name -> (from-list, to-list or None, {scorer: oracle matrix}): tests/blocked_threshold_cases.py's small_two_lists, small_self
    and the hub of 80 characters with its 2 S + 40 partners (three slices of the key walk, the general kernel)"""
    from polyfuzz_amd import _lib
    from tests import blocked_threshold_cases as BT
    from tests import lev_oracle
    from tests import pairs_join_cases as PJ
    oracle = PJ._oracle()
    fl, tl, sims = BT.small_two_lists()
    strings, self_sims = BT.small_self()
    hub, h, partners = BT.hub("first", 80, _lib.PAIR_SLICE)
    assert h == 0 and partners == 2 * _lib.PAIR_SLICE + 40
    hub_sims = {name: lev_oracle.sim_matrix(hub, hub, lev_oracle.matrix(list(hub), list(hub), name, workers=8)) for name in lev_oracle.SCORERS}
    hub_sims.update({name: oracle.jaro_matrix(list(hub), list(hub), name) for name in ("jaro", "jaro_winkler")})
    out = {"small_two_lists": (fl, tl, dict(sims)), "small_self": (strings, None, dict(self_sims)), "hub_first_80": (hub, None, hub_sims)}
    for a, b, s in out.values():
        s["ratio"] = oracle.indel_argmax(list(a), list(b or a), want_matrix=True)[2]
    return out


def run_blocked(ctx):
    from polyfuzz_amd import _lib
    from tests import blocked_threshold_cases as BT
    from tests import pairs_join_cases as PJ
    run = Run()
    for case, (fl, tl, _) in blocked_cases().items():
        self_join = tl is None
        f = _lib.DeviceStrings.upload(ctx, list(fl))
        t = None if self_join else _lib.DeviceStrings.upload(ctx, list(tl))
        vec = _lib.DeviceTfidf.fit(ctx, _lib.TfidfParams(3, 3, 1, 1), f if self_join else t, None if self_join else f)
        a = vec.transform(f)
        index = _lib.DeviceIndex.build(ctx, a if self_join else vec.transform(t))
        row_ptr, idx, sim, _ = _lib.sparse_join(ctx, index, a, BT.B, self_join=self_join)
        run.put(f"{case}.k15", row_ptr, idx, sim)
        pairs = _lib.sparse_join_dev(ctx, index, a, BT.B, self_join=self_join)
        table = PJ.device_table(ctx, BT.padded_table(row_ptr, idx))
        room = max(1, len(idx))
        for name in FIVE:
            run.put(f"{case}.rescore_topn.{name}", *_lib.pairs_rescore_topn(ctx, f, f if self_join else t, table, name, 3))
        for name in PJ.FOUR:
            run.put(f"{case}.pairs_join.{name}", *_lib.pairs_join(ctx, f, t, table, name, 0.8, capacity=room))
            run.put(f"{case}.pairs_join_repeat.{name}", *_lib.pairs_join(ctx, f, t, table, name, 0.8, capacity=1))
            run.put(f"{case}.pairs_join_keys.{name}", *_lib.pairs_join_keys(ctx, f, t, pairs, name, 0.8, capacity=room))
            run.put(f"{case}.pairs_join_keys_repeat.{name}", *_lib.pairs_join_keys(ctx, f, t, pairs, name, 0.8, capacity=1))
            if self_join:
                label, n_pairs, n_comp = _lib.pairs_components(ctx, f, table, name, 0.8)
                run.put(f"{case}.pairs_components.{name}", label, np.array([n_pairs, n_comp], np.int64))
                label, n_pairs, n_comp = _lib.pairs_components_keys(ctx, f, pairs, name, 0.8)
                run.put(f"{case}.pairs_components_keys.{name}", label, np.array([n_pairs, n_comp], np.int64))
    return run


def check_blocked(run, oracle):
    from tests import blocked_threshold_cases as BT
    from tests import pairs_join_cases as PJ
    from tests.test_pairs_rescore_gpu import expected
    for case, (fl, tl, sims) in blocked_cases().items():
        self_join = tl is None
        row_ptr, idx, _ = run.get_all(f"{case}.k15")
        assert len(idx) >= 50                                           # (K15's own pairs are held by the tfidf group and its tests)
        table = BT.padded_table(row_ptr, idx)
        for name in FIVE:
            _equal(run.get_all(f"{case}.rescore_topn.{name}"), expected(sims[name], table, 3), f"{case}.rescore_topn.{name}")
        for name in PJ.FOUR:
            want = BT.expected_keys_join(sims[name], row_ptr, idx, 0.8)
            assert 1 < len(want[1]) <= len(idx), (case, name)           # (capacity 1 is too small: the repeat ran)
            assert len(want[1]) < len(idx) or case.startswith("hub")    # (the threshold cuts; a hub's variants all pass it)
            for entry in ("pairs_join", "pairs_join_repeat", "pairs_join_keys", "pairs_join_keys_repeat"):
                _equal(run.get_all(f"{case}.{entry}.{name}"), want, f"{case}.{entry}.{name}")
            if self_join:
                label = PJ.expected_labels(len(fl), want[0], want[1])
                counts = np.array([len(want[1]), len(np.unique(label))], np.int64)
                for entry in ("pairs_components", "pairs_components_keys"):
                    _equal(run.get_all(f"{case}.{entry}.{name}"), (label, counts), f"{case}.{entry}.{name}")


# ==== sharded: world 2 on the local transport =========================================================================================

@functools.lru_cache(maxsize=None)
def sharded_lists():
    from polyfuzz_amd import synth
    return tuple(synth.company_names(301, 11)), tuple(synth.company_names(257, 12))


def run_sharded(ctxs):
    """ctxs: the two contexts of the ranks (the fill is set on both); the communicators are this run's own"""
    import concurrent.futures as cf
    from polyfuzz_amd import _lib, pipeline
    run = Run()
    fl, tl = [list(x) for x in sharded_lists()]
    comms = _lib.Comm.local_group(ctxs)
    try:
        res = pipeline.run_sharded_job(ctxs, comms, fl, tl, top_n=4, min_similarity=0.0)
        for r, ((idx, val), job) in enumerate(res):
            run.put(f"from_sharded.rank{r}", idx, val, job.vec.export()[1])
        del res

        def rank_fn(r):
            b, e = pipeline.shard_bounds(len(tl), 2, r)
            job = pipeline.ToShardedMatchJob(ctxs[r], fl, tl[b:e], b, comms[r], top_n=4, min_similarity=0.0)
            return job.step().download(), job.vec.export()[1]
        with cf.ThreadPoolExecutor(2) as ex:
            outs = [x.result(timeout=120) for x in [ex.submit(rank_fn, r) for r in range(2)]]
        for r, ((idx, val), idf) in enumerate(outs):
            run.put(f"to_sharded.rank{r}", idx, val, idf)
    finally:
        for c in comms:
            c.free()
    return run


def check_sharded(run, oracle):
    from tests.helpers import vectorize_pair
    fl, tl = [list(x) for x in sharded_lists()]
    a3, b3, n_col = vectorize_pair(oracle, fl, tl)
    o = oracle.TfidfOracle().fit(tl + fl)
    e_idx, e_val = oracle.cossim_topn(a3, b3, n_col, 4, 0.0)
    for entry, near_ties in (("from_sharded", 1), ("to_sharded", 2)):           # tests/test_comm_gpu.py's rule for each
        for r in range(2):
            idx, val, idf = run.get_all(f"{entry}.rank{r}")
            assert np.abs(val - e_val).max() <= 1e-5 and (idx != e_idx).any(axis=1).sum() <= near_ties, (entry, r)
            np.testing.assert_allclose(idf, o.idf, rtol=1e-15)
            for g, w in zip((idx, val, idf), run.get_all(f"{entry}.rank0")):    # every rank holds the whole result
                assert g.tobytes() == w.tobytes(), (entry, r)


GROUPS = {"tfidf": (run_tfidf, check_tfidf), "edit": (run_edit, check_edit), "fuzz": (run_fuzz, check_fuzz),
          "dense": (run_dense, check_dense), "blocked": (run_blocked, check_blocked)}
