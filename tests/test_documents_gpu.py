"""K1/K2 and K3 on DOCUMENTS -- strings of thousands of characters, CSR rows of thousands of entries -- against the oracle.

Part A: the vectoriser's long-row kernel (k_rows_long: LDS sort up to 4 096 n-grams, global-scratch sort beyond) on documents at
its seams, against oracle.TfidfOracle, structure equal and values within 2e-7.
Part B: every form of K3 on a list with rows of 65 .. 16 000 entries against oracle.cossim_topn (float64): each score within
`k3_bound` of the oracle's -- one truncation per shared column: 1e-5 holds up to about 10 000 shared columns, NOT beyond --, the forms
equal bit for bit.
Part C: TFIDF.match_device on names and documents, end to end.
The lists, the acceptance rule and what the oracle alone guarantees about them: tests/document_cases.py, tests/test_documents_cpu.py."""
import contextlib

import numpy as np
import pytest

from tests import document_cases as dc
from tests.helpers import SCORE_TOL, assert_topn_parity, lockstep_launches
from tests.test_k3_cossim_gpu import _self_match
from tests.test_vectorize_gpu import _check_csr, _device_vectorize

pytestmark = pytest.mark.gpu


# ---- part A: K1/K2 -------------------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def _rows_long_launches(ctx):
    """box["launches"]: launches of k_rows_long inside the block"""
    box = {}
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        yield box
        ctx.sync()
        box["launches"] = ctx.prof_get("k2_rows_long")[1]
    finally:
        ctx.prof_enable(False)


def _fit_and_check(ctx, oracle_mod, lst, to, rng, clean, min_longest=4096):
    """fit (on to + lst) and transform on the device, with k_rows_long seen to run, against the oracle: matrices, vocabulary, df, idf"""
    with _rows_long_launches(ctx) as box:
        vec, out = _device_vectorize(ctx, lst, to, rng[0], rng[1], clean)
    assert box["launches"] >= 1
    o = oracle_mod.TfidfOracle(n_gram_range=rng, clean=clean).fit((to or []) + lst)
    assert max(len(o._analyze(s)) for s in (to or []) + lst) > min_longest
    _check_csr(out[0], o.transform(lst), len(o.vocabulary))
    if to is not None:
        _check_csr(out[1], o.transform(to), len(o.vocabulary))
    ngrams, idf, df = vec.export()
    assert ["".join(chr(c) for c in row if c) for row in ngrams.tolist()] == o.vocabulary
    np.testing.assert_array_equal(df, o.df)
    np.testing.assert_allclose(idf, o.idf, rtol=1e-15)
    return vec, out


def _same_bits(x, y):
    for p, q in zip(x, y):
        np.testing.assert_array_equal(p, q)


@pytest.mark.parametrize("clean", [True, False])
def test_documents_at_the_seams_of_the_long_row_sort(ctx, oracle_mod, clean):
    """4 095 / 4 096 / 4 097 / 8 192 / 8 193 n-grams (either side of the LDS sort's limit and of the scratch sort's next power of
    two), each as a document of mostly distinct n-grams, of eight distinct ones at most, and of singleton first and last keys; the
    first row, the last row and rows inside; an empty and a one-character string beside a document in one wave of k_finalize"""
    _fit_and_check(ctx, oracle_mod, dc.seam_list(), None, (3, 3), clean, min_longest=8192)


@pytest.mark.parametrize("rng,lengths,wide_codes", [((2, 4), (1367, 1368, 5000), False), ((3, 7), (823, 824, 3000), True)])
def test_documents_with_several_n_values(ctx, oracle_mod, rng, lengths, wide_codes):
    """three / five slots per character: 4 095 and 4 098 (4 100) n-grams and one far beyond; with (3, 7) the codes are wider than
    32 bits, so the giant rows are ranked by binary search in the sorted vocabulary"""
    vec, _ = _fit_and_check(ctx, oracle_mod, dc.range_list(lengths, 102), None, rng, True)
    assert (vec.info()["code_bits"] > 32) == wide_codes


def test_more_giant_rows_than_scratch_slabs(ctx, oracle_mod):
    """70 tiles of 16 strings with a giant row each -- the giant grid has 64 workgroups, so slabs are used again --, two tiles with
    two giants"""
    _fit_and_check(ctx, oracle_mod, dc.slab_list(), None, (3, 3), True)


def test_transform_of_unseen_documents(ctx, oracle_mod):
    """a transform of documents the fit did not see: one of known letters, one of unknown letters only (an empty row), one mixed
    (its unknown n-grams sort behind the known ones: the run lengths end at the count of valid keys); and a document of wide
    characters (another kernel instance)"""
    from polyfuzz_amd import _lib
    fit, new = dc.unseen_lists()
    params = _lib.TfidfParams(3, 3, 0, 1)
    vec = _lib.DeviceTfidf.fit(ctx, params, _lib.DeviceStrings.upload(ctx, fit), None)
    o = oracle_mod.TfidfOracle(clean=False).fit(fit)
    with _rows_long_launches(ctx) as box:
        got = vec.transform(_lib.DeviceStrings.upload(ctx, new)).download()
    assert box["launches"] >= 1
    exp = o.transform(new)
    _check_csr(got, exp, len(o.vocabulary))
    nnz = np.diff(exp[0])
    docs = [i for i, s in enumerate(new) if len(s) >= 4000]
    assert sorted(nnz[docs] == 0) == [False, False, True]
    rng = np.random.default_rng(7)
    greek = "".join(chr(0x3b1 + i) for i in range(24))
    wide = new[:40] + [dc.doc(rng, 5000, greek), dc.doc(rng, 4200, dc.UNSEEN_FIT_ALPHABET + greek)]
    got = vec.transform(_lib.DeviceStrings.upload(ctx, wide)).download()
    exp = o.transform(wide)
    _check_csr(got, exp, len(o.vocabulary))
    assert exp[0][-2] == exp[0][-3] and exp[0][-1] > exp[0][-2]


def test_two_list_fit_with_giant_rows(ctx, oracle_mod, monkeypatch):
    """giants in the to-list only, in the from-list only, in both: the fit that shares its launches between the lists and the one
    with a launch per list (PFZ_K1_TWO_LISTS=0) agree bit for bit, and with the oracle"""
    for to, frm in dc.two_list_cases():
        got = {}
        for knob in ("1", "0"):
            monkeypatch.setenv("PFZ_K1_TWO_LISTS", knob)
            vec, out = _fit_and_check(ctx, oracle_mod, frm, to, (3, 3), True)
            got[knob] = (vec.export(), out[0], out[1])
        for m in range(3):
            _same_bits(got["1"][m], got["0"][m])


@pytest.mark.parametrize("knob", ["PFZ_NO_LDS_HIST", "PFZ_K2_SELF_SCAN"])
def test_seam_documents_on_both_paths(ctx, oracle_mod, monkeypatch, knob):
    """the seam list with the document frequencies counted by global atomics (PFZ_NO_LDS_HIST=1) and with the row counts added up by
    the scan kernels and by k_finalize itself (PFZ_K2_SELF_SCAN 0 / 1): vectoriser and matrix equal bit for bit"""
    lst = dc.seam_list()
    got = {}
    for value in ("1", "0"):
        monkeypatch.setenv(knob, value)
        vec, out = _fit_and_check(ctx, oracle_mod, lst, None, (3, 3), True, min_longest=8192)
        got[value] = (vec.export(), out[0])
    for m in range(2):
        _same_bits(got["1"][m], got["0"][m])


# ---- part B: K3 ----------------------------------------------------------------------------------------------------------------------

_ROW_MAJOR = (("PFZ_K3_SYM", "0"), ("PFZ_K3_LOCKSTEP", "0"))
_memo = {}


def _knobs(monkeypatch, pairs):
    for k in ("PFZ_K3_SYM", "PFZ_K3_LOCKSTEP", "PFZ_K3_LS_BLOCKS", "PFZ_K3_LS_CHUNK", "PFZ_K3_SLICES", "PFZ_K3_BLOCK",
              "PFZ_K3_BANK_ORDER", "PFZ_NO_LDS_HIST"):
        monkeypatch.delenv(k, raising=False)
    for k, v in pairs:
        monkeypatch.setenv(k, v)


@pytest.fixture(scope="module")
def k3_case(oracle_mod):
    a3, held = dc.k3_list()
    dense = {}

    def dense_row(i):
        if i not in dense:
            dense[i] = oracle_mod.cossim_dense(a3, a3, dc.K3_COLS, rows=(i, i + 1))[0]
        return dense[i]
    return {"a3": a3, "held": held, "dense_row": dense_row, "shared": dc.shared_counter(a3, a3, dc.K3_COLS),
            "others": np.setdiff1d(np.arange(dc.K3_N), held), "size": {r: s for s, p in list(dc.K3_DOCS.items()) + list(dc.K3_PAIR.items()) for r in p}}


def _row_major(ctx, monkeypatch, case, ntop):
    """the row-major kernel's self-match of the list (computed once per ntop; read-only)"""
    if ("self", ntop) not in _memo:
        _knobs(monkeypatch, _ROW_MAJOR)
        _memo["self", ntop] = _self_match(ctx, case["a3"], dc.K3_COLS, ntop, 0.0)
    return _memo["self", ntop]


def _row_major_two_lists(ctx, monkeypatch, case):
    from polyfuzz_amd import _lib
    if "two" not in _memo:
        _knobs(monkeypatch, _ROW_MAJOR)
        _memo["two"] = _lib.cossim_topn_host(ctx, dc.take_rows(case["a3"], case["held"]), case["a3"], dc.K3_COLS, 5, 0.5)
    return _memo["two"]


def _report(case, cells, what):
    """per document size: the largest |error| of a cell, its ratio to the cell's bound, and the largest ratio"""
    by = {}
    for i, j, c, err in cells:
        by.setdefault(case["size"][i], []).append((abs(err), abs(err) / dc.k3_bound(c), c, err))
    for size in sorted(by):
        e = max(by[size])
        print(f"K3 documents [{what}] {size:6d} entries: largest error {e[3]:+.3e} at {e[2]:6d} shared columns = {e[1]:.2f} of its bound; "
              f"largest ratio {max(x[1] for x in by[size]):.2f}; {len(by[size])} cells")


def _hold_to_the_oracle(case, oracle_mod, idx, val, exp_idx, exp_val, what, exclude_diag, lower_bound=0.0):
    held = case["held"]
    cells = dc.assert_topn_within_bound(idx, val, exp_idx, exp_val, case["dense_row"], case["shared"], rows=held,
                                        exclude_diag=exclude_diag, lower_bound=lower_bound)
    _report(case, cells, what)
    # cells whose bound is below 1e-5 are held to 1e-5 as well (the 16 000-entry pair, 15 840 shared columns, is not)
    for i, j, c, err in cells:
        assert dc.k3_bound(c) >= SCORE_TOL or abs(err) <= SCORE_TOL
        assert dc.k3_bound(c) < SCORE_TOL or {i, j} <= set(dc.K3_PAIR[16000])
    assert any(c > 15000 for _, _, c, _ in cells)


@pytest.mark.parametrize("ntop", [1, 5, 32])
def test_row_major_kernel_on_document_rows(ctx, oracle_mod, monkeypatch, k3_case, ntop):
    """the row-major kernel, self-match: the document rows by `assert_topn_within_bound`, the others by `assert_topn_parity`"""
    a3, held, others = k3_case["a3"], k3_case["held"], k3_case["others"]
    idx, val = _row_major(ctx, monkeypatch, k3_case, ntop)
    exp_idx, exp_val = oracle_mod.cossim_topn(a3, a3, dc.K3_COLS, ntop, 0.0, exclude_diag=True)
    _hold_to_the_oracle(k3_case, oracle_mod, idx[held], val[held], exp_idx[held], exp_val[held], f"self-match, top {ntop}", True)
    assert_topn_parity(idx[others], val[others], exp_idx[others], exp_val[others], oracle_mod, a3, a3, dc.K3_COLS, exclude_diag=True,
                       rows=others)
    for r in dc.K3_EMPTY:
        assert (idx[r] == -1).all() and (val[r] == 0).all()
    for size, places in list(dc.K3_DOCS.items()) + list(dc.K3_PAIR.items()):          # the copies are found
        for r in places:
            assert idx[r, 0] in places and idx[r, 0] != r
    # and with one to-side slice instead of the two this size gets: the same bits
    _knobs(monkeypatch, _ROW_MAJOR + (("PFZ_K3_SLICES", "1"),))
    _same_bits(_self_match(ctx, a3, dc.K3_COLS, ntop, 0.0), (idx, val))


def test_row_major_kernel_documents_against_the_list(ctx, oracle_mod, monkeypatch, k3_case):
    """two lists: the document rows as the from-side against the whole list, top 5 above 0.5 (every row finds itself first)"""
    a3, held = k3_case["a3"], k3_case["held"]
    idx, val = _row_major_two_lists(ctx, monkeypatch, k3_case)
    exp_idx, exp_val = oracle_mod.cossim_topn(dc.take_rows(a3, held), a3, dc.K3_COLS, 5, 0.5)
    np.testing.assert_array_equal(idx[:, 0], held)
    _hold_to_the_oracle(k3_case, oracle_mod, idx, val, exp_idx, exp_val, "two lists, top 5 above 0.5", False, lower_bound=0.5)
    np.testing.assert_array_equal(idx, exp_idx)
    assert ((idx >= 0).sum(axis=1) == [2 if k3_case["size"][r] == 16000 else 3 for r in held.tolist()]).all()


@pytest.mark.parametrize("chunk", ["1", "5", None])
@pytest.mark.parametrize("blocks", ["1", "2"])
def test_lockstep_kernel_on_document_rows(ctx, monkeypatch, k3_case, blocks, chunk):
    """the lock-step form: a document is "a window of its own" walked by the slow loop, its state crosses the slices (two or three of
    them), it opens and closes a chunk (chunks of 1, 5 and -- the default at this size -- 4 rows): the row-major result bit for bit,
    twice on one index"""
    from polyfuzz_amd import _lib
    a3, held = k3_case["a3"], k3_case["held"]
    ref = {ntop: _row_major(ctx, monkeypatch, k3_case, ntop) for ntop in (5, 32)}
    ref_two = _row_major_two_lists(ctx, monkeypatch, k3_case)
    _knobs(monkeypatch, (("PFZ_K3_SYM", "0"), ("PFZ_K3_LOCKSTEP", "1"), ("PFZ_K3_LS_BLOCKS", blocks)) +
           ((("PFZ_K3_LS_CHUNK", chunk),) if chunk else ()))
    csr = _lib.DeviceCSR.upload(ctx, a3[0], a3[1], a3[2], dc.K3_COLS)
    index = _lib.DeviceIndex.build(ctx, csr)
    with lockstep_launches(ctx) as box:
        for ntop in (5, 32):
            for _ in range(2):
                _same_bits(_lib.cossim_topn(ctx, index, csr, ntop, 0.0, exclude_diag=True).download(), ref[ntop])
        _same_bits(_lib.cossim_topn_host(ctx, dc.take_rows(a3, held), a3, dc.K3_COLS, 5, 0.5), ref_two)
    assert box["launches"] == 5


@pytest.mark.parametrize("ntop", [1, 5, 32])
def test_symmetric_kernel_on_document_rows(ctx, monkeypatch, k3_case, ntop):
    """the symmetric form: the sums of a document and its copies in higher blocks are handed over through HBM; whole and in the row
    ranges that cut at the empty row 2048 and behind it: the row-major result bit for bit, twice"""
    from polyfuzz_amd import _lib
    a3 = k3_case["a3"]
    ref = _row_major(ctx, monkeypatch, k3_case, ntop)
    _knobs(monkeypatch, (("PFZ_K3_SYM", "1"), ("PFZ_K3_LOCKSTEP", "0")))
    csr = _lib.DeviceCSR.upload(ctx, a3[0], a3[1], a3[2], dc.K3_COLS)
    index = _lib.DeviceIndex.build(ctx, csr)
    for _ in range(2):
        _same_bits(_lib.cossim_topn(ctx, index, csr, ntop, 0.0, exclude_diag=True).download(), ref)
    assert index.symmetric_launches() == (2, 2 * dc.K3_N)
    _same_bits(_self_match(ctx, a3, dc.K3_COLS, ntop, 0.0, ranges=[(0, 2048), (2048, 2049), (2049, dc.K3_N)], repeats=2), ref)


@pytest.mark.parametrize("knobs", [(("PFZ_K3_SLICES", "3"),), (("PFZ_K3_BLOCK", "4096"),),
                                   (("PFZ_NO_LDS_HIST", "1"),), (("PFZ_K3_BANK_ORDER", "1"),)])
def test_launch_shapes_and_index_builds_on_document_rows(ctx, monkeypatch, k3_case, knobs):
    """three to-side slices, to-blocks of 4 096 rows, the index built with global atomics, its heavy lists in bank order: the same
    bits; the index holds the pieces its list lengths say"""
    from polyfuzz_amd import _lib
    a3 = k3_case["a3"]
    ref = _row_major(ctx, monkeypatch, k3_case, 5)
    _knobs(monkeypatch, _ROW_MAJOR + knobs)
    _same_bits(_self_match(ctx, a3, dc.K3_COLS, 5, 0.0), ref)
    info = _lib.DeviceIndex.build(ctx, _lib.DeviceCSR.upload(ctx, a3[0], a3[1], a3[2], dc.K3_COLS)).info()
    blk = info["block_cols"]
    assert blk == (4096 if knobs[0][0] == "PFZ_K3_BLOCK" else 2048) and info["n_blocks"] == (dc.K3_N + blk - 1) // blk
    rows = np.repeat(np.arange(dc.K3_N), np.diff(a3[0]))
    cnt = np.bincount(a3[1].astype(np.int64) * info["n_blocks"] + rows // blk, minlength=dc.K3_COLS * info["n_blocks"])
    assert info["piece_postings"] == 16 and info["n_pieces"] == int(((cnt + 15) // 16).sum())


def test_unnormalised_document_rows(ctx, oracle_mod, monkeypatch, k3_case):
    """the 8 000-entry rows' values times 7.5: the fixed-point scale follows the norm bound (k3_fixed_point: 2^25), the error bound
    with it -- k3_bound(c, 7.5 * 7.5 * 1.0001); the three forms still agree bit for bit"""
    a3 = k3_case["a3"]
    big = np.array(dc.K3_DOCS[8000], np.int64)
    data = a3[2].copy()
    for r in big.tolist():
        data[a3[0][r]:a3[0][r + 1]] *= 7.5
    s3 = (a3[0], a3[1], data)
    _knobs(monkeypatch, _ROW_MAJOR)
    idx, val = _self_match(ctx, s3, dc.K3_COLS, 5, 0.0)
    exp_idx, exp_val = oracle_mod.cossim_topn(s3, s3, dc.K3_COLS, 5, 0.0, exclude_diag=True, rows=big)
    dense_row = lambda i: oracle_mod.cossim_dense(s3, s3, dc.K3_COLS, rows=(i, i + 1))[0]
    norm_bound = 7.5 * 7.5 * 1.0001
    cells = dc.assert_topn_within_bound(idx[big], val[big], exp_idx, exp_val, dense_row, k3_case["shared"], rows=big,
                                        exclude_diag=True, norm_bound=norm_bound)
    np.testing.assert_array_equal(idx[big], exp_idx)
    for i, j, c, err in cells:
        print(f"K3 documents [values x 7.5] rows {i} x {j}: {c} shared columns, error {err:+.3e} = "
              f"{abs(err) / dc.k3_bound(c, norm_bound):.2f} of its bound")
    assert max(c for _, _, c, _ in cells) > 7000
    _knobs(monkeypatch, (("PFZ_K3_SYM", "1"), ("PFZ_K3_LOCKSTEP", "0")))
    _same_bits(_self_match(ctx, s3, dc.K3_COLS, 5, 0.0), (idx, val))
    _knobs(monkeypatch, (("PFZ_K3_SYM", "0"), ("PFZ_K3_LOCKSTEP", "1")))
    _same_bits(_self_match(ctx, s3, dc.K3_COLS, 5, 0.0), (idx, val))


# ---- part C: end to end --------------------------------------------------------------------------------------------------------------

def test_tfidf_match_on_names_and_documents(ctx, oracle_mod):
    """TFIDF(top_n=3).match_device on 300 names, eight documents of 4 099 .. 9 000 characters and two edited copies of each,
    against the oracle's vectoriser followed by oracle.cossim_topn; a document's best match is its 0.5 % copy"""
    from polyfuzz_amd.models import TFIDF
    lst, docs, near, far = dc.end_to_end_list()
    idx, val = TFIDF(n_gram_range=(3, 3), min_similarity=0, top_n=3).match_device(lst).download()
    o = oracle_mod.TfidfOracle().fit(lst)
    a3 = o.transform(lst)
    n_col = len(o.vocabulary)
    exp_idx, exp_val = oracle_mod.cossim_topn(a3, a3, n_col, 3, 0.0, exclude_diag=True)
    held = np.array(sorted(docs + near + far), np.int64)
    others = np.setdiff1d(np.arange(len(lst)), held)
    dense_row = lambda i: oracle_mod.cossim_dense(a3, a3, n_col, rows=(i, i + 1))[0]
    cells = dc.assert_topn_within_bound(idx[held], val[held], exp_idx[held], exp_val[held], dense_row, dc.shared_counter(a3, a3, n_col),
                                        rows=held, exclude_diag=True)
    assert_topn_parity(idx[others], val[others], exp_idx[others], exp_val[others], oracle_mod, a3, a3, n_col, exclude_diag=True,
                       rows=others)
    np.testing.assert_allclose(val[held], exp_val[held], rtol=0, atol=SCORE_TOL)       # every bound here is below 1e-5
    e = max(cells, key=lambda x: abs(x[3]))
    print(f"K1-K3 documents [end to end] largest error {e[3]:+.3e} at {e[2]} shared n-grams = {abs(e[3]) / dc.k3_bound(e[2]):.2f} of its bound")
    assert e[2] > 4000
    np.testing.assert_array_equal(idx[docs, 0], near)
