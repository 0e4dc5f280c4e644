"""Inputs and references of the K15 tests (tests/test_sparse_join_gpu.py, tests/test_sparse_components_gpu.py,
tests/test_sparse_join_cpu.py): the lists, the float64 oracle's pairs (oracle/tfidf_numpy.py), and what the GPU files share on
the device -- each case fitted once, its join computed once, and the existing path to the same pairs (K3's top-n table with
lower_bound 0, thresholded on the host)."""
import functools
import os

import numpy as np

from tests import document_cases as dc
from tests.dense_join_cases import csr_pairs, union_find_labels      # noqa: F401  (shared with the K14 tests)

THRESHOLDS = (0.6, 0.8, 0.9)
BAND = 1e-5              # the project's documented K3 tolerance (these rows share about 13 n-grams)

# name -> (PFZ_K3_BLOCK of the fit or None for the default, ntop of the existing path or None for "the number of rows"); why each is there:
#   names2600  three blocks of 1024, the last one ragged; two strings too short for a trigram (empty rows)
#   names10k   five blocks of the default 2048
#   spliced    equal strings in another block, 150 contiguous copies (more than 64 hits in one sweep step, several per lane),
#              five documents of about 300 characters with an edited copy each (the chunk loop of rows beyond 64 n-grams)
SELF_CASES = {"names2600": ("1024", 128), "names10k": (None, 192), "spliced": ("1024", None)}
# two lists: names[2600:3300] plus 50 edited strings of the to-list, against names2600
TWO_LIST_CASE = "two_list"
CASE_KNOBS = dict(SELF_CASES, **{TWO_LIST_CASE: ("1024", 128)})

# float64 oracle: (unordered pairs with cosine >= t, pairs within BAND of t)
ORACLE_HITS = {
    "names2600": {0.6: (2512, 0), 0.8: (592, 0), 0.9: (296, 0)},
    "names10k": {0.6: (34986, 4), 0.8: (6264, 2), 0.9: (2616, 0)},
}
_ORACLE_FLOOR = 0.5      # the oracle's pairs are kept from here up


@functools.lru_cache(maxsize=None)
def _company_names():
    from polyfuzz_amd import datasets
    return tuple(datasets.load_company_names())


@functools.lru_cache(maxsize=None)
def lists(name):
    """(from-list, to-list or None for a self-join), as tuples"""
    names = _company_names()
    if name == "names2600":
        return names[:2600], None
    if name == "names10k":
        return names[:10000], None
    if name == "names300":
        return names[:300], None
    if name == "spliced":
        rng = np.random.default_rng(15)
        out = list(names[:2600]) + list(names[:300]) + [names[1000]] * 150
        for _ in range(5):
            d = dc.doc(rng, 300)
            out += [d, dc.edited(rng, d, 0.02)]
        return tuple(out), None
    if name == TWO_LIST_CASE:
        rng = np.random.default_rng(16)
        to = names[:2600]
        picks = rng.choice(len(to), size=50, replace=False)
        return tuple(list(names[2600:3300]) + [dc.edited(rng, to[int(i)].lower(), 0.1) for i in picks]), to
    raise KeyError(name)


# ---- the float64 oracle ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def oracle_csr(name):
    """the self case's TF-IDF rows as the float64 oracle computes them: scipy CSR"""
    import oracle
    from scipy.sparse import csr_matrix
    strings, _ = lists(name)
    o = oracle.tfidf_numpy.TfidfNumpyOracle((3, 3)).fit(list(strings))
    indptr, cols, data = o.transform_fitted(0, len(strings))
    return csr_matrix((data, cols, indptr), shape=(len(strings), len(o.codes)))


@functools.lru_cache(maxsize=None)
def oracle_pairs(name):
    """scipy CSR of the float64 cosines >= 0.5 of the self case, columns j > i only"""
    from scipy.sparse import triu, vstack
    a = oracle_csr(name)
    at = a.T.tocsr()
    parts = []
    for r0 in range(0, a.shape[0], 1000):
        p = (a[r0:r0 + 1000] @ at).tocsr()
        p.data[p.data < _ORACLE_FLOOR] = 0.0
        p.eliminate_zeros()
        parts.append(p)
    return triu(vstack(parts), k=1).tocsr()


def oracle_counts(name, t):
    """(hits, pairs within BAND of t) of the float64 oracle"""
    d = oracle_pairs(name).data
    return int((d >= t).sum()), int((np.abs(d - t) < BAND).sum())


# ---- the device side, shared by the GPU test files ------------------------------------------------------------------------------
_cache = {}


def _fit(strings, to, block):
    """a TFIDF model fitted as match() fits it, under the case's PFZ_K3_BLOCK -> (model, from-side DeviceCSR)"""
    from polyfuzz_amd.models import TFIDF
    old = os.environ.pop("PFZ_K3_BLOCK", None)
    if block is not None:
        os.environ["PFZ_K3_BLOCK"] = block
    try:
        m = TFIDF()
        from_dev, _ = m._extract_tf_idf(list(strings), None if to is None else list(to), True)
    finally:
        os.environ.pop("PFZ_K3_BLOCK", None)
        if old is not None:
            os.environ["PFZ_K3_BLOCK"] = old
    return m, from_dev


def fitted(ctx, name, block="case"):
    """(model, from-side DeviceCSR, DeviceIndex, self?) of a case, resident"""
    if block == "case":
        block = CASE_KNOBS.get(name, ("1024", None))[0]
    if ("fit", name, block) not in _cache:
        strings, to = lists(name)
        m, from_dev = _fit(strings, to, block)
        _cache["fit", name, block] = (m, from_dev, m._dev_index, to is None)
    return _cache["fit", name, block]


def join(ctx, name, t):
    """the join of a case (computed once): (rows, cols, scores, row_ptr, counts)"""
    from polyfuzz_amd import _lib
    if ("join", name, t) not in _cache:
        _, from_dev, index, self_join = fitted(ctx, name)
        row_ptr, idx, sim, counts = _lib.sparse_join(ctx, index, from_dev, t, self_join=self_join, counters=True)
        rows, cols = csr_pairs(row_ptr, idx)
        _cache["join", name, t] = (rows, cols, sim, row_ptr, counts)
    return _cache["join", name, t]


def existing_table(ctx, name, ntop=None):
    """the way to the same pairs before K15: K3's top-n table of the case with lower_bound 0, every row wide enough that nothing
    is cut (asserted) -> (idx, val), computed once"""
    from polyfuzz_amd import _lib
    if ("table", name) not in _cache:
        _, from_dev, index, _ = fitted(ctx, name)
        if ntop is None:
            ntop = CASE_KNOBS.get(name, (None, None))[1] or from_dev.n_rows
        idx, val = _lib.cossim_topn(ctx, index, from_dev, int(ntop), 0.0, exclude_diag=False).download()
        _cache["table", name] = (idx, val)
    return _cache["table", name]


def threshold_table(idx, val, t, self_join):
    """(rows, cols, scores) of a top-n table's entries with float64(score) >= t, by row, then column; a self-join keeps j > i.
    Nothing was cut: no row is full of entries that pass (with lower_bound 0 a row holds every to-row it shares an n-gram with,
    best first, so many rows are full -- of scores far below t; a row whose LAST entry passes may have lost a pair)."""
    passes = (idx >= 0) & (val.astype(np.float64) >= t)
    assert not passes[:, -1].any(), f"a row of the existing path's table is full of hits at t = {t}, ntop = {idx.shape[1]}"
    rows, slot = np.nonzero(passes)
    cols, vals = idx[rows, slot], val[rows, slot]
    if self_join:
        keep = cols > rows
        rows, cols, vals = rows[keep], cols[keep], vals[keep]
    order = np.lexsort((cols, rows))
    return rows[order], cols[order], vals[order]


def existing_path(ctx, name, t):
    return threshold_table(*existing_table(ctx, name), t, lists(name)[1] is None)
