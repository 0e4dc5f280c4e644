"""Inputs and references of the K14 tests (tests/test_dense_join_gpu.py, tests/test_dense_components_gpu.py): the clustered
generator, the cases, the float64 cosines of oracle/dense.py with their hits, a ten-line union-find, and what the two files share
on the device -- the resident lists, each case's join computed once, and the existing path to the same pairs."""
import functools

import numpy as np

THRESHOLDS = (0.6, 0.8, 0.9)
BAND = 1e-5              # the project's fp32 tolerance of a dense score (tests/test_dense_gpu.py)

# name -> (n, d, k, seed); why each is there:
#   300x96   three row tiles, one with 44 rows
#   257x40   width padded to 64; a last tile of ONE row
#   130x32   one k-chunk, so the pipeline's shortest trip; diagonal tiles plus one off-diagonal tile
SELF_CASES = {"300x96": (300, 96, 30, 7), "257x40": (257, 40, 20, 8), "130x32": (130, 32, 5, 10)}
# two lists: 200 x 1000 of width 64; the to-list is the generator's 1000 rows reversed
TWO_LIST_CASE = "200x1000"

# float64 oracle: hits, and the pairs within BAND of t (computed with numpy from the generator below)
ORACLE_HITS = {
    "300x96": {0.6: (1478, 0), 0.8: (1254, 0), 0.9: (2, 0)},
    "257x40": {0.6: (1636, 0), 0.8: (1347, 0), 0.9: (106, 0)},
    "130x32": {0.6: (1721, 0), 0.8: (859, 1), 0.9: (30, 0)},
    "200x1000": {0.6: (10039, 0), 0.8: (7659, 0), 0.9: (164, 0)},
}
ORACLE_COMPONENTS = {
    "300x96": {0.6: 30, 0.8: 34, 0.9: 298},
    "257x40": {0.6: 19, 0.8: 24, 0.9: 194},
    "130x32": {0.6: 5, 0.8: 7, 0.9: 103},
}


def gen(n, d, k, seed, noise=0.45):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((k, d))
    lab = rng.integers(0, k, n)
    return (c[lab] + noise * rng.standard_normal((n, d))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def lists(name):
    """(from-vectors, to-vectors or None for a self-join); cached, read-only"""
    if name == TWO_LIST_CASE:
        x, y = gen(200, 64, 20, 11), np.ascontiguousarray(gen(1000, 64, 20, 11)[::-1])
    else:
        x, y = gen(*SELF_CASES[name]), None
    x.setflags(write=False)
    if y is not None:
        y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def cosines(name):
    """float64 cosines of the case (oracle/dense.py); for a self-join everything but col > row is -inf"""
    import oracle
    x, y = lists(name)
    c = oracle.dense.dense_cossim(x, x if y is None else y)
    if y is None:
        c[np.tril_indices(len(x))] = -np.inf
    c.setflags(write=False)
    return c


def oracle_counts(name, t):
    """(hits, pairs within BAND of t) of the float64 oracle"""
    c = cosines(name)
    return int((c >= t).sum()), int((np.abs(c - t) < BAND).sum())


def union_find_labels(n, rows, cols):
    """label[i] = the smallest position of i's component under the edges (rows[k], cols[k])"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in zip(np.asarray(rows).tolist(), np.asarray(cols).tolist()):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)], np.int32)


def csr_pairs(row_ptr, idx):
    """(row of every hit, its column) from a join's CSR"""
    return np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr)), np.asarray(idx)


# ---- the device side, shared by the two GPU test files: resident lists and the joins computed once ------------------------
_cache = {}


def devs(ctx, name):
    """(from handle, to handle or None): the case's lists, resident"""
    from polyfuzz_amd import _lib
    if ("dev", name) not in _cache:
        x, y = lists(name)
        _cache["dev", name] = (_lib.DeviceDense.upload(ctx, x), None if y is None else _lib.DeviceDense.upload(ctx, y))
    return _cache["dev", name]


def join(ctx, name, t):
    """the join of a case (computed once): (rows, cols, scores, row_ptr, counts)"""
    from polyfuzz_amd import _lib
    if ("join", name, t) not in _cache:
        f, to = devs(ctx, name)
        row_ptr, idx, sim, counts = _lib.dense_join(ctx, f, to, t, counters=True)
        rows, cols = csr_pairs(row_ptr, idx)
        _cache["join", name, t] = (rows, cols, sim, row_ptr, counts)
    return _cache["join", name, t]


def existing_path(ctx, f, to, t):
    """the way to the same pairs before K14: the whole score panel, every column ranked, the filter `>` just below t32;
    (rows, cols, scores) by row, then column"""
    from polyfuzz_amd import _lib
    t32 = _lib.dense_threshold32(t)
    self_join = to is None
    to = f if self_join else to
    idx, val = _lib.dense_topn(ctx, f, to, to.n, float(np.nextafter(t32, np.float32(-np.inf))), exclude_diag=self_join).download()
    rows, slot = np.nonzero(idx >= 0)
    cols, vals = idx[rows, slot], val[rows, slot]
    if self_join:
        keep = cols > rows
        rows, cols, vals = rows[keep], cols[keep], vals[keep]
    order = np.lexsort((cols, rows))
    return rows[order], cols[order], vals[order]
