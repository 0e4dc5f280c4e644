"""Inputs and references of the K23 tests (tests/test_hamming_join_cpu.py, test_hamming_join_gpu.py, test_hamming_components_gpu.py):
the clustered code generator, the cases, the XOR / popcount matrix of tests/test_hamming_cpu.py thresholded at a distance, the
reference's own counts as constants, K14's ten-line union-find, and what the two GPU files share on the device -- the resident
handles, each case's join computed once, and the existing path (the whole score panel, every column ranked) to the same pairs."""
import functools

import numpy as np

from tests.dense_join_cases import csr_pairs, union_find_labels      # noqa: F401  (K14's, as they are)
from tests.test_hamming_cpu import hamming

THRESHOLDS = (0.6, 0.8, 0.9)
FLIP = 0.05             # every bit of a row differs from its cluster's base code with this probability

# name -> (n, d, k, seed); why each is there:
#   300x96     three row tiles, the last of 44 rows; a pitch with padding, 96 bits in 128
#   257x64     fingerprint width; a last tile of ONE row
#   130x4104   513 bytes a row: five LDS stages, the last one of 16 bytes; diagonal tiles plus one off-diagonal tile
SELF_CASES = {"300x96": (300, 96, 30, 7), "257x64": (257, 64, 20, 8), "130x4104": (130, 4104, 5, 10)}
# two lists: 200 x 1000 of 768 bits; the to-list is the generator's 1000 rows reversed
TWO_LIST_CASE = "200x1000"
CASES = tuple(SELF_CASES) + (TWO_LIST_CASE,)

# the distance each threshold stands for: the largest h with float64(float32(d - 2 h) / float32(d)) >= t (numpy)
HMAX = {
    "300x96": {0.6: 19, 0.8: 9, 0.9: 4},
    "257x64": {0.6: 12, 0.8: 6, 0.9: 3},
    "130x4104": {0.6: 820, 0.8: 410, 0.9: 205},
    "200x1000": {0.6: 153, 0.8: 76, 0.9: 38},
}
# the numpy oracle on the generator below: (hits, pairs exactly AT the cutoff).  The cutoffs fall inside the distance distribution:
# hundreds of pairs sit on them, so a `<` in place of `<=` cannot pass; the two empty results are the "no hit touches no memory" path.
ORACLE_HITS = {
    "300x96": {0.6: (1490, 1), 0.8: (885, 189), 0.9: (71, 41)},
    "257x64": {0.6: (1689, 14), 0.8: (1069, 265), 0.9: (306, 175)},
    "130x4104": {0.6: (1666, 0), 0.8: (1502, 14), 0.9: (0, 0)},
    "200x1000": {0.6: (10182, 0), 0.8: (7107, 466), 0.9: (0, 0)},
}
ORACLE_COMPONENTS = {
    "300x96": {0.6: 30, 0.8: 48, 0.9: 249},
    "257x64": {0.6: 20, 0.8: 34, 0.9: 130},
    "130x4104": {0.6: 5, 0.8: 5, 0.9: 130},
}


def gen(n, d, k, seed):
    """n packed rows of d bits around k random base codes"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 2, (k, d), dtype=np.uint8)
    lab = rng.integers(0, k, n)
    return np.packbits(base[lab] ^ (rng.random((n, d)) < FLIP), axis=1)


def bits(name):
    return 768 if name == TWO_LIST_CASE else SELF_CASES[name][1]


@functools.lru_cache(maxsize=None)
def lists(name):
    """(from-codes, to-codes or None for a self-join), packed uint8; cached, read-only"""
    if name == TWO_LIST_CASE:
        x, y = gen(200, 768, 20, 11), np.ascontiguousarray(gen(1000, 768, 20, 11)[::-1])
    else:
        x, y = gen(*SELF_CASES[name]), None
    x.setflags(write=False)
    if y is not None:
        y.setflags(write=False)
    return x, y


def distances_of(x, y=None):
    """int64 Hamming distances of packed rows; for a self-join (y None) everything but col > row is a distance no cutoff reaches"""
    h = hamming(x, x if y is None else y)
    if y is None:
        h[np.tril_indices(len(x))] = np.iinfo(np.int64).max
    return h


@functools.lru_cache(maxsize=None)
def distances(name):
    h = distances_of(*lists(name))
    h.setflags(write=False)
    return h


def rule_max_distance(d, t):
    """the rule itself, evaluated in numpy at every h: the largest h in [0, d] with float64(float32(d - 2 h) / float32(d)) >= t; -1: none"""
    h = np.arange(d + 1, dtype=np.int64)
    s = ((np.float32(d) - np.float32(2) * h.astype(np.float32)) / np.float32(d)).astype(np.float64)
    ok = np.nonzero(s >= t)[0]
    return int(ok[-1]) if len(ok) else -1


def oracle_pairs(h, hmax):
    """(rows, cols, distances) of the pairs with h <= hmax, row-major"""
    rows, cols = np.nonzero(h <= hmax)
    return rows, cols, h[rows, cols]


def oracle_counts(name, t):
    """(hmax, hits, pairs exactly at hmax) of the numpy oracle"""
    h, hmax = distances(name), rule_max_distance(bits(name), t)
    return hmax, int((h <= hmax).sum()), int((h == hmax).sum())


def oracle_components(name, t):
    rows, cols, _ = oracle_pairs(distances(name), rule_max_distance(bits(name), t))
    return len(np.unique(union_find_labels(len(lists(name)[0]), rows, cols)))


# ---- the device side, shared by the two GPU test files: resident handles and the joins computed once -----------------------
_cache = {}


def devs(ctx, name):
    """(from handle, to handle or None): the case's codes, resident"""
    from polyfuzz_amd import _lib
    if ("dev", name) not in _cache:
        x, y = lists(name)
        _cache["dev", name] = (_lib.DeviceDense.upload_bits(ctx, x), None if y is None else _lib.DeviceDense.upload_bits(ctx, y))
    return _cache["dev", name]


def join(ctx, name, t):
    """the join of a case at the distance HMAX names (computed once): (rows, cols, distances, row_ptr, counts)"""
    from polyfuzz_amd import _lib
    if ("join", name, t) not in _cache:
        f, to = devs(ctx, name)
        row_ptr, idx, dist, counts = _lib.hamming_join(ctx, f, to, HMAX[name][t], counters=True)
        rows, cols = csr_pairs(row_ptr, idx)
        _cache["join", name, t] = (rows, cols, dist, row_ptr, counts)
    return _cache["join", name, t]


def existing_path(ctx, f, to, hmax):
    """the way to the same pairs before K23: dense_topn on the two bit handles -- the whole score panel, every column ranked --
    with the filter `>` just below the score of hmax; (rows, cols, scores) by row, then column.  hmax < d / 2: the score is > 0."""
    from polyfuzz_amd import _lib
    self_join = to is None
    to = f if self_join else to
    s = _lib.hamming_similarity(np.array([hmax]), f.dim)[0]
    assert s > 0
    idx, val = _lib.dense_topn(ctx, f, to, to.n, float(np.nextafter(s, np.float32(-np.inf))), exclude_diag=self_join).download()
    rows, slot = np.nonzero(idx >= 0)
    cols, vals = idx[rows, slot], val[rows, slot]
    if self_join:
        keep = cols > rows
        rows, cols, vals = rows[keep], cols[keep], vals[keep]
    order = np.lexsort((cols, rows))
    return rows[order], cols[order], vals[order]
