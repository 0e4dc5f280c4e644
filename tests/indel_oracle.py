"""The definition K13 is held to: rapidfuzz.distance.Indel.normalized_similarity with its default arguments, restated on Unicode
code points.  lcs = the textbook longest-common-subsequence table; S = |a| + |b|; d = S - 2 lcs; sim = 1.0 - d / S in float64 (one
division, one subtraction), 1.0 for two empty strings.  rapidfuzz.fuzz.ratio is (1.0 - d / S) * 100.0: tests/test_indel_join_cpu.py
pins this module to oracle/indel.c through that.  `lcs` is the table in plain Python; `lcs_matrix` is the same table, one
from-string against many to-strings per numpy row step, as tests/lev_oracle.py walks its table.  Test code only -- the package never
imports this module."""
import numpy as np

from tests.lev_oracle import _chunks, _codes, left_out, lengths  # noqa: F401  (lengths and left_out are part of this module's surface)


def lcs(a, b):
    """the textbook table, plain Python"""
    L = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            L[i][j] = L[i - 1][j - 1] + 1 if a[i - 1] == b[j - 1] else max(L[i - 1][j], L[i][j - 1])
    return L[len(a)][len(b)]


def _rows(ac, B, lens):
    """the last table cell of from-string `ac` (code points) against every ROW of B ([to-string, j], padded with -1): the table
    row by row (i) over all to-strings at once; the dependency on the cell to the left, L[i][j] = max(t[j], L[i][j-1]) with
    t[j] = L[i-1][j-1] + 1 where a[i-1] == b[j-1] and L[i-1][j] elsewhere, is a running maximum along j"""
    n, width = B.shape
    prev = np.zeros((n, width + 1), np.int32)
    for c in ac:
        t = prev.copy()
        np.copyto(t[:, 1:], prev[:, :-1] + 1, where=B == c)
        prev = np.maximum.accumulate(t, axis=1)
    return prev[np.arange(n), lens]


def lcs_matrix(from_list, to_list):
    """every LCS length, int32 [len(from_list), len(to_list)]; equal from-strings are walked once"""
    out = np.empty((len(from_list), len(to_list)), np.int32)
    chunks = [(idx, np.ascontiguousarray(B.T), lens) for idx, B, lens in _chunks(to_list)]
    first = {}
    for i, a in enumerate(from_list):
        first.setdefault(a, i)
    for i in sorted(first.values()):
        ac = _codes(from_list[i])
        for idx, B, lens in chunks:
            out[i, idx] = _rows(ac, B, lens)
    for i, a in enumerate(from_list):
        if first[a] != i:
            out[i] = out[first[a]]
    return out


def distance(lcs_len, la, lb):
    """the Indel distance |a| + |b| - 2 lcs, int32; arrays broadcast"""
    return (np.asarray(la, np.int64) + np.asarray(lb, np.int64) - 2 * np.asarray(lcs_len, np.int64)).astype(np.int32)


def similarity(lcs_len, la, lb):
    """1.0 - (S - 2 lcs) / S in float64 (one division, one subtraction), 1.0 where S = la + lb is 0; arrays broadcast"""
    s = np.asarray(la, np.int64) + np.asarray(lb, np.int64)
    d = (s - 2 * np.asarray(lcs_len, np.int64)).astype(np.float64)
    return np.where(s > 0, 1.0 - d / np.where(s > 0, s, 1).astype(np.float64), 1.0)


def sim_matrix(from_list, to_list, lcs_len):
    return similarity(lcs_len, lengths(from_list)[:, None], lengths(to_list)[None, :])
