"""What the tests of K16 (pfz_pairs_join / pfz_pairs_components, BlockedEditDistance.join / .components) share: the definition of
the candidate pairs of a table and of the join over them, restated on the host from include/polyfuzz_hip.h; the labels of a graph by
a union-find; and the lists and tables of the cases, built once per session with the oracles' scores (tests/lev_oracle.py,
oracle/jaro.c).  No tests here."""
import functools

import numpy as np

from tests import lev_oracle

FOUR = ("levenshtein", "osa", "jaro", "jaro_winkler")
THRESHOLDS = (0.0, 0.5, 0.8, 1.0)


# ---- the definition ------------------------------------------------------------------------------------------------------------

def candidate_pairs(cand, n_to, self_join):
    """(i int64[p], j int64[p], cells): the distinct candidate pairs of table `cand` (int [n, m]) in (i, j) order, and the number of
    table cells that are one.  A cell outside [0, n_to) is none; an index listed twice in a row counts once.  self_join: a row's own
    index is none, and the pairs are the unordered {i, j} of the symmetrised table, as (min, max)."""
    n, m = cand.shape
    rows, cols = np.repeat(np.arange(n, dtype=np.int64), m), cand.reshape(-1).astype(np.int64)
    ok = (cols >= 0) & (cols < n_to)
    if self_join:
        ok &= cols != rows
    i, j = rows[ok], cols[ok]
    if self_join:
        i, j = np.minimum(i, j), np.maximum(i, j)
    key = np.unique(i * n_to + j)
    return key // n_to, key % n_to, int(ok.sum())


def expected_join(sim, cand, t, self_join):
    """(row_ptr int64[n + 1], idx int32[hits], sim float64[hits], counts) of the candidate pairs of `cand` whose score -- oracle
    matrix `sim` at [i, j], in a self-join at [min, max] -- is >= t; counts as _lib.PAIR_JOIN_COUNTERS names them"""
    n, n_to = sim.shape
    i, j, cells = candidate_pairs(cand[:n], n_to, self_join)
    s = sim[i, j]
    hit = s >= np.float64(t)
    row_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(i[hit], minlength=n), out=row_ptr[1:])
    return row_ptr, j[hit].astype(np.int32), s[hit].astype(np.float64), {"candidates": cells, "scored": len(i), "pairs": int(hit.sum())}


def expected_labels(n, row_ptr, idx):
    """int32[n]: the smallest position in every position's component of the graph whose edges are the CSR's pairs"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i in range(n):
        for j in idx[row_ptr[i]:row_ptr[i + 1]].tolist():
            a, b = find(i), find(j)
            parent[max(a, b)] = min(a, b)
    return np.array([find(x) for x in range(n)], np.int32)


def frame_of(from_list, names, row_ptr, idx, sim):
    import pandas as pd
    frm = np.repeat(np.arange(len(from_list)), np.diff(row_ptr))
    return pd.DataFrame({"From": [from_list[i] for i in frm], "To": [names[j] for j in idx], "Similarity": sim})


def all_scores(oracle_mod, fl, tl):
    """{scorer: float64 [len(fl), len(tl)]} of the four join scorers, from the oracles"""
    out = {name: lev_oracle.sim_matrix(fl, tl, lev_oracle.matrix(fl, tl, name, workers=4)) for name in lev_oracle.SCORERS}
    for name in ("jaro", "jaro_winkler"):
        out[name] = oracle_mod.jaro_matrix(fl, tl, name)
    return out


# ---- strings and tables (the recipe of tests/test_pairs_rescore_gpu.py, restated) ------------------------------------------------

def rand_strings(rng, alpha, lo, hi, n):
    return ["".join(rng.choice(list(alpha), size=int(rng.integers(lo, hi + 1)))) for _ in range(n)]


def swapped(rng, s, k):
    """`s` with k transpositions of two adjacent, different characters at places that do not touch"""
    s, free = list(s), set(range(len(s) - 1))
    for _ in range(k):
        ok = [i for i in sorted(free) if s[i] != s[i + 1]]
        if not ok:
            break
        i = ok[int(rng.integers(len(ok)))]
        s[i], s[i + 1] = s[i + 1], s[i]
        free -= {i - 1, i, i + 1}
    return "".join(s)


def random_table(rng, n, n_to, m, duplicates=True):
    """int32 [n, m]: per row a random number (0 .. min(m, n_to); the first rows none, the next ones as many as fit) of distinct
    to-indices at random places, -1 / n_to / -7 everywhere else; duplicates: every third row with a junk cell gets one of its own
    indices a second time there"""
    tab = rng.choice(np.array([-1, -1, n_to, -7], np.int32), size=(n, m))
    for i in range(n):
        k = 0 if i < 3 else (min(m, n_to) if i < 8 else int(rng.integers(0, min(m, n_to) + 1)))
        tab[i, rng.choice(m, k, replace=False)] = rng.choice(n_to, k, replace=False)
        junk = np.flatnonzero((tab[i] < 0) | (tab[i] >= n_to))
        if duplicates and i % 3 == 0 and 0 < len(junk) < m:
            tab[i, junk[0]] = tab[i, np.flatnonzero((tab[i] >= 0) & (tab[i] < n_to))[0]]
    return tab


def device_table(ctx, tab):
    from polyfuzz_amd import _lib
    return _lib.DeviceTopN.from_host(ctx, np.ascontiguousarray(tab, np.int32), np.zeros(tab.shape, np.float32))


BASE = "the quick brown fox jumps over the lazy dog and runs far away from home again"


def _golden():
    import json
    import os
    g = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    out = {}
    for name in ("titles_lists", "titles_self_list"):
        with open(os.path.join(g, name + ".json")) as f:
            out[name] = json.load(f)
    return out


def _oracle():
    import oracle
    oracle.build_native()
    return oracle


@functools.lru_cache(maxsize=None)
def mixed():
    """~120 x 250, two lists: (fl, tl, {scorer: oracle matrix}, {m: table}).  From-lengths {0, 1, 31, 32, 33, 63, 64, 65, 100-200},
    to-lengths {0, 1, 255, 256, 257, 1000}, 8-bit, 16-bit and astral symbols, every to-string present twice; tables with junk
    cells and, in some rows, a duplicated index."""
    rng = np.random.default_rng(1601)
    t = _golden()["titles_lists"]
    edge = [31, 32, 33, 63, 64, 65]
    cut = lambda: BASE[:int(rng.integers(24, 65))]
    fl = (t["from_list"][:16] + ["", "a", "ab", "CA", "the matrix", "Z"] + [BASE[:n] for n in edge] + [BASE[::-1][:n] for n in edge] +
          ["ab" * 100, "naïve café Ωmega \U0001f600 smile", "qqq中文", "####", "\U0001f600\U0001f601"] + rand_strings(rng, "ab", 1, 70, 30) +
          ["ab" * k for k in (1, 16, 17, 32, 33)] + ["abba" * 6, "baab" * 9] + rand_strings(rng, "abcdefgh ", 60, 66, 4) +
          rand_strings(rng, "abcdefgh ", 100, 200, 3) + [swapped(rng, cut(), int(rng.integers(1, 6))) for _ in range(37)])
    uniq = (t["to_list"][:20] + ["", "a", "ba", "ABC", "the matrix", "The Matrix"] + [BASE[:n] for n in edge] + [BASE[3:3 + n] for n in edge] +
            ["ba" * 75, "naïve cafe Ωmega \U0001f601 smile \U0001f600", "中文qqq"] + [(BASE * 4)[:n] for n in (255, 256, 257)] + [(BASE * 14)[:1000]] +
            rand_strings(rng, "ab", 1, 70, 24) + ["ba" * k for k in range(1, 8)] + ["ab" * k + "ba" * k for k in range(1, 6)] +
            rand_strings(rng, "abcdefgh ", 60, 66, 5) + rand_strings(rng, "abc", 1, 9, 8) +
            [swapped(rng, cut(), int(rng.integers(1, 6))) for _ in range(36)])
    tl = uniq + uniq[::-1]
    n, n_to = len(fl), len(tl)
    assert 110 <= n <= 130 and 230 <= n_to <= 270
    assert {0, 1, 31, 32, 33, 63, 64, 65, 200} <= set(map(len, fl)) and any(100 <= len(s) < 200 for s in fl)
    assert {0, 1, 255, 256, 257, 1000} <= set(map(len, tl))
    assert max(map(ord, "".join(tl))) > 0xFFFF and any(255 < ord(c) <= 0xFFFF for c in "".join(tl))
    tables = {m: random_table(rng, n, n_to, m) for m in (1, 5, 64, 65, 130)}
    for m, tab in tables.items():
        if m > 1:      # junk cells of all three kinds, and rows that list an index twice
            assert all((tab == v).any() for v in (-1, -7, n_to))
            assert any(len(np.unique(r[(r >= 0) & (r < n_to)])) < ((r >= 0) & (r < n_to)).sum() for r in tab)
    sims = all_scores(_oracle(), fl, tl)
    # no threshold passes vacuously: from the oracle alone
    for name in FOUR:
        for m, tab in tables.items():
            for t_ in (0.5, 0.8):
                c = expected_join(sims[name], tab, t_, False)[3]
                assert 0 < c["pairs"] < c["scored"] <= c["candidates"] and (m == 1 or c["scored"] < c["candidates"]), (name, m, t_, c)
    return fl, tl, sims, tables


@functools.lru_cache(maxsize=None)
def self_list():
    """~200 strings with repeats and one table of 8 columns for the self-join: (strings, {scorer: oracle matrix}, table).  The table
    has pairs listed in both rows, pairs listed only in the higher row, rows that list their own index, duplicates within a row and
    junk; among the pairs are long (65+: general kernel) lower positions with short higher ones and the reverse, and short
    strings with a partner beyond 256 characters (Jaro's border)."""
    rng = np.random.default_rng(1602)
    t = _golden()["titles_self_list"]["from_list"]
    cut = lambda lo, hi: BASE[:int(rng.integers(lo, hi))]
    seeds = (t[:30] + ["", "a", "ab", "the matrix", BASE[:31], BASE[:32], BASE[:33], BASE[:63], BASE[:64]] +
             [swapped(rng, cut(24, 65), 2) for _ in range(21)])                                       # 60 short ones
    longs = [BASE[:65], (BASE * 2)[:100], (BASE * 3)[:200], (BASE * 4)[:257], (BASE * 4)[:300], "naïve café Ωmega \U0001f600 " * 4]
    strings = (longs + seeds + [swapped(rng, s, 1) for s in seeds] + seeds[:40] + [s[:70] + "!" for s in longs] +
               [swapped(rng, (BASE * 4)[:260], 3), BASE[:40]] + seeds[40:] + rand_strings(rng, "abc", 1, 9, 6))
    n = len(strings)
    assert 190 <= n <= 210 and len(set(strings)) < n - 50
    m = 8
    tab = rng.choice(np.array([-1, n, -7], np.int32), size=(n, m))
    cells = rng.random((n, m)) < 0.6
    tab[cells] = rng.integers(0, n, int(cells.sum()))                          # with replacement: duplicates and own indices occur
    first = lambda s: strings.index(s)
    both = [(6 + k, 66 + k) for k in range(0, 60, 3)]                          # a seed and its variant: listed in both rows
    high = [(6 + k, 126 + k) for k in range(0, 40, 2)]                         # a seed and its repeat: only the higher row lists it
    long_low = [(0, first(BASE[:40])), (2, 6 + 38), (3, first(BASE[:32])), (4, 6 + 34)]          # long lower, short higher
    short_high_long = [(6 + 34, 172), (6 + 35, 172), (6 + 36, 166), (6 + 37, 170)]      # short lower, long (beyond 256 / 64) higher
    for i, j in both:
        tab[i, 0], tab[j, 1] = j, i
    for i, j in high + long_low + short_high_long:
        assert i < j
        tab[i][tab[i] == j] = -1
        tab[j, 2] = i
    for i in range(0, n, 7):
        tab[i, 3] = i                                                          # the row's own index
    for i in range(3, n, 5):
        tab[i, 5] = tab[i, 4] = (i * 31 + 7) % n                               # a duplicate within the row
    tab[n - 1, 6], tab[0, 6] = 0, n - 1
    lens = np.array([len(s) for s in strings])
    lists = lambda i, j: (tab[i] == j).any()
    assert all(lists(i, j) and lists(j, i) for i, j in both) and all(lists(j, i) and not lists(i, j) for i, j in high)
    assert any(lens[i] > 64 >= lens[j] for i, j in long_low) and any(lens[i] <= 64 < lens[j] for i, j in short_high_long)
    assert any(lens[i] <= 64 and lens[j] > 256 for i, j in short_high_long), [(lens[i], lens[j]) for i, j in short_high_long]
    sims = all_scores(_oracle(), strings, strings)
    for name in FOUR:
        for t_ in (0.5, 0.8):
            c = expected_join(sims[name], tab, t_, True)[3]
            assert 0 < c["pairs"] < c["scored"] < c["candidates"], (name, t_, c)
    return strings, sims, tab


@functools.lru_cache(maxsize=None)
def hub(position, length):
    """m = 5; one string (of `length` characters; position "first" or "last") that 70 other rows list while its own row lists
    two: (strings, {scorer: oracle matrix}, table).  After the symmetrisation the hub has 72 partners: with the hub first, its
    row has a second chunk of lanes."""
    rng = np.random.default_rng(1603 + length)
    core = (BASE * 2)[:length]
    others = [swapped(rng, core, int(rng.integers(0, 4)))[:int(rng.integers(max(1, length - 6), length + 1))] for _ in range(60)] + \
             rand_strings(rng, "abcdefgh ", max(1, length - 10), length + 10, 24)
    strings = [core] + others if position == "first" else others + [core]
    n = len(strings)
    h = 0 if position == "first" else n - 1
    rest = [i for i in range(n) if i != h]
    tab = np.full((n, 5), -1, np.int32)
    for i in rest:
        k = int(rng.integers(1, 4))
        tab[i, :k] = rng.choice(rest, k, replace=False)
    for i in rest[:70]:
        tab[i, int(rng.integers(0, 5))] = h
    tab[h, 1], tab[h, 3] = rest[75], rest[80]
    assert (tab == h).any(axis=1).sum() == 70 and not (tab[rest[75]] == h).any() and not (tab[rest[80]] == h).any()
    i, j, _ = candidate_pairs(tab, n, True)
    assert ((i == h) | (j == h)).sum() == 72 and (position != "first" or (i == 0).sum() == 72)
    return strings, all_scores(_oracle(), strings, strings), tab


@functools.lru_cache(maxsize=None)
def titles_self():
    """the 400 titles with repeats of tests/test_pairs_rescore_gpu.py's `titles` and their oracle matrices"""
    g = _golden()
    dup = (g["titles_lists"]["to_list"] + g["titles_self_list"]["from_list"])[:400]
    assert len(dup) == 400
    return dup, all_scores(_oracle(), dup, dup)
