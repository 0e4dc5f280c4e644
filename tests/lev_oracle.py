"""The definition K9 is held to: rapidfuzz's Levenshtein.normalized_similarity / OSA.normalized_similarity with their default
arguments, restated on Unicode code points.  d = the Wagner-Fischer table with unit costs; "osa" adds the transposition of two
adjacent characters (optimal string alignment: no substring edited twice); sim = 1.0 - d / max(|a|, |b|) in float64, 1.0 for two
empty strings.  `distance` is the table in plain Python; `matrix` is the same table, one from-string against many to-strings per
numpy row step (tests/test_levenshtein_cpu.py holds the two to each other).  PARITY UNPINNED: rapidfuzz is not importable where
this was written; tests/test_levenshtein_cpu.py compares with it wherever it is.  Test code only -- the package never imports
this module."""
import numpy as np

SCORERS = ("levenshtein", "osa")


def distance(a, b, scorer):
    """the textbook table, plain Python"""
    assert scorer in SCORERS
    la, lb = len(a), len(b)
    D = [[0] * (lb + 1) for _ in range(la + 1)]
    for i in range(la + 1):
        D[i][0] = i
    for j in range(lb + 1):
        D[0][j] = j
    for i in range(1, la + 1):
        for j in range(1, lb + 1):
            v = min(D[i - 1][j] + 1, D[i][j - 1] + 1, D[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
            if scorer == "osa" and i >= 2 and j >= 2 and a[i - 1] == b[j - 2] and a[i - 2] == b[j - 1]:
                v = min(v, D[i - 2][j - 2] + 1)
            D[i][j] = v
    return D[la][lb]


def _codes(s):
    return np.frombuffer(s.encode("utf-32-le", "surrogatepass"), np.uint32).astype(np.int32)


def _chunks(to_list):
    """the to-strings sorted by length, cut where a chunk would pad its short strings to more than about twice their length:
    [(original indices, code points [L, n] -- one to-string per COLUMN, padded with -1 --, lengths [n])]"""
    lens = np.array([len(s) for s in to_list], np.int64)
    order = np.argsort(lens, kind="stable")
    out, k = [], 0
    while k < len(order):
        lo = int(lens[order[k]])
        e = k
        while e < len(order) and e - k < 4096 and lens[order[e]] <= 2 * lo + 8:
            e += 1
        idx = order[k:e]
        L = int(lens[idx].max())
        B = np.full((L, len(idx)), -1, np.int32)
        for r, j in enumerate(idx):
            B[:lens[j], r] = _codes(to_list[j])
        out.append((idx, B, lens[idx]))
        k = e
    return out


def _prefix_min(t, spare):
    """np.minimum.accumulate(t, axis=0) by doubling: whole-row minima of [j, to-string] arrays, seven of them for a hundred
    positions, where numpy's own scan along the first axis takes one short step per position.  Returns the result, which is `t` or
    `spare` (same shape; the two take turns, so that no step reads what it writes)"""
    s = 1
    while s < len(t):
        np.minimum(t[s:], t[:-s], out=spare[s:])
        spare[:s] = t[:s]
        t, spare = spare, t
        s *= 2
    return t


def _rows(ac, B, lens, osa):
    """the last table cell of from-string `ac` (code points) against every column of B: the table row by row (i) over all
    to-strings at once, a table row being the array [j, to-string]; the dependency on the cell to the left,
    D[i][j] = min(t[j], D[i][j-1] + 1), is min over k <= j of t[k] + (j - k)"""
    L, n = B.shape
    cell = np.int16 if L + len(ac) < 32000 else np.int32
    ar = np.arange(L + 1, dtype=cell)[:, None]
    rows = [np.empty((L + 1, n), cell) for _ in range(4)]  # D[i], D[i-1], D[i-2] and a spare (no allocation per row step)
    eqs = [np.empty((L, n), bool) for _ in range(2)]
    ne, tmp = np.empty((L, n), bool), np.empty((L, n), cell)
    prev = rows[0]
    prev[:] = ar                                           # D[0][j] = j
    prev2 = eq_prev = None
    for i in range(1, len(ac) + 1):
        np.not_equal(B, ac[i - 1], out=ne)                 # ne[j - 1]: a[i-1] != b[j-1]
        t, spare = [r for r in rows if r is not prev and r is not prev2][:2]
        t[0] = i
        np.add(prev[:-1], ne, out=t[1:])                   # substitute or keep
        np.add(prev[1:], cell(1), out=tmp)
        np.minimum(t[1:], tmp, out=t[1:])
        eq = eqs[i % 2]
        np.logical_not(ne, out=eq)
        if osa and i >= 2 and L >= 2:
            tr = eq[:-1] & eq_prev[1:]                     # j = 2 .. L: a[i-1] == b[j-2] and a[i-2] == b[j-1]
            cand = tmp[:-1]
            np.add(prev2[:-2], cell(1), out=cand)
            np.minimum(t[2:], cand, out=cand)
            np.copyto(t[2:], cand, where=tr)
        t -= ar
        t = _prefix_min(t, spare)
        t += ar
        prev2, prev, eq_prev = prev, t, eq
    return prev[lens, np.arange(n)]


def matrix(from_list, to_list, scorer, workers=1):
    """every distance, int32 [len(from_list), len(to_list)]; equal from-strings are walked once; workers: threads over the
    from-strings (numpy lets go of the interpreter lock inside a row step)"""
    assert scorer in SCORERS
    out = np.empty((len(from_list), len(to_list)), np.int32)
    chunks = _chunks(to_list)
    first = {}
    for i, a in enumerate(from_list):
        first.setdefault(a, i)

    def walk(i):
        ac = _codes(from_list[i])
        for idx, B, lens in chunks:
            out[i, idx] = _rows(ac, B, lens, scorer == "osa")
    todo = sorted(first.values())
    if workers > 1 and len(todo) > 1:
        import concurrent.futures as cf
        with cf.ThreadPoolExecutor(workers) as ex:
            list(ex.map(walk, todo))
    else:
        for i in todo:
            walk(i)
    for i, a in enumerate(from_list):
        if first[a] != i:
            out[i] = out[first[a]]
    return out


def lengths(strings):
    return np.array([len(s) for s in strings], np.int32)


def similarity(d, la, lb):
    """1.0 - d / max(la, lb) in float64 (one division, one subtraction), 1.0 where both lengths are 0; arrays broadcast"""
    d, m = np.asarray(d, np.float64), np.maximum(np.asarray(la), np.asarray(lb)).astype(np.float64)
    return np.where(m > 0, 1.0 - d / np.where(m > 0, m, 1.0), 1.0)


def sim_matrix(from_list, to_list, d):
    return similarity(d, lengths(from_list)[:, None], lengths(to_list)[None, :])


def left_out(n_to, skip):
    """[n, n_to] bool: the skip codes of the best-choice kernels, as tests/jaro_oracle.py reads them -- skip >= 0 leaves that
    choice out, skip <= -2 every choice up to -2 - skip, -1 nothing"""
    j = np.arange(n_to, dtype=np.int64)[None, :]
    sk = np.asarray(skip).astype(np.int64)[:, None]
    return (j == sk) | (j <= -2 - sk)


def argmax(sim, skip=None):
    """(first arg-max int32[n], score float64[n]) of a similarity matrix as np.argmax gives it (reference _distance.py:97-100) over
    the choices `skip` leaves in; a row without a choice gets -1 / 0.0"""
    n, n_to = sim.shape
    if n_to == 0:
        return np.full(n, -1, np.int32), np.zeros(n)
    out = np.zeros(sim.shape, bool) if skip is None else left_out(n_to, skip)
    mm = np.where(out, -1.0, sim)                          # (similarities are >= 0)
    idx = mm.argmax(axis=1).astype(np.int32)
    score = mm[np.arange(n), idx]
    none = out.all(axis=1)
    idx[none], score[none] = -1, 0.0
    return idx, score
