"""Generators, rules restated and the pair oracle of the second-row and table-border tests (test_second_row_cpu.py,
test_second_row_gpu.py, test_indel_table_borders_gpu.py).  Everything is seeded; nothing is read from disk.

The general form of every edit-distance kernel keeps the from-string's match table in global memory and runs a capped grid of
persistent workgroups: a workgroup takes row r, then r + grid, on a table that is "zero on entry, zero again after every row".  A
list exercises the second half of that sentence only when it has more general rows than the grid has workgroups; the caps are
multiples of the compute-unit count, so every list here is sized by `n_cu` (the GPU tests read it from the context).

The joins of such lists have millions of pairs, far more than the numpy oracles can walk.  `survivors` leaves out a pair only when
an exact lower bound on its distance already puts its similarity below the threshold; `pair_lev` / `pair_lcs` walk the textbook
tables of the pairs that remain, many pairs per numpy step."""
import numpy as np

from tests import lev_oracle

LETTERS20 = "abcdefghijklmnopqrst"
K4_GRID_PER_CU, K7_GRID_PER_CU, JOIN_GRID_PER_CU, K10_GRID_PER_CU = 2, 2, 8, 32      # the caps of the general launches


def text(rng, n, alphabet=LETTERS20):
    a = np.array(list(alphabet))
    return "".join(a[rng.integers(0, len(a), int(n))])


def edited(rng, s, k, alphabet=LETTERS20):
    """s after k seeded edits: an insertion, a deletion, a swap of two neighbours or a replacement each"""
    s = list(s)
    for _ in range(int(k)):
        kind, at = int(rng.integers(4)), int(rng.integers(0, len(s) + 1))
        if kind == 0:
            s.insert(at, alphabet[int(rng.integers(len(alphabet)))])
        elif kind == 1 and len(s) > 1:
            del s[min(at, len(s) - 1)]
        elif kind == 2 and len(s) > 1:
            i = min(at, len(s) - 2)
            s[i], s[i + 1] = s[i + 1], s[i]
        elif s:
            s[min(at, len(s) - 1)] = alphabet[int(rng.integers(len(alphabet)))]
    return "".join(s)


def first_occurrence(strings):
    first = {}
    for j, s in enumerate(strings):
        first.setdefault(s, j)
    return np.array([first[s] for s in strings], np.int32)


# ---- K4: more from-strings than the general grid ----------------------------------------------------------------------------------

K4_EDGE_LENGTHS = (0, 64, 65, 128, 129)
WIDE_ALPHABET = "".join(chr(c) for c in list(range(0x4E00, 0x4E00 + 400)) + list(range(0x61, 0x75)))


def k4_lists(n_cu, wide=False, seed=701):
    """-> (from-list of 2 n_cu + 96 strings of 0 .. 130 characters, to-list of 256 strings of 0 .. 300 characters).  The to-list is
    128 strings, '' among them, followed by the same 128 in reverse order: every score is there twice and the index decides.  A
    from-string is a slice of a to-string after 0 .. 5 edits, so most LCS values are large; the lengths of K4_EDGE_LENGTHS are in
    the list's last 96 strings and in its first ones.  Twenty letters (8-bit symbols), or, wide, 420 code points of which every one
    is in the to-list (16-bit symbols)."""
    rng = np.random.default_rng(seed + int(wide))
    alpha = WIDE_ALPHABET if wide else LETTERS20
    uniq = [""] + [text(rng, n, alpha) for n in rng.integers(1, 301, 125)] + [text(rng, 300, alpha), text(rng, 130, alpha)]
    if wide:
        uniq[1], uniq[2] = alpha[:210], alpha[210:]
    tl = uniq + uniq[::-1]
    n = K4_GRID_PER_CU * n_cu + 96
    long_ones = [s for s in uniq if len(s) >= 130]

    def derived(length=None):
        src = uniq[int(rng.integers(len(uniq)))] if length is None else long_ones[int(rng.integers(len(long_ones)))]
        want = int(rng.integers(0, 131)) if length is None else length
        at = int(rng.integers(0, max(1, len(src) - want + 1)))
        s = edited(rng, src[at:at + want], rng.integers(0, 6), alpha)[:130]
        if length is not None:
            s = (s + src)[:length]
        return s
    fl = [derived() for _ in range(n)]
    for k, length in enumerate(K4_EDGE_LENGTHS):
        fl[3 + 7 * k] = derived(length)
        fl[n - 90 + 11 * k] = derived(length)
    return fl, tl


# ---- K11 / K12 / K13: more general rows than eight workgroups per compute unit ------------------------------------------------------

FAMILY_MIN, FAMILY_MAX, FAMILY_EDITS = 65, 93, 7
JOIN_THRESHOLDS = (0.9, 0.88)


def family_list(n_cu, seed=702):
    """-> (list, family number of every position).  8 n_cu + 256 strings of 65 .. 93 characters over twenty letters: families of
    four variants (0 .. 7 edits each) of one random base of 72 .. 86 characters, in a seeded order.  Longer than 64: every row is
    the general kernel's, with a table that fits LDS"""
    rng = np.random.default_rng(seed)
    n = JOIN_GRID_PER_CU * n_cu + 256
    assert n % 4 == 0
    out = []
    for _ in range(n // 4):
        base = text(rng, rng.integers(FAMILY_MIN + FAMILY_EDITS, FAMILY_MAX - FAMILY_EDITS + 1))
        out += [edited(rng, base, rng.integers(0, FAMILY_EDITS + 1)) for _ in range(4)]
    order = rng.permutation(n)
    return [out[k] for k in order], order // 4               # position p holds variant order[p], of family order[p] // 4


def _counts(strings):
    """(counts int16 [n, symbols], lengths int32 [n]): how often every character of the lists' alphabet is in every string"""
    alphabet = sorted({c for s in strings for c in s})
    col = {c: k for k, c in enumerate(alphabet)}
    out = np.zeros((len(strings), max(1, len(alphabet))), np.int16)
    for i, s in enumerate(strings):
        for c in s:
            out[i, col[c]] += 1
    return out, lev_oracle.lengths(strings)


def distance_bounds(fl, tl):
    """(length difference, surplus of the from-string, surplus of the to-string) int32 [len(fl), len(tl)] each: the two one-sided
    sums of per-character count differences.  Two exact lower bounds on the distance of every pair come from them (`lower_bounds`)"""
    both = list(fl) + list(tl)
    counts, lens = _counts(both)
    ca, cb = counts[:len(fl)], counts[len(fl):]
    la, lb = lens[:len(fl)], lens[len(fl):]
    more_a, more_b = np.empty((len(fl), len(tl)), np.int32), np.empty((len(fl), len(tl)), np.int32)
    for r0 in range(0, len(fl), 128):
        diff = ca[r0:r0 + 128, None, :] - cb[None, :, :]
        more_a[r0:r0 + 128] = np.clip(diff, 0, None).sum(axis=2)
        more_b[r0:r0 + 128] = np.clip(-diff, 0, None).sum(axis=2)
    return np.abs(la[:, None] - lb[None, :]).astype(np.int32), more_a, more_b


def lower_bounds(bounds, metric):
    """(length difference, bag distance).  Levenshtein and OSA: the bag distance is the LARGER of the two one-sided sums -- an
    insertion or a deletion lowers one of them by at most one, a replacement both, a transposition moves no count.  Indel knows
    insertions and deletions only, and each lowers the SUM of the two by exactly one: there the sum is the bound."""
    len_diff, more_a, more_b = bounds
    return len_diff, (more_a + more_b if metric == "indel" else np.maximum(more_a, more_b))


def best_possible(metric, bound, la, lb):
    """the similarity of a pair whose distance were `bound`, in the oracles' own float64 formula: division and subtraction are
    monotone, so a pair at a distance >= bound scores at most this"""
    if metric == "indel":
        s = (np.asarray(la, np.int64) + np.asarray(lb, np.int64))
        return np.where(s > 0, 1.0 - np.asarray(bound, np.float64) / np.where(s > 0, s, 1).astype(np.float64), 1.0)
    return lev_oracle.similarity(bound, la, lb)


def survivors(fl, tl, thr, metric, self_join=False, bounds=None):
    """bool [len(fl), len(tl)]: the pairs neither bound puts below thr (self_join: of the upper triangle only).  bounds: what
    distance_bounds(fl, tl) gave, where a caller keeps it between thresholds and metrics"""
    len_diff, bag = lower_bounds(distance_bounds(fl, tl) if bounds is None else bounds, metric)
    la, lb = lev_oracle.lengths(fl)[:, None], lev_oracle.lengths(tl)[None, :]
    keep = (best_possible(metric, len_diff, la, lb) >= thr) & (best_possible(metric, bag, la, lb) >= thr)
    if self_join:
        keep &= np.triu(np.ones(keep.shape, bool), 1)
    return keep


def _padded(strings, fill):
    width = max([len(s) for s in strings] + [1])
    out = np.full((len(strings), width), fill, np.int32)
    for i, s in enumerate(strings):
        out[i, :len(s)] = lev_oracle._codes(s)
    return out


def pair_lev(a_strings, b_strings, scorer):
    """int32 [pairs]: the Levenshtein / OSA distance of a_strings[p] against b_strings[p] -- lev_oracle.distance's table, row by
    row over all pairs at once (the dependency on the cell to the left is a running minimum, as in lev_oracle._rows)"""
    assert scorer in lev_oracle.SCORERS and len(a_strings) == len(b_strings)
    A, B = _padded(a_strings, -2), _padded(b_strings, -1)
    la, lb = lev_oracle.lengths(a_strings), lev_oracle.lengths(b_strings)
    P, LB = B.shape
    if P == 0:
        return np.zeros(0, np.int32)
    cell = np.int16 if LB + A.shape[1] < 32000 else np.int32
    ar = np.arange(LB + 1, dtype=cell)[None, :]
    prev, prev2, eq_prev = np.repeat(ar, P, axis=0), None, None
    out = np.where(la == 0, lb, 0).astype(np.int32)
    pick = np.arange(P)
    for i in range(1, int(la.max()) + 1):
        eq = B == A[:, i - 1:i]
        t = np.empty_like(prev)
        t[:, 0] = i
        np.minimum(prev[:, :-1] + (~eq).astype(cell), prev[:, 1:] + cell(1), out=t[:, 1:])
        if scorer == "osa" and i >= 2 and LB >= 2:
            tr = eq[:, :-1] & eq_prev[:, 1:]               # j = 2 .. LB: a[i-1] == b[j-2] and a[i-2] == b[j-1]
            np.copyto(t[:, 2:], np.minimum(t[:, 2:], prev2[:, :-2] + cell(1)), where=tr)
        t = np.minimum.accumulate(t - ar, axis=1) + ar
        done = la == i
        out[done] = t[pick[done], lb[done]]
        prev2, prev, eq_prev = prev, t, eq
    return out


def pair_lcs(a_strings, b_strings):
    """int32 [pairs]: the LCS length of a_strings[p] and b_strings[p] -- indel_oracle.lcs's table over all pairs at once"""
    assert len(a_strings) == len(b_strings)
    A, B = _padded(a_strings, -2), _padded(b_strings, -1)
    la, lb = lev_oracle.lengths(a_strings), lev_oracle.lengths(b_strings)
    P, LB = B.shape
    out = np.zeros(P, np.int32)
    if P == 0:
        return out
    prev = np.zeros((P, LB + 1), np.int16 if LB < 32000 else np.int32)
    pick = np.arange(P)
    for i in range(1, int(la.max()) + 1):
        t = prev.copy()
        np.copyto(t[:, 1:], prev[:, :-1] + 1, where=B == A[:, i - 1:i], casting="unsafe")
        prev = np.maximum.accumulate(t, axis=1)
        done = la == i
        out[done] = prev[pick[done], lb[done]]
    return out


def join_oracle(fl, tl, thr, metric, self_join=False, cache=None, bounds=None):
    """(row_ptr int64, idx int32, dist int32, sim float64) of the pairs with similarity >= thr, row-major, as the kernels' CSR:
    the pairs `survivors` leaves are walked, every other pair is absent because its bound says so.  metric: "levenshtein", "osa" or
    "indel" (dist = |a| + |b| - 2 lcs).  cache: a dict that keeps walked distances by (from-string, to-string, metric) between
    calls -- a distance depends on nothing else"""
    from tests import indel_oracle
    keep = survivors(fl, tl, thr, metric, self_join, bounds)
    i, j = np.nonzero(keep)
    cache = {} if cache is None else cache
    todo = sorted({(fl[a], tl[b]) for a, b in zip(i.tolist(), j.tolist())} - {k[:2] for k in cache if k[2] == metric})
    if todo:
        a_s, b_s = [p[0] for p in todo], [p[1] for p in todo]
        if metric == "indel":
            d = indel_oracle.distance(pair_lcs(a_s, b_s), lev_oracle.lengths(a_s), lev_oracle.lengths(b_s))
        else:
            d = pair_lev(a_s, b_s, metric)
        for p, v in zip(todo, d.tolist()):
            cache[(p[0], p[1], metric)] = v
    dist = np.array([cache[(fl[a], tl[b], metric)] for a, b in zip(i.tolist(), j.tolist())], np.int32).reshape(-1)
    la, lb = lev_oracle.lengths(fl)[i], lev_oracle.lengths(tl)[j]
    sim = best_possible(metric, dist, la, lb)               # (the formula of lev_oracle.similarity / indel_oracle.similarity at d)
    hit = sim >= thr
    i, j, dist, sim = i[hit], j[hit], dist[hit], sim[hit]
    row_ptr = np.zeros(len(fl) + 1, np.int64)
    np.cumsum(np.bincount(i, minlength=len(fl)), out=row_ptr[1:])
    return row_ptr, j.astype(np.int32), dist, sim


# ---- K7: more from-strings than the general grid -----------------------------------------------------------------------------------

K7_WORDS = ["new", "york", "mets", "braves", "the", "atlanta", "vs", "a", "bb", "inc", "llc", "co", "yankees", "red", "sox", "x", "of",
            "los", "angeles", "dodgers"]


def word_soup(rng, n):
    """n strings of 0 .. 6 words of K7_WORDS, one or two spaces between them, some with spaces around, some with one character
    replaced by 'q' (the recipe of test_fuzz_gpu.py's lists)"""
    out = []
    for _ in range(n):
        toks = list(rng.choice(K7_WORDS, size=int(rng.integers(0, 7))))
        s = (" " * int(rng.integers(1, 3))).join(toks)
        if rng.random() < 0.15:
            s = " " + s + "  "
        if rng.random() < 0.2 and s:
            p = int(rng.integers(0, len(s)))
            s = s[:p] + "q" + s[p + 1:]
        out.append(s)
    return out


def k7_lists(n_cu, seed=703):
    """-> (2 n_cu + 64 from-strings, 48 to-strings) of word soup; '' and one-token strings in the from-list's first and last rows"""
    rng = np.random.default_rng(seed)
    fl, tl = word_soup(rng, K7_GRID_PER_CU * n_cu + 64), word_soup(rng, 44) + ["", "mets", "new york mets", "york  new mets"]
    fl[0], fl[1], fl[-1], fl[-2], fl[-3] = "", "yankees", "", "dodgers", "new york mets"
    return fl, tl


# ---- K10: two general rows in one workgroup ------------------------------------------------------------------------------------------

K10_FROM, K10_CANDIDATES = 200, 8


def k10_lists(seed=704):
    """-> (200 from-strings, 120 to-strings, candidate table int32 [200, 8]).  The from-strings at the even positions are longer
    than 64 characters (the general kernel's), the others at most 64; every one is an edited piece of a to-string, and that
    to-string is among its eight distinct candidates"""
    rng = np.random.default_rng(seed)
    tl = [text(rng, n) for n in rng.integers(70, 200, 118)] + ["", text(rng, 300)]
    fl, tab = [], np.empty((K10_FROM, K10_CANDIDATES), np.int32)
    for i in range(K10_FROM):
        src = int(rng.integers(0, 118))
        want = int(rng.integers(66, 70)) if i % 2 == 0 else int(rng.integers(0, 65))
        s = edited(rng, tl[src][:want], rng.integers(0, 5))
        s = (s + tl[src])[:max(want, 65)] if i % 2 == 0 else s[:64]
        fl.append(s)
        others = rng.choice(np.setdiff1d(np.arange(len(tl)), [src]), K10_CANDIDATES - 1, replace=False)
        tab[i] = rng.permutation(np.concatenate([[src], others]))
    return fl, tl, tab


def k10_general_grid(n_from, n_general, n_cu, jaro):
    """the grid of K10's general launch: one workgroup per general row -- per from-row under Jaro, whose register kernels hand rows
    on -- capped at 32 per compute unit"""
    return min(n_general if n_general > 0 and not jaro else n_from, K10_GRID_PER_CU * n_cu)


def k10_rows_of_workgroups(n_from, grid):
    """workgroup b is dealt the from-rows b, b + grid, b + 2 grid, ... (row = b mod grid) and serves the general ones among them"""
    return [list(range(b, n_from, grid)) for b in range(grid)]


# ---- K4 at the sizes where a word class's match table stops fitting LDS ----------------------------------------------------------

K4_CLASS_MAX = (32, 64, 128, 256, 512, 1024)          # from-string length: the word class
K4_CLASS_WORD_BYTES = (4, 8, 16, 32, 64, 128)         # bytes of one symbol's table entry in that class
K4_LDS_BYTES = 60 * 1024
K4_QUAD_ENTRY_BYTES = 16                              # the quad / octo kernels: one 128-bit entry per symbol
K4_BORDERS = (479, 480, 959, 960, 1919, 1920, 3839, 3840, 7679, 7680, 15359, 15360)
BORDER_FROM_LENGTHS = (0, 1, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025)


def k4_class(length):
    c = 0
    while c < 6 and length > K4_CLASS_MAX[c]:
        c += 1
    return c                                           # 6: beyond 1 024 characters, the general kernel whatever the alphabet


def k4_general_rows(lengths, n_sym):
    """how many of the from-strings K4 sends to the general kernel: the class beyond 1 024 characters, and every class whose table
    of n_sym + 1 entries is larger than 60 KiB"""
    return sum(1 for m in lengths if k4_class(m) == 6 or (n_sym + 1) * K4_CLASS_WORD_BYTES[k4_class(m)] > K4_LDS_BYTES)


def k4_quad_launches(lengths, n_sym):
    """launches of the quad / octo kernels of ONE arg-max call (no matrix, no top-n): eight from-strings of <= 16 characters per
    pass in one launch, four of 17 .. 32 in another -- while the 32-bit class keeps its rows and 16 bytes per symbol fit LDS"""
    if (n_sym + 1) * K4_CLASS_WORD_BYTES[0] > K4_LDS_BYTES or (n_sym + 1) * K4_QUAD_ENTRY_BYTES > K4_LDS_BYTES:
        return 0
    return int(any(m <= 16 for m in lengths)) + int(any(16 < m <= 32 for m in lengths))


def border_hot_count(n_sym):
    """strings over the hot symbols in the to-list: 40, and more where the 64-character strings alone would outnumber them -- a
    from-string shares a symbol with few of those, and more than half of the score matrix has to be non-zero"""
    return max(40, (5 * ((n_sym + 63) // 64) + 3) // 4)


def border_lists(n_sym, seed=705):
    """-> (from-list, to-list, hot symbols) for an alphabet of exactly n_sym code points.  The to-list: ceil(n_sym / 64) strings of 64
    characters that use every code point (the last one filled up with hot symbols), then border_hot_count strings of 1 .. 600
    characters over a dozen hot symbols.  The from-list: two strings per length of BORDER_FROM_LENGTHS, pieces of to-strings and runs
    of hot symbols in turn."""
    rng = np.random.default_rng(seed + n_sym)
    cps = [chr(0x4E00 + k) for k in range(n_sym)]
    hot = "".join(cps[(k * n_sym) // 12] for k in range(12))
    base = ["".join(cps[k:k + 64]) for k in range(0, n_sym, 64)]
    base[-1] = (base[-1] + text(rng, 64, hot))[:64]
    n_hot = border_hot_count(n_sym)
    hot_lens = [1, 600] + [int(x) for x in rng.integers(1, 601, n_hot - 2)]
    tl = base + [text(rng, n, hot) for n in hot_lens]

    def mixed(length):
        s = ""
        while len(s) < length:
            src = tl[int(rng.integers(len(tl)))]
            at, n = int(rng.integers(0, len(src))), int(rng.integers(4, 33))
            s += src[at:at + n] + text(rng, rng.integers(2, 24), hot)
        return s[:length]
    fl = [mixed(n) for n in BORDER_FROM_LENGTHS for _ in range(2)]
    return fl, tl, hot
