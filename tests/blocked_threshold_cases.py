"""What the tests of K17 share (tests/test_blocked_threshold_gpu.py, tests/test_blocked_threshold_cpu.py): the lists of the cases,
each verified on the CPU with the float64 oracle vectoriser (oracle/tfidf_numpy.py) to have the K15 pairs it is there for, and the
definition of the join over a given pair list, restated on the host.  The oracle's cosines decide nothing the device could
disagree with: wherever a test needs a row to have EXACTLY so many partners, every intended pair is at least MARGIN above b and
every other pair at least MARGIN below it, a hundred times K3's documented error.  No tests here."""
import functools
import json
import os

import numpy as np

from tests import pairs_join_cases as P

HERE = os.path.dirname(os.path.abspath(__file__))
B = 0.5                  # the blocking similarity of the constructed cases
MARGIN = 1e-3


def _golden(name):
    with open(os.path.join(HERE, "golden", name + ".json")) as f:
        return json.load(f)


# ---- the float64 oracle's cosines ---------------------------------------------------------------------------------------------

def oracle_rows(fl, tl=None):
    """(from-rows, to-rows) as scipy CSR, fitted as TFIDF.match fits: on the to-list followed by the from-list, or on the one list"""
    import oracle
    from scipy.sparse import csr_matrix
    docs = list(fl) if tl is None else list(tl) + list(fl)
    o = oracle.tfidf_numpy.TfidfNumpyOracle((3, 3)).fit(docs)

    def rows(strings):
        indptr, cols, data = o.transform(list(strings))
        return csr_matrix((data, cols, indptr), shape=(len(strings), len(o.codes)))
    a = rows(fl)
    return a, a if tl is None else rows(tl)


def oracle_cosines(fl, tl=None):
    """dense float64 [len(fl), len(tl or fl)] (small lists only)"""
    a, b = oracle_rows(fl, tl)
    return np.asarray((a @ b.T).todense())


# ---- the definition, over a given pair list -----------------------------------------------------------------------------------

def expected_keys_join(sim, row_ptr, idx, t):
    """(row_ptr int64[n + 1], idx int32[hits], sim float64[hits]) of the pairs of the CSR (row_ptr, idx) -- K15's, every one a
    candidate -- whose score, matrix `sim` at [row, idx], is >= t"""
    n = len(row_ptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(row_ptr))
    s = sim[rows, idx.astype(np.int64)]
    hit = s >= np.float64(t)
    out = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows[hit], minlength=n), out=out[1:])
    return out, idx[hit].astype(np.int32), s[hit].astype(np.float64)


def items_of(row_ptr, S):
    """the work items of a pair list: the sum over the rows of ceil(partners / S)"""
    return int(((np.diff(row_ptr) + S - 1) // S).sum())


def padded_table(row_ptr, idx):
    """int32 [n, widest row]: the CSR's rows, -1 behind each"""
    per = np.diff(row_ptr)
    tab = np.full((len(per), max(1, int(per.max(initial=0)))), -1, np.int32)
    for i in range(len(per)):
        tab[i, :per[i]] = idx[row_ptr[i]:row_ptr[i + 1]]
    return tab


# ---- slices of the golden company names -----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def company_two_lists():
    """2 000 x 2 000 of the golden two-list case (test 1)"""
    g = _golden("company_c2_lists")
    return tuple(g["from_list"][:2000]), tuple(g["to_list"][:2000])


@functools.lru_cache(maxsize=None)
def company_self():
    return tuple(_golden("company_self_list")["from_list"])


def _unreached(fl, tl):
    """1.0 is a threshold no pair of the lists reaches: the oracle's largest cosine is MARGIN below it"""
    a, b = oracle_rows(fl, tl)
    p = (a @ b.T).tocoo()
    off = p.data if tl is not None else p.data[p.row != p.col]
    return float(off.max(initial=0.0)) < 1.0 - MARGIN


@functools.lru_cache(maxsize=None)
def company_two_lists_distinct():
    """the two-list slice without the to-strings some from-string equals or nearly equals, so that no pair reaches 1.0"""
    fl, tl = company_two_lists()
    a, b = oracle_rows(fl, tl)
    p = (a @ b.T).tocoo()
    drop = set(p.col[p.data >= 1.0 - 2 * MARGIN].tolist())
    tl = tuple(s for j, s in enumerate(tl) if j not in drop)
    assert len(tl) > 1900 and _unreached(fl, tl)
    return fl, tl


@functools.lru_cache(maxsize=None)
def company_self_distinct():
    strings = company_self()
    a, _ = oracle_rows(strings)
    p = (a @ a.T).tocoo()
    near = (p.data >= 1.0 - 2 * MARGIN) & (p.row < p.col)
    drop = set(p.col[near].tolist())
    out = tuple(s for j, s in enumerate(strings) if j not in drop)
    assert len(out) > 2000 and _unreached(out, None)
    return out


def _dense_slice(fl, tl, n_from, n_to):
    """the first n_from from-strings that have a partner at cosine >= 0.6 in the (larger) lists, with all their partners and other
    to-strings up to n_to: a slice small enough for the oracles' full matrices that still has pairs"""
    a, b = oracle_rows(fl, tl)
    p = (a @ (a if tl is None else b).T).tocoo()
    keep = (p.data >= 0.6) & ((p.row != p.col) if tl is None else True)
    rows = sorted(set(p.row[keep].tolist()))[:n_from]
    cols = sorted(set(p.col[keep][np.isin(p.row[keep], rows)].tolist()))
    return rows, cols


@functools.lru_cache(maxsize=None)
def small_two_lists():
    """~100 x ~200 (test 2, 3, 7, 8): (fl, tl, {scorer: oracle matrix}); at least 50 K15 pairs at b = 0.5 and no row beyond 64"""
    g = _golden("company_c2_lists")
    fl, tl = g["from_list"][:3000], g["to_list"][:3000]
    rows, cols = _dense_slice(fl, tl, 100, 200)
    more = [j for j in range(len(tl)) if j not in set(cols)][:max(0, 200 - len(cols))]
    fl, tl = [fl[i] for i in rows], [tl[j] for j in sorted(cols + more)]
    fl += ["", "a", "no partner here 0123456789"]
    cos = oracle_cosines(fl, tl)
    assert (cos >= B + MARGIN).sum() >= 50 and (cos >= B - MARGIN).sum(axis=1).max() <= 64
    return tuple(fl), tuple(tl), P.all_scores(P._oracle(), fl, tl)


@functools.lru_cache(maxsize=None)
def small_self():
    """~200 strings of the golden self-join list with their partners (test 2, 7, 8): (strings, {scorer: oracle matrix})"""
    s = list(company_self())
    rows, cols = _dense_slice(s, None, 45, 0)
    pick = sorted(set(rows) | set(cols))
    strings = [s[i] for i in pick] + s[:30] + ["", "a"]
    cos = oracle_cosines(strings)
    assert 150 <= len(strings) <= 330 and (np.triu(cos, 1) >= B + MARGIN).sum() >= 50
    return tuple(strings), P.all_scores(P._oracle(), strings, strings)


# ---- constructed lists: every row's partners are known ----------------------------------------------------------------------------

def _variants(rng, core, alpha, n):
    """n strings near `core` that hold no n-gram the core does not: its first 0 .. 3 and last 0 .. 3 characters dropped and, in two
    of three, a space put in at a place that goes round (the n-grams across a space are not counted).  A NEW n-gram would be a
    rare one, which weighs six times one that every variant shares: three of them sink the cosine of a short string below any b."""
    out = []
    for i in range(n):
        s = core[i % 4:len(core) - (i // 4) % 4]
        if (i // 16) % 3:
            k = 3 + (i // 48) % (len(s) - 5)
            s = s[:k] + " " + s[k:]
        out.append(s)
    return out


def border_sizes(S):
    return [0, 1, 63, 64, 65, S, S + 1, 2 * S, 2 * S + 1]


@functools.lru_cache(maxsize=None)
def borders(S):
    """two lists (test 4): nine from-strings over nine alphabets of four symbols each, from-string k with border_sizes(S)[k]
    variants of itself in the (shuffled) to-list and no n-gram in common with anybody else's -> (fl, tl, sizes, {scorer: matrix}).
    From-lengths 24 / 40 / 70 go round: 32-bit words, 64-bit words, the general kernel."""
    rng = np.random.default_rng(1701)
    symbols = "abcdefghijklmnopqrstuvwxyz0123456789"
    sizes = border_sizes(S)
    fl, tl, owner = [], [], []
    for k, size in enumerate(sizes):
        alpha = symbols[4 * k:4 * k + 4]
        core = "".join(rng.choice(list(alpha), size=(24, 40, 70)[k % 3]))
        fl.append(core)
        tl += _variants(rng, core, alpha, size)
        owner += [k] * size
    order = rng.permutation(len(tl))
    tl, owner = [tl[i] for i in order], np.array(owner)[order]
    cos = oracle_cosines(fl, tl)
    mine = owner[None, :] == np.arange(len(fl))[:, None]
    assert (cos[mine] >= B + MARGIN).all() and (cos[~mine] == 0.0).all()
    assert mine.sum(axis=1).tolist() == sizes and mine[-1].any()      # (the last row's range ends at the last key)
    return tuple(fl), tuple(tl), sizes, P.all_scores(P._oracle(), fl, tl)


@functools.lru_cache(maxsize=None)
def hub(position, length, S, long_partner=False):
    """one list (test 5): a hub of `length` characters over "abcdefgh", 2 S + 40 variants of it (2 S + 39 and, last of the list,
    fifteen copies of the hub in one string of 300 characters and more when long_partner), and 30 strings over digits that share no
    n-gram with them; the hub first or last -> (strings, position of the hub, its number of partners)"""
    rng = np.random.default_rng(1702 + length)
    alpha = "abcdefgh"
    core = "".join(rng.choice(list(alpha), size=length))
    n_var = 2 * S + 40 - (1 if long_partner else 0)
    near = _variants(rng, core, alpha, n_var)
    far = P.rand_strings(rng, "0123456789", 8, 30, 30)
    body = [near[i] for i in rng.permutation(n_var)]
    body = body[:100] + far + body[100:]
    if long_partner:
        assert position == "first"
        body.append(" ".join([core] * 15))
        assert len(body[-1]) >= 300
    strings = [core] + body if position == "first" else body + [core]
    h = 0 if position == "first" else len(strings) - 1
    cos = oracle_cosines(strings)[h]
    is_far = np.array([s in set(far) for s in strings])
    assert (cos[~is_far] >= B + MARGIN).all() and (cos[is_far] == 0.0).all() and (~is_far).sum() - 1 == 2 * S + 40
    return tuple(strings), h, 2 * S + 40


@functools.lru_cache(maxsize=None)
def copies():
    """test 9: 40 copies of one 12-character name mixed into 60 distinct names -> (names, positions of the copies)"""
    rng = np.random.default_rng(1703)
    others = P.rand_strings(rng, "bcdfghjklmnpqrstvwxyz", 9, 16, 60)
    name = "acme widgets"
    assert len(name) == 12 and len(set(others)) == 60
    names = others + [name] * 40
    order = rng.permutation(100)
    names = [names[i] for i in order]
    at = [i for i, s in enumerate(names) if s == name]
    cos = oracle_cosines(names)
    np.fill_diagonal(cos, 0.0)
    same = np.zeros((100, 100), bool)
    same[np.ix_(at, at)] = True
    np.fill_diagonal(same, False)
    assert (cos[same] >= 1.0 - 1e-9).all() and (cos[~same] <= 0.9 - MARGIN).all()
    return tuple(names), at
