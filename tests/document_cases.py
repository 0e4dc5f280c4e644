"""Generators and the acceptance rule of the document tests (test_documents_cpu.py, test_documents_gpu.py): strings of thousands
of characters for K1/K2, CSR rows of thousands of entries for K3.  Everything is seeded; nothing is read from disk.

K3's contract on such rows.  Every product a*b is truncated to a multiple of 1/S (S = 2^30 / norm bound), so a score is at most
one such step too low PER SHARED COLUMN: |score - exact| <= c * 2^-30 * (norm bound) + 3e-7 for a pair with c columns in common
(`k3_bound`).  The company names the other tests use share about 13; a document shares thousands, and 1e-5 holds up to about
10 000 of them."""
import numpy as np

from tests.helpers import NEAR_TIE, random_csr

LETTERS = "abcdefghijklmnopqrstuvwxyz"


# ---- strings -----------------------------------------------------------------------------------------------------------------------

def doc(rng, n_chars, alphabet=LETTERS):
    """random text of n_chars characters over `alphabet`"""
    a = np.array(list(alphabet))
    return "".join(a[rng.integers(0, len(a), int(n_chars))])


def edited(rng, s, share, alphabet=LETTERS):
    """s with that share of its characters replaced, at random places, by another character of `alphabet`"""
    c = list(s)
    k = max(1, int(round(share * len(c))))
    for p in rng.choice(len(c), size=k, replace=False).tolist():
        others = [x for x in alphabet if x != c[p]]
        c[p] = others[int(rng.integers(0, len(others)))]
    return "".join(c)


def doc_with_singleton_ends(rng, n_chars):
    """letters b .. y at random between "aaa" and "zzz": the document's smallest and largest 3-gram occur once each, so the first
    and the last key of its sorted n-grams are runs of one"""
    return "aaa" + doc(rng, n_chars - 6, LETTERS[1:25]) + "zzz"


def short_names(rng, n, alphabet=LETTERS):
    """n names of one to four words of 2 .. 9 characters"""
    out = []
    for _ in range(n):
        out.append(" ".join(doc(rng, int(rng.integers(2, 10)), alphabet) for _ in range(int(rng.integers(1, 5)))))
    return out


def splice(names, docs):
    """`names` with `docs` at the first row, at the last row and spread inside; beside the first three of them an empty string and
    a one-character string, so that the three sit in one group of four consecutive rows (index 4k .. 4k + 3)"""
    n = len(docs)
    if n == 0:
        return list(names)
    out = [docs[0], "", "b"] + list(names)
    inner = docs[1:-1] if n > 1 else []
    step = max(4, (len(out) // (len(inner) + 1)) // 4 * 4)
    for i in range(len(inner)):                       # front to back: an insertion moves nothing in front of it
        p = min((i + 1) * step + 4 * i, len(out) // 4 * 4)    # rows p, p + 1, p + 2 = "", the document, "a"
        out[p:p] = ["", inner[i], "a"] if i < 2 else [inner[i]]
    if n > 1:
        while (len(out) + 2) % 4 < 2:
            out.pop()
        out += ["", "c", docs[-1]]
    return out


# ---- CSR rows ----------------------------------------------------------------------------------------------------------------------

def doc_rows(rng, n_col, nnz):
    """one L2-normalised CSR row (columns int32 ascending, values float64) of nnz distinct columns, values in [0.05, 1.05) before
    normalising: random_csr's rows at a chosen length"""
    cols = np.sort(rng.choice(n_col, size=int(nnz), replace=False)).astype(np.int32)
    vals = rng.random(len(cols)) + 0.05
    return cols, vals / np.sqrt((vals * vals).sum())


def copy_row(rng, row, share, n_col):
    """a near-copy of a CSR row: that share of its columns replaced by columns it did not have, every value moved by up to
    +-5 %, renormalised"""
    cols, vals = row
    k = max(1, int(round(share * len(cols))))
    drop = rng.choice(len(cols), size=k, replace=False)
    free = np.setdiff1d(np.arange(n_col, dtype=np.int64), cols, assume_unique=False)
    new = cols.copy()
    new[drop] = rng.choice(free, size=k, replace=False)
    v = vals * (1.0 + 0.05 * (2.0 * rng.random(len(vals)) - 1.0))
    order = np.argsort(new, kind="stable")
    new, v = new[order].astype(np.int32), v[order]
    return new, v / np.sqrt((v * v).sum())


def rows_to_csr(rows):
    ptr = np.zeros(len(rows) + 1, np.int64)
    for r, (c, _) in enumerate(rows):
        ptr[r + 1] = ptr[r] + len(c)
    return (ptr, np.concatenate([np.asarray(c, np.int32) for c, _ in rows]).astype(np.int32),
            np.concatenate([np.asarray(v, np.float64) for _, v in rows]).astype(np.float64))


def csr_to_rows(a3):
    ip, ix, dv = [np.asarray(x) for x in a3]
    return [(ix[ip[r]:ip[r + 1]].copy(), dv[ip[r]:ip[r + 1]].copy()) for r in range(len(ip) - 1)]


def take_rows(a3, rows):
    r = csr_to_rows(a3)
    return rows_to_csr([r[int(i)] for i in rows])


def shared_counter(a3, b3, n_col):
    """shared(i, j) -> number of columns that row i of a3 and row j of b3 have in common"""
    ap, ai = np.asarray(a3[0]), np.asarray(a3[1])
    bp, bi = np.asarray(b3[0]), np.asarray(b3[1])
    masks = {}

    def shared(i, j):
        i, j = int(i), int(j)
        if i not in masks:
            m = np.zeros(n_col, bool)
            m[ai[ap[i]:ap[i + 1]]] = True
            masks[i] = m
        return int(masks[i][bi[bp[j]:bp[j + 1]]].sum())
    return shared


def shared_row(a3, b3, n_col, i):
    """shared(i, j) for every j at once"""
    m = np.zeros(n_col, np.int64)
    m[np.asarray(a3[1])[a3[0][i]:a3[0][i + 1]]] = 1
    c = np.concatenate([[0], np.cumsum(m[np.asarray(b3[1])])])
    return c[np.asarray(b3[0])[1:]] - c[np.asarray(b3[0])[:-1]]


# ---- the K3 list of part B ---------------------------------------------------------------------------------------------------------

K3_N, K3_COLS, K3_BLOCK = 4300, 24000, 2048
K3_SEED = 37               # chosen so that the ORACLE shows no near-tie among the documents' best scores (test_documents_cpu.py)
K3_EMPTY = (0, 2048, K3_N - 1)
# size -> rows of (original, 1 % copy, 5 % copy): the original in to-block 0, the copies in blocks 1 and 2.
#   65:   row 40 opens a lock-step chunk of 4 and of 5 rows (40 = 0 mod 20); all three in one LDS bank class (row mod 32)
#   128:  row 59 closes a chunk of 4 and of 5 (59 = 19 mod 20); three different bank classes
#   129:  row 301 lies between two 20-entry rows (300, 302); the 1 % copy in its bank class, the 5 % copy in another
#   1000: three bank classes
#   4097: one bank class
#   8000: the last row of block 0, the first row after the empty row 2048, the row before the empty last row
K3_DOCS = {65: (40, 2048 + 40, 4096 + 40), 128: (59, 2048 + 100, 4096 + 77), 129: (301, 2048 + 301 + 32, 4096 + 150),
           1000: (777, 2048 + 1500, 4096 + 3), 4097: (1234, 2048 + 1234, 4096 + 82), 8000: (2047, 2049, K3_N - 2)}
K3_PAIR = {16000: (1600, 3000)}             # original and 1 % copy only; beyond 1e-5, held to its bound alone
K3_TWENTY = (300, 302)


def k3_list(seed=K3_SEED):
    """-> (a3, doc_rows): the self-match list of part B (float64 CSR triple) and the sorted rows that hold documents"""
    rng = np.random.default_rng(seed)
    rows = csr_to_rows(random_csr(rng, K3_N, K3_COLS, 0.0005, empty_rows=K3_EMPTY))
    for r in K3_TWENTY:
        rows[r] = doc_rows(rng, K3_COLS, 20)
    for size, places in list(K3_DOCS.items()) + list(K3_PAIR.items()):
        orig = doc_rows(rng, K3_COLS, size)
        rows[places[0]] = orig
        for place, share in zip(places[1:], (0.01, 0.05)):
            rows[place] = copy_row(rng, orig, share, K3_COLS)
    held = sorted(r for places in list(K3_DOCS.values()) + list(K3_PAIR.values()) for r in places)
    return rows_to_csr(rows), np.array(held, np.int64)


# ---- the acceptance rule -----------------------------------------------------------------------------------------------------------

def k3_bound(c, norm_bound=1.0):
    """|K3 score - exact| for a pair of rows with c columns in common: one truncation of at most 2^-30 * norm_bound per shared
    column, plus the float32 storage of the two values, the float32 product and the final int -> float conversion (relative 2^-24
    each, four in all, on a score <= 1: 2.4e-7, rounded up).  Derived, not measured."""
    return c * 2.0 ** -30 * norm_bound + 3e-7


def assert_topn_within_bound(idx, val, exp_idx, exp_val, dense_row, shared, rows=None, exclude_diag=False, lower_bound=0.0,
                             norm_bound=1.0, max_swap_rows=None):
    """The acceptance rule for document rows.  idx / val: K3's result (int32, fp32) for the from-rows `rows` (default 0 .. n - 1),
    exp_idx / exp_val the float64 oracle's (canonical order); dense_row(i) -> the oracle's scores of from-row i against every
    to-row; shared(i, j) -> the number of columns from-row i and to-row j have in common.

    * every score is within k3_bound(shared(i, j)) of the oracle's score of that very pair;
    * an index may differ from the oracle's at a rank only if the oracle's scores of the two candidates differ by less than
      NEAR_TIE plus the two candidates' bounds (a candidate missing on one side: its oracle score is that close to lower_bound);
    * no column twice in a row, no diagonal where it is excluded;
    * rows with such a swap: at most max(1, 1 % of the rows checked).
    Returns [(row, column, shared, signed error)] of every cell, for reports."""
    idx, val = np.asarray(idx), np.asarray(val, np.float64)
    exp_idx, exp_val = np.asarray(exp_idx), np.asarray(exp_val, np.float64)
    assert idx.shape == exp_idx.shape == val.shape, (idx.shape, exp_idx.shape)
    rows = np.arange(len(idx)) if rows is None else np.asarray(rows)
    bound = lambda i, j: k3_bound(shared(i, j), norm_bound)
    cells, swapped = [], 0
    for p, i in enumerate(rows.tolist()):
        dense = dense_row(i)
        got = idx[p][idx[p] >= 0]
        assert len(set(got.tolist())) == len(got), f"row {i}: a column twice in {idx[p]}"
        assert (idx[p][len(got):] == -1).all() and (val[p][len(got):] == 0).all(), f"row {i}: a hole inside {idx[p]}"
        if exclude_diag:
            assert i not in got.tolist(), f"row {i}: the diagonal is in {idx[p]}"
        swap = False
        for r in range(idx.shape[1]):
            j, e = int(idx[p, r]), int(exp_idx[p, r])
            if j >= 0:
                err = val[p, r] - dense[j]
                assert abs(err) <= bound(i, j), f"row {i} rank {r} column {j}: score {val[p, r]!r}, oracle {dense[j]!r}, " \
                                                f"error {err:.3e} beyond {bound(i, j):.3e} ({shared(i, j)} shared columns)"
                cells.append((i, j, shared(i, j), float(err)))
            if j == e:
                continue
            swap = True
            s_j, b_j = (dense[j], bound(i, j)) if j >= 0 else (lower_bound, 0.0)
            s_e, b_e = (exp_val[p, r], bound(i, e)) if e >= 0 else (lower_bound, 0.0)
            assert abs(s_j - s_e) < NEAR_TIE + b_j + b_e, f"row {i} rank {r}: column {j} (oracle score {s_j!r}) where the oracle " \
                                                          f"has column {e} (score {s_e!r}): no near-tie"
        swapped += swap
    cap = max(1, len(rows) // 100) if max_swap_rows is None else max_swap_rows
    assert swapped <= cap, f"{swapped} of {len(rows)} rows differ from the oracle's indices"
    return cells


def oracle_near_ties(dense, shared_all, n_scores, skip=None, lower_bound=0.0, norm_bound=1.0):
    """On the oracle alone: the pairs among the n_scores best scores of one from-row (`dense`: its scores against every to-row,
    `shared_all`: its shared-column counts, `skip`: the diagonal) that the rule above would let swap, plus the scores that close
    to lower_bound -> list of (column, column or -1)"""
    d = np.array(dense, np.float64)
    if skip is not None:
        d[skip] = -1.0
    order = np.lexsort((np.arange(len(d)), -d))[:n_scores]
    order = order[d[order] > 0]
    b = k3_bound(np.asarray(shared_all)[order], norm_bound)
    out = []
    for x in range(len(order)):
        if lower_bound > 0 and abs(d[order[x]] - lower_bound) < NEAR_TIE + b[x]:
            out.append((int(order[x]), -1))
        for y in range(x + 1, len(order)):
            if abs(d[order[x]] - d[order[y]]) < NEAR_TIE + b[x] + b[y]:
                out.append((int(order[x]), int(order[y])))
    return out


# ---- K3's arithmetic restated (numpy, CPU) -----------------------------------------------------------------------------------------

def k3_scale_exponent(norm_a, norm_b):
    """k of k3_fixed_point (k3_core.h): S = 2^k, the largest power of two that keeps norm_a * norm_b * 1.0001 * S below 2^31"""
    bound = float(norm_a) * float(norm_b) * 1.0001 + 1e-30
    k = 30
    while k > -60 and np.ldexp(bound, k) >= 2147483000.0:
        k -= 1
    while k < 60 and np.ldexp(bound, k + 1) < 1073741824.0:
        k += 1
    return k


def k3_simulated_score(row_a, row_b, k=30):
    """what K3 computes for one pair of rows: values stored as float32, fp32(fp32(a * S) * b) truncated to an integer, integer
    sum, float32(sum) * 2^-k -> (score as float64, number of shared columns)"""
    ca, va = row_a
    cb, vb = row_b
    _, ia, ib = np.intersect1d(ca, cb, assume_unique=True, return_indices=True)
    a = np.asarray(va, np.float64).astype(np.float32)[ia]
    b = np.asarray(vb, np.float64).astype(np.float32)[ib]
    a_s = (a * np.float32(2.0 ** k)).astype(np.float32)
    prod = (a_s * b).astype(np.float32)
    total = int(np.trunc(prod.astype(np.float64)).astype(np.int64).sum())
    return float(np.float32(np.float32(total) * np.float32(2.0 ** -k))), len(ia)


def exact_score(row_a, row_b):
    ca, va = row_a
    cb, vb = row_b
    _, ia, ib = np.intersect1d(ca, cb, assume_unique=True, return_indices=True)
    return float(np.dot(np.asarray(va, np.float64)[ia], np.asarray(vb, np.float64)[ib]))


# ---- the string lists of parts A and C ---------------------------------------------------------------------------------------------

SEAM_COUNTS = (4095, 4096, 4097, 8192, 8193)      # n-grams: either side of k_rows_long's LDS sort (4 096) and of the next power of two


def _names(n, seed):
    from polyfuzz_amd import synth
    return synth.company_names(n, seed=seed)


def seam_documents(rng):
    """(3, 3)-grams of letters: count = length - 2.  Per count: 26 letters (most n-grams distinct), two letters (eight distinct at
    most), singleton first and last key"""
    out = []
    for n in SEAM_COUNTS:
        out += [doc(rng, n + 2), doc(rng, n + 2, "ab"), doc_with_singleton_ends(rng, n + 2)]
    return out


def seam_list(seed=101):
    rng = np.random.default_rng(seed)
    return splice(_names(300, seed), seam_documents(rng))


def range_list(lengths, seed):
    """names with one 26-letter document per length (several n values: count = R * length - const)"""
    rng = np.random.default_rng(seed)
    return splice(_names(200, seed), [doc(rng, n) for n in lengths])


SLAB_TILES, SLAB_DOUBLE = 70, (3, 66)             # more tiles with a giant than the 64 workgroups of the giant grid; two with two


def slab_list(seed=103):
    """1 200 strings; one 4 100-character document in each of the first 70 tiles of 16 strings (at changing places inside the
    tile), a second giant of 5 000 characters in two of them"""
    rng = np.random.default_rng(seed)
    out = _names(1200, seed)
    for t in range(SLAB_TILES):
        out[16 * t + (5 * t) % 16] = doc(rng, 4100)
        if t in SLAB_DOUBLE:
            out[16 * t + (5 * t + 7) % 16] = doc(rng, 5000)
    return out


UNSEEN_FIT_ALPHABET, UNSEEN_ALPHABET = "abcdefghijklmnop", "qrstuvwxyz"


def unseen_lists(seed=104):
    """-> (fit list, transform list): names and documents over 16 letters; the transform list ends with a 6 000-character document
    of letters the fit never saw (an empty row) and one mixed about 50 / 50 in runs of 1 .. 8 characters (its unknown n-grams sort
    behind the known ones)"""
    rng = np.random.default_rng(seed)
    fit = splice(short_names(rng, 150, UNSEEN_FIT_ALPHABET), [doc(rng, n, UNSEEN_FIT_ALPHABET) for n in (4200, 5000, 9000)])
    mixed = ""
    while len(mixed) < 6000:
        mixed += doc(rng, int(rng.integers(1, 9)), UNSEEN_FIT_ALPHABET) + doc(rng, int(rng.integers(1, 9)), UNSEEN_ALPHABET)
    new = splice(short_names(rng, 150, UNSEEN_FIT_ALPHABET + "qr"),
                 [doc(rng, 4500, UNSEEN_FIT_ALPHABET), doc(rng, 6000, UNSEEN_ALPHABET), mixed[:6000]])
    return fit, new


def two_list_cases(seed=105):
    """(to-list, from-list): giants in the to-list only, in the from-list only, in both"""
    rng = np.random.default_rng(seed)
    to, frm = _names(260, seed), _names(170, seed + 1)
    g = [doc(rng, n) for n in (4098, 4099, 6000, 8200)]
    return [(splice(to, g[:2]), list(frm)), (list(to), splice(frm, g[2:])), (splice(to, g[:2]), splice(frm, g[1:]))]


E2E_LENGTHS = (4099, 4500, 5000, 5600, 6300, 7000, 8000, 9000)
E2E_SEED = 106


def end_to_end_list(seed=E2E_SEED):
    """-> (list, rows of the documents, rows of their 0.5 % copies, rows of their 2 % copies): 300 names, eight documents of
    4 099 .. 9 000 characters and two edited copies of each, spread over the list"""
    rng = np.random.default_rng(seed)
    out = _names(300, seed)
    docs = [doc(rng, n) for n in E2E_LENGTHS]
    near = [edited(rng, d, 0.005) for d in docs]
    far = [edited(rng, d, 0.02) for d in docs]
    rows = ([], [], [])
    for k, group in enumerate((docs, near, far)):
        for i, d in enumerate(group):
            p = (37 * i + 101 * k + 11) % len(out)
            out.insert(p, d)
    for k, group in enumerate((docs, near, far)):
        for d in group:
            rows[k].append(out.index(d))
    return out, rows[0], rows[1], rows[2]
