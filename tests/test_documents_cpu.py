"""What the document tests of the GPU suite (test_documents_gpu.py) rely on, checked on the CPU: K3's fixed-point arithmetic restated
in numpy stays inside `k3_bound` on rows of thousands of entries -- and is far outside the "13 * 2^-30" that holds for company
names --, the generated documents sit on the seams they are meant for, and the float64 oracle alone shows no near-tie among the
document rows' best scores (so a GPU result that differs there is wrong, not unlucky)."""
import numpy as np
import pytest

from tests import document_cases as dc
from tests.helpers import SCORE_TOL


@pytest.fixture(scope="module")
def k3_case():
    a3, held = dc.k3_list()
    return a3, held, dc.csr_to_rows(a3)


def _pairs():
    for size, places in list(dc.K3_DOCS.items()) + list(dc.K3_PAIR.items()):
        for x in range(len(places)):
            for y in range(x + 1, len(places)):
                yield size, places[x], places[y]


def test_k3_list_is_the_one_described(k3_case):
    a3, held, rows = k3_case
    n = len(a3[0]) - 1
    assert n == dc.K3_N == 4300 and (n + dc.K3_BLOCK - 1) // dc.K3_BLOCK == 3
    assert int(a3[1].max()) < dc.K3_COLS == 24000
    for r in dc.K3_EMPTY:
        assert len(rows[r][0]) == 0
    for r in dc.K3_TWENTY:
        assert len(rows[r][0]) == 20
    # either side of the 64 entries one trip of K3's from-row loop takes, of 128 and of 4 096
    assert sorted(dc.K3_DOCS) == [65, 128, 129, 1000, 4097, 8000] and list(dc.K3_PAIR) == [16000]
    for size, places in list(dc.K3_DOCS.items()) + list(dc.K3_PAIR.items()):
        for k, r in enumerate(places):
            cols, vals = rows[r]
            assert len(cols) == size and (np.diff(cols) > 0).all() and abs(float((vals * vals).sum()) - 1.0) < 1e-12
            assert r // dc.K3_BLOCK == k or size == 16000          # original in to-block 0, the copies in blocks 1 and 2
    assert [r // dc.K3_BLOCK for r in dc.K3_PAIR[16000]] == [0, 1]
    cls = lambda size: {r % 32 for r in dc.K3_DOCS[size]}
    assert len(cls(65)) == 1 and len(cls(4097)) == 1 and len(cls(128)) == 3 and len(cls(1000)) == 3 and len(cls(129)) == 2
    assert dc.K3_DOCS[65][0] % 20 == 0 and dc.K3_DOCS[128][0] % 20 == 19          # first / last row of a chunk of 4 and of 5 rows
    assert dc.K3_DOCS[129][0] - 1 in dc.K3_TWENTY and dc.K3_DOCS[129][0] + 1 in dc.K3_TWENTY
    # the rest are short rows (density 0.0005: about 12 entries)
    others = np.setdiff1d(np.arange(n), np.concatenate([held, dc.K3_TWENTY]))
    assert np.diff(a3[0])[others].max() < 64


def test_k3_arithmetic_restated_stays_within_the_bound(k3_case):
    """fp32(fp32(a * 2^30) * b) truncated, integer sum, float32(sum) * 2^-30 against the float64 dot product: inside k3_bound for
    every document pair -- and, for the longest, far beyond the 13 * 2^-30 that was the statement for company names"""
    a3, held, rows = k3_case
    worst = {}
    for size, i, j in _pairs():
        got, c = dc.k3_simulated_score(rows[i], rows[j])
        err = got - dc.exact_score(rows[i], rows[j])
        assert c >= 0.9 * size * 0.95
        assert abs(err) <= dc.k3_bound(c), (size, i, j, c, err)
        assert err <= 3e-7                                   # truncation only ever lowers a score
        worst[size] = max(worst.get(size, 0.0), abs(err))
        print(f"simulated: {size:6d} entries, rows {i:4d} x {j:4d}: {c:6d} shared, error {err:+.3e} = {abs(err) / dc.k3_bound(c):.2f} of the bound")
    assert worst[16000] > 13 * 2.0 ** -30 and worst[8000] > 13 * 2.0 ** -30
    assert worst[16000] > worst[1000] > worst[65]                 # it grows with the shared columns


def test_k3_arithmetic_restated_on_unnormalised_rows(k3_case):
    """values times 7.5: the scale follows the norm bound (k3_fixed_point: 2^25 for 56.25 * 1.0001), the bound with it"""
    a3, held, rows = k3_case
    k = dc.k3_scale_exponent(7.5, 7.5)
    assert k == 25
    for i, j in ((2047, 2049), (2047, dc.K3_N - 2)):
        a, b = (rows[i][0], rows[i][1] * 7.5), (rows[j][0], rows[j][1] * 7.5)
        got, c = dc.k3_simulated_score(a, b, k)
        err = got - dc.exact_score(a, b)
        assert abs(err) <= dc.k3_bound(c, 7.5 * 7.5 * 1.0001) and abs(err) > dc.k3_bound(c)


def test_bounds_of_the_rows_held_to_1e5(k3_case):
    a3, held, rows = k3_case
    for size, places in dc.K3_DOCS.items():
        assert dc.k3_bound(size) < SCORE_TOL                # at most `size` shared columns
    for size, (i, j) in dc.K3_PAIR.items():
        c = len(np.intersect1d(rows[i][0], rows[j][0]))
        assert dc.k3_bound(c) >= SCORE_TOL                  # this pair is promised its bound only
    assert dc.k3_bound(10_000) < SCORE_TOL < dc.k3_bound(10_500)         # "1e-5 holds up to about 10 000 shared n-grams"


def test_oracle_has_no_near_tie_among_the_document_rows(k3_case, oracle_mod):
    """the self-match's first 32 + 1 scores of every document row (diagonal left out) and the two-list match's first 5 + 1 with the
    lower bound 0.5: no two closer than NEAR_TIE + their bounds, none that close to the lower bound"""
    a3, held, rows = k3_case
    for i in held.tolist():
        dense = oracle_mod.cossim_dense(a3, a3, dc.K3_COLS, rows=(i, i + 1))[0]
        sh = dc.shared_row(a3, a3, dc.K3_COLS, i)
        assert dc.oracle_near_ties(dense, sh, 33, skip=i) == [], i
        assert dc.oracle_near_ties(dense, sh, 6, lower_bound=0.5) == [], i
        # the copies are the best matches, well apart
        group = [p for p in list(dc.K3_DOCS.values()) + list(dc.K3_PAIR.values()) if i in p][0]
        best = np.argsort(-np.where(np.arange(len(dense)) == i, -1.0, dense))[:len(group) - 1]
        assert set(best.tolist()) == set(group) - {i}


def test_seam_documents_sit_on_the_seams(oracle_mod):
    from oracle.tfidf_oracle import create_ngrams
    rng = np.random.default_rng(1)
    docs = dc.seam_documents(rng)
    assert len(docs) == 15
    for clean in (True, False):
        counts = [len(create_ngrams(d, (3, 3), clean)) for d in docs]
        assert counts == [n for n in (4095, 4096, 4097, 8192, 8193) for _ in range(3)]
    for k, d in enumerate(docs):
        grams = create_ngrams(d, (3, 3), True)
        distinct = len(set(grams))
        if k % 3 == 0:
            assert distinct > 0.85 * min(len(grams), 17576 * (1 - np.exp(-len(grams) / 17576)))        # most are distinct
        elif k % 3 == 1:
            assert distinct <= 8
        else:
            assert grams.count(min(grams)) == 1 and grams.count(max(grams)) == 1 and min(grams) == "aaa" and max(grams) == "zzz"
    # several n values: three slots per character, five with (3, 7)
    assert [len(create_ngrams(dc.doc(rng, n), (2, 4), True)) for n in (1367, 1368, 5000)] == [4095, 4098, 14994]
    assert [len(create_ngrams(dc.doc(rng, n), (3, 7), True)) for n in (823, 824, 3000)] == [4095, 4100, 14980]


def test_lists_of_part_a():
    from oracle.tfidf_oracle import create_ngrams
    cnt = lambda s: len(create_ngrams(s, (3, 3), True))
    lst = dc.seam_list()
    big = [i for i, s in enumerate(lst) if cnt(s) > 128]
    assert len(big) == 15 and big[0] == 0 and big[-1] == len(lst) - 1
    # "", a document and a one-character string within one group of four rows, at the front, inside and at the end
    for i in (big[0], big[1], big[2], big[-1]):
        group = lst[i // 4 * 4:i // 4 * 4 + 4]
        assert "" in group and any(len(s) == 1 for s in group), i
    slab = dc.slab_list()
    assert len(slab) == 1200
    giants = [i for i, s in enumerate(slab) if cnt(s) > 4096]
    per_tile = np.bincount(np.array(giants) // 16, minlength=75)
    assert (per_tile[:70] >= 1).all() and (per_tile[70:] == 0).all() and sorted(np.nonzero(per_tile == 2)[0].tolist()) == [3, 66]
    assert (per_tile > 0).sum() > 64
    fit, new = dc.unseen_lists()
    seen = set("".join(fit))
    docs =[s for s in new if len(s) >= 4000]
    assert len(docs) == 3
    assert sum(1 for s in docs if not (set(s) & seen)) == 1                    # one of symbols the fit never saw
    mixed = [s for s in docs if set(s) & seen and set(s) - seen]
    assert len(mixed) == 1 and 0.4 < sum(c in seen for c in mixed[0]) / len(mixed[0]) < 0.6 and cnt(mixed[0]) > 4096
    vocab = {g for s in fit for g in create_ngrams(s, (3, 3), False)}
    known = sum(g in vocab for g in create_ngrams(mixed[0], (3, 3), False))
    assert 100 < known < cnt(mixed[0]) - 100                                   # valid and invalid keys, many of each
    for to, frm in dc.two_list_cases():
        assert max(map(cnt, to)) > 4096 or max(map(cnt, frm)) > 4096
    t = [(max(map(cnt, to)) > 4096, max(map(cnt, frm)) > 4096) for to, frm in dc.two_list_cases()]
    assert t == [(True, False), (False, True), (True, True)]


def test_end_to_end_list_has_no_oracle_near_tie(oracle_mod):
    lst, docs, near, far = dc.end_to_end_list()
    assert len(lst) == 324 and [len(lst[i]) for i in docs] == [4099, 4500, 5000, 5600, 6300, 7000, 8000, 9000]
    assert [len(lst[i]) for i in near] == [len(lst[i]) for i in far] == [len(lst[i]) for i in docs]
    o = oracle_mod.TfidfOracle().fit(lst)
    a3 = o.transform(lst)
    n_col = len(o.vocabulary)
    for k, i in enumerate(docs + near + far):
        assert a3[0][i + 1] - a3[0][i] > 2000
        dense = oracle_mod.cossim_dense(a3, a3, n_col, rows=(i, i + 1))[0]
        sh = dc.shared_row(a3, a3, n_col, i)
        assert dc.oracle_near_ties(dense, sh, 4, skip=i) == [], i
        assert dc.k3_bound(int(sh.max())) < SCORE_TOL
        d = dense.copy()
        d[i] = -1
        if k < 8:
            assert int(d.argmax()) == near[k]                # a document's best match is its 0.5 % copy
