"""What the second-row and table-border tests of the GPU suite (test_second_row_gpu.py, test_indel_table_borders_gpu.py) rely on,
checked on the CPU: the pair oracle is the textbook table, the two lower bounds never leave out a pair that reaches a threshold,
both thresholds cut through the families, the filtered oracle is affordable, and every generated list has the sizes, lengths and
alphabets that take a workgroup of each kernel to a second row or a word class of K4 across its table-size border."""
import numpy as np
import pytest

from tests import indel_oracle, lev_oracle
from tests import second_row_cases as sc

N_CU = 256               # the lists as an MI355X gets them (the GPU tests read the count from the context)
METRICS = ("levenshtein", "osa", "indel")


def _distances(metric, fl, tl):
    if metric == "indel":
        return indel_oracle.distance(indel_oracle.lcs_matrix(fl, tl), lev_oracle.lengths(fl)[:, None], lev_oracle.lengths(tl)[None, :])
    return lev_oracle.matrix(fl, tl, metric)


def test_pair_oracle_is_the_textbook_table():
    rng = np.random.default_rng(711)
    a = ["", "", "a", "ab", "ba", "CA", "abcdef", "ab" * 20] + [sc.text(rng, n, "abc") for n in rng.integers(0, 30, 40)]
    b = ["", "abc", "", "ba", "ab", "ABC", "badcfe", "ba" * 20] + [sc.edited(rng, s, rng.integers(0, 6), "abc") for s in a[8:]]
    for name in lev_oracle.SCORERS:
        np.testing.assert_array_equal(sc.pair_lev(a, b, name), [lev_oracle.distance(x, y, name) for x, y in zip(a, b)], err_msg=name)
    np.testing.assert_array_equal(sc.pair_lcs(a, b), [indel_oracle.lcs(x, y) for x, y in zip(a, b)])
    assert sc.pair_lev(["ab"], ["ba"], "osa")[0] == 1 and sc.pair_lev(["ab"], ["ba"], "levenshtein")[0] == 2
    assert (sc.pair_lev(a, b, "osa") < sc.pair_lev(a, b, "levenshtein")).sum() >= 5          # (the two scorers did part)


@pytest.fixture(scope="module")
def families():
    return sc.family_list(N_CU)


def test_family_list_is_the_one_described(families):
    sl, fam = families
    assert len(sl) == 8 * N_CU + 256 == 2304 and np.array_equal(np.bincount(fam), np.full(len(sl) // 4, 4))
    lens = lev_oracle.lengths(sl)
    assert lens.min() >= 65 and lens.max() <= 93 and len(set(lens.tolist())) > 15           # beyond 64: the general kernel's rows
    assert set("".join(sl)) == set(sc.LETTERS20)
    assert (np.diff(fam) != 0).mean() > 0.99                                                 # (the families are spread over the list)
    assert len(sc.family_list(4)[0]) == 8 * 4 + 256


def test_no_filtered_pair_reaches_a_threshold(families):
    """300 strings -- 75 whole families -- scored in full by the matrix oracles: both bounds are at most the distance of every pair,
    no pair the filter leaves out reaches either threshold, and the filtered oracle is the thresholded matrix"""
    sl, fam = families
    sample = [s for s, f in zip(sl, fam) if f < 75]
    assert len(sample) == 300
    bounds = sc.distance_bounds(sample, sample)
    la = lev_oracle.lengths(sample)
    for metric in METRICS:
        d = _distances(metric, sample, sample)
        len_diff, bag = sc.lower_bounds(bounds, metric)
        assert (len_diff <= d).all() and (bag <= d).all(), metric
        assert (bag > len_diff).mean() > 0.9                                                  # (the bag distance is the one that bites)
        sim = sc.best_possible(metric, d, la[:, None], la[None, :])
        full = indel_oracle.similarity((la[:, None] + la[None, :] - d) // 2, la[:, None], la[None, :]) if metric == "indel" else \
            lev_oracle.sim_matrix(sample, sample, d)
        np.testing.assert_array_equal(sim, full, err_msg=metric)                              # (best_possible at d IS the oracle's score)
        for thr in sc.JOIN_THRESHOLDS:
            for self_join in (False, True):
                keep = sc.survivors(sample, sample, thr, metric, self_join, bounds)
                hit = (sim >= thr) & (np.triu(np.ones(d.shape, bool), 1) if self_join else True)
                assert not (hit & ~keep).any(), (metric, thr)
                assert keep.sum() > hit.sum()                                                 # (and some survivors are misses)
                i, j = np.nonzero(hit)
                row_ptr, idx, dist, s = sc.join_oracle(sample, sample, thr, metric, self_join, bounds=bounds)
                np.testing.assert_array_equal(np.repeat(np.arange(300), np.diff(row_ptr)), i)
                np.testing.assert_array_equal(idx, j)
                np.testing.assert_array_equal(dist, d[i, j])
                np.testing.assert_array_equal(s, sim[i, j])


def test_both_thresholds_cut_through_the_families_and_the_oracle_is_affordable(families):
    sl, fam = families
    n = len(sl)
    pairs = n * (n - 1) // 2
    in_family = 6 * (n // 4)
    bounds = sc.distance_bounds(sl, sl)
    for metric in METRICS:
        cache = {}
        for thr in sc.JOIN_THRESHOLDS:
            keep = sc.survivors(sl, sl, thr, metric, True, bounds)
            row_ptr, idx, dist, sim = sc.join_oracle(sl, sl, thr, metric, True, cache, bounds)
            rows = np.repeat(np.arange(n), np.diff(row_ptr))
            hits = int((fam[rows] == fam[idx]).sum())
            print(f"families {metric} t={thr}: {int(keep.sum())} of {pairs} pairs survive the bounds ({keep.sum() / pairs:.4%}), {len(idx)} hits, "
                  f"{hits} of the {in_family} pairs inside families")
            assert keep.sum() < 0.02 * pairs, (metric, thr)
            assert 0.3 * in_family < hits < 0.99 * in_family, (metric, thr, hits)            # hits and misses inside families
            assert (sim >= thr).all() and (rows < idx).all()
    assert len(sc.JOIN_THRESHOLDS) == 2 and sc.JOIN_THRESHOLDS[0] == 0.9 > sc.JOIN_THRESHOLDS[1]


@pytest.mark.parametrize("wide", (False, True), ids=("symbols8", "symbols16"))
def test_k4_lists(wide):
    fl, tl = sc.k4_lists(N_CU, wide)
    n = len(fl)
    assert n == 2 * N_CU + 96 and len(tl) == 256
    lf, lt = lev_oracle.lengths(fl), lev_oracle.lengths(tl)
    assert lf.min() == 0 and lf.max() <= 130 and (lf.max() + 63) // 64 == 3                  # W = 3 words
    assert set(sc.K4_EDGE_LENGTHS) <= set(lf[:n - 96].tolist()) and set(sc.K4_EDGE_LENGTHS) <= set(lf[n - 96:].tolist())
    assert lt.min() == 0 and lt.max() == 300 and "" in tl
    assert all(tl.count(s) >= 2 for s in tl) and tl[:128] == tl[128:][::-1]                  # every to-string twice: ties
    distinct = len(set("".join(tl)))
    assert distinct == (420 if wide else 20) and (distinct > 255) == wide
    assert set("".join(fl)) <= set("".join(tl))
    assert len(sc.k4_lists(8, wide)[0]) == 2 * 8 + 96


def test_k4_from_strings_are_near_a_to_string(oracle_mod):
    fl, tl = sc.k4_lists(N_CU)
    idx, score = oracle_mod.indel_argmax(fl, tl)
    la, lb = lev_oracle.lengths(fl), lev_oracle.lengths(tl)[idx]
    lcs = np.rint(score * (la + lb) / 200.0)
    assert np.median(lcs[la > 0] / la[la > 0]) > 0.9                                          # most of a from-string is in its best match
    assert (idx < 128).all()                                                                  # (the later twin never wins)


def test_k7_lists():
    fl, tl = sc.k7_lists(N_CU)
    assert len(fl) == 2 * N_CU + 64 and len(tl) == 48
    for part in (fl[:2 * N_CU], fl[2 * N_CU:]):                                               # among the first rows and the second ones
        assert "" in part and any(len(s.split()) == 1 for s in part) and any(len(s.split()) >= 4 for s in part)
    assert "" in tl and len(set(fl)) < len(fl)                                                 # (repeats: a self-match has first occurrences)


def test_k10_lists_and_the_dealing_rule():
    fl, tl, tab = sc.k10_lists()
    lens = lev_oracle.lengths(fl)
    assert len(fl) == 200 and tab.shape == (200, 8) and (lens[0::2] > 64).all() and (lens[1::2] <= 64).all() and lens.min() == 0
    assert all(len(set(r.tolist())) == 8 for r in tab) and tab.min() >= 0 and tab.max() < len(tl)
    general = set(np.nonzero(lens > 64)[0].tolist())
    for n_cu in (4, 64, N_CU, 304):
        grid = sc.k10_general_grid(len(fl), len(general), n_cu, jaro=False)
        assert grid == 100
        dealt = sc.k10_rows_of_workgroups(len(fl), grid)
        assert sorted(r for rows in dealt for r in rows) == list(range(200))
        assert sum(1 for rows in dealt if len(general & set(rows)) == 2) == 50
        assert sc.k10_general_grid(len(fl), len(general), n_cu, jaro=True) == min(200, 32 * n_cu)


def test_k4_dispatch_rule_restated():
    lengths = [n for n in sc.BORDER_FROM_LENGTHS for _ in range(2)]
    assert [sc.k4_class(n) for n in sc.BORDER_FROM_LENGTHS] == [0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6]
    # below a border the class keeps its rows, at it they go: two strings of each of two lengths per class, ten for the 32-bit class
    want = {479: 2, 480: 6, 959: 6, 960: 10, 1919: 10, 1920: 14, 3839: 14, 3840: 18, 7679: 18, 7680: 22, 15359: 22, 15360: 32}
    assert {s: sc.k4_general_rows(lengths, s) for s in sc.K4_BORDERS} == want
    assert [sc.k4_quad_launches(lengths, s) for s in sc.K4_BORDERS] == [2] * 7 + [0] * 5      # 16 bytes per symbol: up to 3 839
    assert sc.k4_quad_launches([40, 70], 100) == 0 and sc.k4_quad_launches([5], 100) == 1
    for c in range(6):
        fits = sc.K4_LDS_BYTES // sc.K4_CLASS_WORD_BYTES[c] - 1                               # symbols whose table (+ entry 0) just fits
        assert fits in sc.K4_BORDERS and fits + 1 in sc.K4_BORDERS


@pytest.mark.parametrize("n_sym", sc.K4_BORDERS)
def test_border_lists(oracle_mod, n_sym):
    fl, tl, hot = sc.border_lists(n_sym)
    n_base = (n_sym + 63) // 64
    assert len(set("".join(tl))) == n_sym and len(hot) == 12 and set(hot) <= set("".join(tl[:n_base]))
    assert all(len(s) == 64 for s in tl[:n_base]) and len(tl) == n_base + sc.border_hot_count(n_sym)
    assert all(set(s) <= set(hot) for s in tl[n_base:]) and {1, 600} <= set(map(len, tl[n_base:]))
    assert sc.border_hot_count(n_sym) == 40 or n_sym > 1920
    assert [len(s) for s in fl] == [n for n in sc.BORDER_FROM_LENGTHS for _ in range(2)]
    assert set("".join(fl)) <= set("".join(tl))
    m = oracle_mod.indel_argmax(fl, tl, want_matrix=True)[2]
    assert (m != 0).mean() > 0.5, (m != 0).mean()
