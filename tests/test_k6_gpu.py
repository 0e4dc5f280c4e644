"""K6's two kernels on the GPU at the shapes where they can go wrong (tests/test_k6_core_cpu.py holds their per-element decisions to
the same oracles on the CPU).  k_linkage_top1: `==` against the sequential walk (linkage.greedy_assign on the kept rows: cluster,
the order by key, key == -1 where unmapped, the founding count, the rounds) from 1 to 8191 rows -- one to eight rows per thread
-- on random graphs, chains, stars, 2-cycles and rows that point at themselves, with scores at the float32 neighbours of the
rounding ties and To indices outside [0, n); three ranks per row; and the reference's same-list case end to end.  k_pr_hist
through _lib.pr_curve: counts `==` numpy's, sums against the exact sum within the bound the fixed point implies, from 1 to 4096
thresholds and 0 to 600 000 similarities."""
import math

import numpy as np
import pytest

from tests.test_k6_core_cpu import check_against_walk, graph_shapes, kept_oracle, pr_error_bound, scores_for

pytestmark = pytest.mark.gpu
THRESHOLDS = (0.0, 0.3, 0.75)


# ---- k_linkage_top1 ----------------------------------------------------------------------

def _linkage(ctx, g, val, thr):
    from polyfuzz_amd import _lib
    return _lib.linkage_top1(ctx, _lib.DeviceTopN.from_host(ctx, g, val), thr)


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 8191])
def test_linkage_equals_the_walk(ctx, n):
    """eight graph shapes x three thresholds per row count.  The structural shapes keep every row (their scores round above the
    threshold from either side of a tie), so that the chains stay whole: i -> i + 1 settles one row per activity round, the most a graph of n rows
    takes.  The random shapes -- and every shape up to 65 rows -- also draw scores at the threshold's own ties and
    around 0.001, which fall on both sides of the rule."""
    from polyfuzz_amd.linkage import greedy_assign
    rng = np.random.default_rng(1000 + n)
    for name, g in graph_shapes(n, rng):
        for thr in THRESHOLDS:
            val = scores_for(n, thr, name.startswith("random") or n <= 65, rng)
            kept = kept_oracle(g, val, n, thr)
            cluster, key, info = _linkage(ctx, g, val, thr)
            try:
                check_against_walk(g, kept, cluster, key, info, n, greedy_assign)
            except AssertionError as e:
                raise AssertionError(f"{name}, {n} rows, min_similarity {thr}: {e}") from None
            if name == "forward_chain" and thr == 0.0:
                assert n // 2 <= info["rounds"] <= n + 1
                print(f"K6 linkage, forward chain of {n} rows: {info['rounds']} fixpoint rounds")
            if name == "all_self" and n > 65:
                assert kept.all() and info["clusters"] == n and info["rounds"] == 1 and (cluster == np.arange(n)).all()


def test_smallest_self_pointing_case(ctx):
    """idx = [0, 1]: row 0 is the first kept row, row 1 points at itself -- two clusters of one string each, one round"""
    cluster, key, info = _linkage(ctx, np.array([0, 1]), np.array([0.9, 0.9], np.float32), 0.5)
    assert cluster.tolist() == [0, 1] and info == {"first_row": 0, "rounds": 1, "clusters": 2}
    assert np.argsort(key, kind="stable").tolist() == [0, 1]


@pytest.mark.parametrize("n", [1025, 2049])
def test_only_rank_0_is_read(ctx, n):
    """a result with three ranks per row (row stride 3): ranks 1 and 2 hold indices in and outside [0, n), the row itself among
    them, and scores above every threshold -- the answer is byte for byte that of the one-rank call"""
    rng = np.random.default_rng(n)
    for name, g in graph_shapes(n, rng)[:3]:                # random, forward chain, backward chain
        for thr in THRESHOLDS:
            val = scores_for(n, thr, name == "random", rng)
            junk = rng.integers(-9, n + 9, (n, 2))
            self_rows = rng.random(n) < 0.3
            junk[self_rows, 0] = np.arange(n)[self_rows]
            g3 = np.concatenate([g[:, None], junk], 1)
            v3 = np.concatenate([val[:, None], 1.0 + rng.random((n, 2)).astype(np.float32)], 1)
            one = _linkage(ctx, g, val, thr)
            three = _linkage(ctx, g3, v3, thr)
            assert one[0].tobytes() == three[0].tobytes() and one[1].tobytes() == three[1].tobytes() and one[2] == three[2], (name, thr)
            check_against_walk(g, kept_oracle(g, val, n, thr), three[0], three[1], three[2], n)


def _same_dicts(a, b):
    assert len(a) == len(b) == 3
    for x, y in zip(a, b):
        assert list(x.items()) == list(y.items())


@pytest.mark.parametrize("thr", [0.0, 0.5, 0.75, 0.9])
def test_same_list_as_two_lists_end_to_end(ctx, thr):
    """the reference's own same-list case (its tests/test_polyfuzz.py: match(fl, fl) before group) on the device path: a list
    matched against itself as two lists keeps the diagonal, so a string's best match is itself at 1.0 -- group_top1 of the
    device result == single_linkage of the frame, all three dicts and their order.  Then 1 500 company names the same way."""
    from polyfuzz_amd import datasets
    from polyfuzz_amd.linkage import group_top1, single_linkage
    from polyfuzz_amd.models import TFIDF
    fl = ["apple", "apples", "appl", "recal", "house", "similarity"]
    names = list(dict.fromkeys(datasets.load_company_names()))[:1500]
    for strings in (fl, names):
        m = TFIDF(min_similarity=0)
        result = m.match_device(strings, strings)
        frame = m.match(strings, strings)
        got = group_top1(result, strings, thr)
        _same_dicts(got, single_linkage(frame, thr))
        idx, val = result.download()
        own = (idx[:, 0] == np.arange(len(strings))).mean()
        assert own > 0.9, own                               # (the case is what it claims to be: nearly every row points at itself)
        if strings is fl:
            assert own == 1.0 and got[0] == {0: ["apple"], 1: ["apples"], 2: ["appl"], 3: ["recal"], 4: ["house"], 5: ["similarity"]}


# ---- k_pr_hist ---------------------------------------------------------------------------

def _exact_suffix_sums(sorted_desc):
    """exact sums of the first 1, 2, ... values as (int array, e): sum_j = ints[j] * 2^e"""
    m, e = np.frexp(sorted_desc)
    mant = (m * 2.0 ** 53).astype(np.int64)                  # exact: 53-bit mantissas
    e = e.astype(np.int64) - 53
    e0 = int(e[mant != 0].min()) if (mant != 0).any() else 0
    shift = np.where(mant != 0, e - e0, 0)
    ints = np.array([int(a) << int(s) for a, s in zip(mant.tolist(), shift.tolist())], dtype=object)
    return np.cumsum(ints) if len(ints) else ints, e0


def _check_curve(ctx, sims, thr, exact=None):
    """counts == numpy's; |sum - exact sum| within count * 2^(e - 62) + |exact sum| * 2^-52; three calls agree to the byte"""
    from polyfuzz_amd import _lib
    sims, thr = np.asarray(sims, np.float64), np.asarray(thr, np.float64)
    count, ssum = _lib.pr_curve(ctx, sims, thr)
    for _ in range(2):
        c2, s2 = _lib.pr_curve(ctx, sims, thr)
        assert c2.tobytes() == count.tobytes() and s2.tobytes() == ssum.tobytes()
    v = np.sort(sims[~np.isnan(sims)])[::-1]                 # descending: the values >= p are a prefix
    want = len(v) - np.searchsorted(v[::-1], thr, side="left")
    np.testing.assert_array_equal(count, want)
    if len(v) * len(thr) <= 20_000_000:
        np.testing.assert_array_equal(count, (v[:, None] >= thr[None, :]).sum(0))
    else:
        some = np.unique(np.linspace(0, len(thr) - 1, 16).astype(int))
        np.testing.assert_array_equal(count[some], (v[:, None] >= thr[None, some]).sum(0))
    step, e = pr_error_bound(len(sims), float(np.abs(v).max()) if len(v) else 0.0)
    ints, e0 = exact if exact is not None else _exact_suffix_sums(v)
    worst = 0.0
    for k in range(len(thr)):
        c = int(want[k])
        total = int(ints[c - 1]) if c else 0
        fsum = math.ldexp(total, e0) if abs(total) < 2 ** 53 else float(total) * 2.0 ** e0     # int -> float rounds to nearest
        if len(v) <= 2000:
            assert fsum == math.fsum(v[:c].tolist())
        bound = c * step + abs(fsum) * 2.0 ** -52
        assert abs(float(ssum[k]) - fsum) <= bound, (k, thr[k], c, ssum[k], fsum, bound)
        worst = max(worst, abs(float(ssum[k]) - fsum) / bound if bound else 0.0)
    return count, ssum, worst


def _thresholds(n_thr):
    return {1: np.array([0.5]), 2: np.array([0.25, 0.75])}.get(n_thr, np.linspace(0.0, 1.0, n_thr))


@pytest.fixture(scope="module")
def similarities():
    """per size: uniform values in [0, 1), one in sixteen moved ONTO a threshold of the 101- or the 4096-point grid (and 0.25,
    0.5, 0.75, 1.0), one in a hundred NaN -- with the exact prefix sums of the sorted values, computed once"""
    out = {}
    for n in (0, 1, 1023, 1025, 262_144 + 7, 600_000):
        rng = np.random.default_rng(n)
        v = rng.random(n)
        on = rng.random(n) < 1 / 16
        grid = np.concatenate([np.linspace(0, 1, 101), np.linspace(0, 1, 4096), np.linspace(0, 1, 4095), [0.25, 0.5, 0.75, 1.0]])
        v[on] = rng.choice(grid, int(on.sum()))
        v[rng.random(n) < 0.01] = np.nan
        out[n] = (v, _exact_suffix_sums(np.sort(v[~np.isnan(v)])[::-1]))
    return out


@pytest.mark.parametrize("n_thr", [1, 2, 101, 4095, 4096])
@pytest.mark.parametrize("n", [0, 1, 1023, 1025, 262_144 + 7, 600_000])
def test_pr_curve_counts_and_sums(ctx, similarities, n, n_thr):
    """from no similarity to more than two grid passes (256 workgroups x 1024 threads), from one threshold to the documented
    4096 (96 KiB of LDS), values on thresholds and NaNs among them"""
    sims, exact = similarities[n]
    thr = _thresholds(n_thr)
    count, ssum, worst = _check_curve(ctx, sims, thr, exact)
    assert count[0] <= n and (np.diff(count) <= 0).all()
    if n > 200_000:
        assert np.isin(sims, thr).sum() >= (1 if n_thr <= 2 else 100)      # values do sit on thresholds
    print(f"K6 PR curve, {n} similarities, {n_thr} thresholds: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("n", [1025, 262_144 + 7])
def test_pr_curve_value_ranges_and_repeats(ctx, n):
    rng = np.random.default_rng(n + 1)
    base = rng.random(n)
    base[rng.random(n) < 0.02] = np.nan
    # repeated thresholds: equal thresholds get equal answers
    thr = np.sort(np.concatenate([np.linspace(0, 1, 11)] * 3 + [[0.5] * 8]))
    count, ssum, _ = _check_curve(ctx, base, thr)
    same = thr[1:] == thr[:-1]
    assert same.sum() >= 29 and (count[1:][same] == count[:-1][same]).all() and (ssum[1:][same] == ssum[:-1][same]).all()
    # negative values with negative thresholds (the sums pass through an unsigned add), on thresholds too
    neg = base * 4 - 3
    thr = np.linspace(-3, 1, 41)
    neg[::7] = rng.choice(thr, len(neg[::7]))
    count, ssum, _ = _check_curve(ctx, neg, thr)
    assert (ssum[:10] < 0).all() and (ssum[-10:-1] > 0).all()
    # scores in [0, 100] (EditDistance(normalize=False))
    _check_curve(ctx, np.round(base * 100, 1), np.linspace(0, 100, 101))
    if n > 2000:                                             # (the rest does not depend on the number of grid passes)
        return
    _check_curve(ctx, base, np.full(5, 0.5))
    _check_curve(ctx, -base, np.array([-0.75, -0.5, -0.5, -0.25, 0.0]))
    # every value below the first threshold, and above the last
    count, ssum, _ = _check_curve(ctx, base, np.array([1.5, 2.0, 2.0, 7.0]))
    assert not count.any() and not ssum.any() and not np.signbit(ssum).any()
    count, ssum, _ = _check_curve(ctx, base, np.array([-3.0, -1.0, -1e-300]))
    assert (count == np.count_nonzero(~np.isnan(base))).all() and (ssum == ssum[0]).all()
    # NaNs only: never >= a threshold
    count, ssum, _ = _check_curve(ctx, np.full(n, np.nan), np.linspace(0, 1, 101))
    assert not count.any() and not ssum.any()


def test_pr_curve_refusals(ctx):
    """more than 4096 thresholds, descending thresholds, no threshold, an infinite similarity: PFZ_ERR_INVALID, each time"""
    from polyfuzz_amd import _lib
    sims = np.linspace(0, 1, 50)
    bad = [(sims, np.linspace(0, 1, 4097)), (sims, np.array([0.5, 0.4])), (sims, np.linspace(1, 0, 101)), (sims, np.zeros(0)),
           (np.append(sims, np.inf), np.linspace(0, 1, 101)), (np.append(sims, -np.inf), np.linspace(0, 1, 101)),
           (np.array([np.nan, np.inf]), np.array([0.5]))]
    for s, t in bad:
        with pytest.raises(_lib.PfzError) as e:
            _lib.pr_curve(ctx, s, t)
        assert e.value.code == -1 and not isinstance(e.value, _lib.PfzUnsupported), (len(s), len(t))
    _check_curve(ctx, sims, np.linspace(0, 1, 4096))          # the context is as good as before
