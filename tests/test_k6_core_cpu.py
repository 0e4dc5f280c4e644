"""K6 (k_linkage_top1: the greedy single_linkage walk restated in parallel phases; k_pr_hist: the threshold histogram of
precision_recall_curve) without a GPU: the per-element decisions of polyfuzz_amd/csrc/k6_core.h compiled for the host and driven
phase by phase (tests/k6_core_host.cpp) -- every top-1 graph on up to 6 rows, rows that point at themselves included, against the
SEQUENTIAL walk; both loops within their caps; the threshold rule at the float32 neighbours of every rounding tie; the bin search
against numpy.searchsorted; the fixed point of the sums.  tests/test_k6_gpu.py runs the kernels themselves on the same shapes
(graph_shapes, tie_scores, kept_oracle below)."""
import ctypes
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
DONE, FIXPOINT_OVERRUN, JUMP_OVERRUN = 0, 1, 2              # k6_core.h: LinkStatus


@pytest.fixture(scope="module")
def host():
    so = os.path.join(REPO, "oracle", "_build", "k6_core_host.so")
    src = [os.path.join(HERE, "k6_core_host.cpp"), os.path.join(REPO, "polyfuzz_amd", "csrc", "k6_core.h")]
    os.makedirs(os.path.dirname(so), exist_ok=True)
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", src[0], "-o", so])
    lib = ctypes.CDLL(so)
    vp, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    lib.k6_host_link.restype = lib.k6_host_exhaustive.restype = ctypes.c_int
    lib.k6_host_link.argtypes = [i32, vp, vp, i32, f64, i32, i32, vp, vp, vp]
    lib.k6_host_exhaustive.argtypes = [i32, i32, i32, vp]
    lib.k6_host_kept.restype = lib.k6_host_bin.restype = None
    lib.k6_host_kept.argtypes = [vp, vp, i64, i32, f64, vp]
    lib.k6_host_bin.argtypes = [vp, i32, vp, i64, vp]
    lib.k6_host_fixed.restype = f64
    lib.k6_host_fixed.argtypes = [vp, i64, i64, f64, vp]
    return lib


def _p(x):
    return x.ctypes.data_as(ctypes.c_void_p)


# ---- shared with tests/test_k6_gpu.py ----------------------------------------------------

def tie_scores():
    """float32 [1001, 9]: for k = 0 .. 1000 the float32 nearest to k/1000 - 0.0005, to k/1000 + 0.0005 (the two rounding ties
    around k/1000) and to k/1000 itself (where `> thr` is strict for thr = k/1000), each with its two float32 neighbours"""
    k = np.arange(1001, dtype=np.float64)
    cols = []
    for t in (k / 1000 - 0.0005, k / 1000 + 0.0005, k / 1000):
        f = t.astype(np.float32)
        cols += [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    return np.stack(cols, 1)


def kept_oracle(g, v, n, thr):
    """the frame's filter: Similarity = np.round(float64(score), 3); below 0.001 or without a To the row has Similarity 0"""
    r3 = np.round(np.asarray(v, np.float32).astype(np.float64), 3)
    g = np.asarray(g)
    return (g >= 0) & (g < n) & (r3 >= 0.001) & (r3 > thr)


def graph_shapes(n, rng):
    """(name, To index per row): the shapes of the issue; rows that point at themselves are left in"""
    i = np.arange(n)
    pairs = i ^ 1
    pairs[pairs >= n] = n - 1                                # (odd n: the last row has no partner and points at itself)
    rand = rng.integers(0, n, n)
    holes = np.where(rng.random(n) < 0.1, rng.choice([-1, -7, n, n + 5], n), rng.integers(0, n, n))
    return [("random", rand), ("forward_chain", np.minimum(i + 1, n - 1)), ("backward_chain", np.maximum(i - 1, 0)),
            ("all_to_first", np.zeros(n, np.int64)), ("all_to_last", np.full(n, n - 1)), ("two_cycles", pairs), ("all_self", i),
            ("random_with_unkept", holes)]


def scores_for(n, thr, border, rng, ties=tie_scores()):
    """float32 [n] drawn from the tie neighbours.  Every score comes from k/1000 with k >= 1000 thr + 2, whose nine values all
    round above thr -- the row is kept whatever the rounding does, as long as it is done in float64 --; with `border` one row
    in eight comes from k = 1000 thr and k = 1000 thr + 1 instead, where the nine values fall on both sides of `> thr`, and
    from k = 0 and 1, where they fall on both sides of the 0.001 rule."""
    k0 = int(round(1000 * thr))
    k = rng.integers(k0 + 2, 1001, n)
    if border:
        k = np.where(rng.random(n) < 0.125, rng.choice([k0, k0 + 1, 0, 1], n), k)
    return ties[k, rng.integers(0, 9, n)]


def walk(g, kept, n, assign=None):
    """(cluster, order, foundings) of the sequential walk over the kept rows: `assign`, by default
    polyfuzz_amd.linkage._greedy_py"""
    from polyfuzz_amd.linkage import _greedy_py
    rows = np.nonzero(kept)[0].astype(np.int32)
    cluster, order = (assign or _greedy_py)(rows, np.asarray(g)[rows].astype(np.int32), n)
    return cluster, order, (int(cluster.max()) + 1 if len(rows) else 0)


def check_against_walk(g, kept, cluster, key, info, n, assign=None):
    e_cluster, e_order, e_founded = walk(g, kept, n, assign)
    np.testing.assert_array_equal(cluster, e_cluster)
    mapped = np.nonzero(cluster >= 0)[0]
    np.testing.assert_array_equal(mapped[np.argsort(key[mapped], kind="stable")], e_order)
    assert (key[cluster < 0] == -1).all()
    assert info["clusters"] == e_founded and info["rounds"] <= n + 1
    assert info["first_row"] == (np.nonzero(kept)[0][0] if kept.any() else -1)


# ---- the linkage phases ------------------------------------------------------------------

def _link(host, g, val, thr, threads=1024, rule=0):
    g = np.ascontiguousarray(g, np.int32)
    val = np.ascontiguousarray(val, np.float32)
    n, stride = g.shape[0], (1 if g.ndim == 1 else g.shape[1])
    cluster, key, info = np.full(n + 4, -9, np.int32), np.full(n + 4, -9, np.int32), np.zeros(4, np.int32)
    status = host.k6_host_link(n, _p(g), _p(val), stride, thr, threads, rule, _p(cluster), _p(key), _p(info))
    assert (cluster[n:] == -9).all() and (key[n:] == -9).all() and status == info[3]
    return status, cluster[:n], key[:n], {"first_row": int(info[0]), "rounds": int(info[1]), "clusters": int(info[2])}


@pytest.mark.parametrize("slices", [1024, 4], ids=("one_row_per_slice", "two_rows_per_slice"))
def test_every_top1_graph_on_up_to_6_rows(host, slices):
    """all 2 + 9 + 64 + 625 + 7 776 + 117 649 = 126 125 assignments g_i in {-1, 0 .. n-1}, n = 1 .. 6: cluster == the sequential
    walk's, the mapped strings sorted by key == its insertion order, the founding count, the activity loop within n + 1 rounds and
    the pointer jumping within ceil(log2 n) + 2 on every graph.  With 4 slices the founding scan has two rows per slice."""
    report = np.zeros(8, np.int64)
    assert host.k6_host_exhaustive(6, slices, 0, _p(report)) == 0
    assert report[0] == sum((n + 1) ** n for n in range(1, 7)) == 126125
    assert report[1] == 0 and report[2] == 0 and report[7] == 0, report.tolist()
    assert report[3] == 0 and report[4] == 0 and report[5] <= 0 and report[6] <= 0, report.tolist()
    print(f"K6 host, {slices} slices: fixpoint rounds - (n + 1) <= {report[5]}, jumping rounds - cap <= {report[6]}")


def test_every_top1_graph_on_7_rows(host):
    """the 2 097 152 assignments on 7 rows on top (8 slices: one row each)"""
    report = np.zeros(8, np.int64)
    assert host.k6_host_exhaustive(7, 8, 0, _p(report)) == 0
    assert report[0] == 126125 + 8 ** 7 and not report[[1, 2, 3, 4, 7]].any() and report[5] <= 0 and report[6] <= 0, report.tolist()


def test_caps_catch_the_rule_that_spun(host):
    """the activity rule as it stood before rows with To == From were served (fin[x] > x: such a row turns inactive, then active
    again, for ever) ends at the cap of the host driver on 53 970 of the 126 125 graphs and is right on every other one; the
    smallest case is idx = [0, 1]"""
    report = np.zeros(8, np.int64)
    assert host.k6_host_exhaustive(6, 1024, 1, _p(report)) == 0
    assert report[3] == 53970 and report[1] == 0 and report[2] == 0 and report[4] == 0, report.tolist()
    two = (np.array([0, 1]), np.array([0.9, 0.9], np.float32), 0.5)
    assert _link(host, *two, rule=1)[0] == FIXPOINT_OVERRUN
    status, cluster, key, info = _link(host, *two)
    assert status == DONE and cluster.tolist() == [0, 1] and info == {"first_row": 0, "rounds": 1, "clusters": 2}


def test_phases_equal_greedy_py(host):
    """the host program's own walk is not the only judge: every graph on up to 4 rows and the issue's shapes at sizes around the
    slice borders (4 slices: up to 17 rows each), straight against polyfuzz_amd.linkage._greedy_py -- with scores on both sides
    of the threshold rule, To indices outside [0, n), and three ranks per row of which only rank 0 counts"""
    import itertools
    rng = np.random.default_rng(6)
    n_graphs = 0
    for n in (1, 2, 3, 4):
        for g in itertools.product(range(-1, n), repeat=n):
            g = np.array(g)
            status, cluster, key, info = _link(host, g, np.full(n, 0.5, np.float32), 0.3, threads=2)
            assert status == DONE
            check_against_walk(g, g >= 0, cluster, key, info, n)
            n_graphs += 1
    assert n_graphs == 2 + 9 + 64 + 625
    for n in (1, 2, 3, 5, 8, 9, 63, 64, 65):
        for name, g in graph_shapes(n, rng):
            for thr in (0.0, 0.3, 0.75):
                val = scores_for(n, thr, True, rng)
                kept = kept_oracle(g, val, n, thr)
                status, cluster, key, info = _link(host, g, val, thr, threads=4)
                assert status == DONE, (n, name, thr)
                check_against_walk(g, kept, cluster, key, info, n)
                g3 = np.stack([g, np.roll(np.arange(n), 1), rng.integers(-9, n + 9, n)], 1)
                v3 = np.stack([val, np.ones(n, np.float32), rng.random(n).astype(np.float32)], 1)
                again = _link(host, g3, v3, thr, threads=4)
                assert again[0] == DONE and again[3] == info
                assert again[1].tobytes() == cluster.tobytes() and again[2].tobytes() == key.tobytes()


@pytest.mark.parametrize("n", [1023, 1025, 2049])
def test_long_chains_stay_within_the_caps(host, n):
    """the shapes with the most rounds, several rows per slice: the forward chain settles one row per activity round, the backward
    chain the most pointer jumping"""
    rng = np.random.default_rng(n)
    for name, g in graph_shapes(n, rng):
        val = scores_for(n, 0.3, False, rng)
        status, cluster, key, info = _link(host, g, val, 0.3)
        assert status == DONE, name
        check_against_walk(g, kept_oracle(g, val, n, 0.3), cluster, key, info, n)
        if name == "forward_chain":
            assert n // 2 <= info["rounds"] <= n + 1


# ---- the threshold rule ------------------------------------------------------------------

def test_kept_row_at_every_rounding_tie(host):
    """kept_row == (np.round(float64(v), 3) >= 0.001 and np.round(float64(v), 3) > thr) for the float32 values next to
    k/1000 +- 0.0005 and to k/1000, k = 0 .. 1000, at thr = 0, 0.3, 0.75 and at thr = k/1000 itself; an index outside [0, n) is
    never kept"""
    ties = tie_scores()
    assert ties.shape == (1001, 9) and ties.dtype == np.float32 and len(np.unique(ties)) > 6000
    v = np.ascontiguousarray(ties.ravel())
    g = np.zeros(len(v), np.int32)
    out = np.zeros(len(v), np.uint8)
    n_kept = 0
    for thr in [0.0, 0.3, 0.75] + [k / 1000 for k in range(1001)]:
        host.k6_host_kept(_p(g), _p(v), len(v), 1, thr, _p(out))
        r3 = np.round(v.astype(np.float64), 3)
        want = (r3 >= 0.001) & (r3 > thr)
        assert np.array_equal(out.astype(bool), want), (thr, v[out.astype(bool) != want][:5])
        n_kept += int(want.sum())
    assert 0.4 < n_kept / (1004 * len(v)) < 0.6                # (both answers are well represented)
    # the ties really are ties: around each, the three neighbours do not all round alike
    r3 = np.round(ties.astype(np.float64), 3)
    assert ((r3[:, 0:3].max(1) > r3[:, 0:3].min(1)) | (r3[:, 3:6].max(1) > r3[:, 3:6].min(1))).mean() > 0.9
    for bad in (-1, -7, 5, 10, 2 ** 31 - 1, -2 ** 31):
        gb = np.full(len(v), bad, np.int32)
        host.k6_host_kept(_p(gb), _p(v), len(v), 5, 0.0, _p(out))
        assert not out.any()
    g4 = np.full(len(v), 4, np.int32)
    host.k6_host_kept(_p(g4), _p(v), len(v), 5, 0.0, _p(out))
    assert np.array_equal(out.astype(bool), kept_oracle(g4, v, 5, 0.0)) and out.any()


# ---- the PR curve ------------------------------------------------------------------------

def test_bin_search_is_searchsorted_right(host):
    """pr_bin == numpy.searchsorted(thr, v, side="right") for ascending thresholds with repeats: values on, between, below and
    above the thresholds, one threshold, all thresholds equal, 4096 of them, negative ones"""
    rng = np.random.default_rng(66)
    sets = [np.array([0.5]), np.array([0.25, 0.25]), np.full(7, 0.5), np.linspace(0, 1, 101), np.linspace(-3, 3, 4096),
            np.sort(rng.integers(0, 20, 300) / 20.0), np.sort(np.concatenate([rng.random(50), rng.random(50)[:20], [-1.5, -1.5]]))]
    for thr in sets:
        thr = np.ascontiguousarray(thr, np.float64)
        mid = (thr[1:] + thr[:-1]) / 2
        v = np.concatenate([thr, mid, np.nextafter(thr, -np.inf), np.nextafter(thr, np.inf), [thr[0] - 1, thr[-1] + 1, -1e300, 1e300,
                                                                                              -0.0, 0.0], rng.random(500) * 2 - 0.5])
        v = np.ascontiguousarray(v, np.float64)
        out = np.full(len(v), -1, np.int32)
        host.k6_host_bin(_p(thr), len(thr), _p(v), len(v), _p(out))
        np.testing.assert_array_equal(out, np.searchsorted(thr, v, side="right"))
        assert out.min() == 0 and out.max() == len(thr)


def pr_error_bound(n, max_abs):
    """2^(e - 62): the most one value moves when it is rounded to the fixed point of (n values, largest magnitude max_abs)"""
    e = math.frexp(max(n, 1) * (max_abs if max_abs > 0 else 1.0))[1]
    return math.ldexp(1.0, e - 62), e


def test_fixed_point_conversion(host):
    """scale = 2^(61 - e) with e from frexp(n * max|v|); every value is rounded once, to the nearest multiple of 1 / scale: it
    moves by at most 2^(e - 62); n values of the largest magnitude sum to less than 2^61; the sign survives the unsigned add"""
    rng = np.random.default_rng(7)
    for n, hi in ((1, 1.0), (1000, 1.0), (600_000, 100.0), (3, 1e-3), (1 << 30, 1e6), (5, 0.0)):
        v = np.ascontiguousarray(np.concatenate([(rng.random(2000) * 2 - 1) * hi, [hi, -hi, 0.0, hi / 3, -hi / 7]]))
        fixed = np.zeros(len(v), np.int64)
        scale = host.k6_host_fixed(_p(v), len(v), n, hi, _p(fixed))
        bound, e = pr_error_bound(n, hi)
        assert scale == math.ldexp(1.0, 61 - e) and bound == 0.5 / scale
        for x, f in zip(v.tolist(), fixed.tolist()):            # in exact rationals: the nearest integer to x * scale
            assert abs(f - Fraction(x) * Fraction(scale)) <= Fraction(1, 2), (n, hi, x, f)
        assert abs(int(fixed[2000])) * max(n, 1) < 2 ** 61 and int(fixed[2000]) == -int(fixed[2001])


def test_headers_and_documents_say_what_a_self_pointing_row_does():
    header = open(os.path.join(REPO, "include", "polyfuzz_hip.h")).read()
    k6 = header[header.index("int pfz_pr_curve_host("):header.index("int pfz_linkage_top1(")]
    assert "To == From" in k6 and "founds a cluster with itself" in k6 and "PFZ_ERR_UNSUPPORTED" in k6
    from polyfuzz_amd.linkage import group_top1
    assert "two lists" in group_top1.__doc__
    kernel = open(os.path.join(REPO, "polyfuzz_amd", "csrc", "k6_reductions.hip")).read()
    assert kernel.count("for (;;)") == 2 and "link_round_cap(n)" in kernel and "link_jump_cap(n)" in kernel
    core = open(os.path.join(REPO, "polyfuzz_amd", "csrc", "k6_core.h")).read()
    for fn in ("kept_row", "link_initial_state", "link_active", "link_founding", "link_founded", "link_pointer", "link_patch_cluster0",
               "pr_bin", "pr_scale", "pr_fixed"):           # the kernels call the functions the host program checks, and define none
        assert fn + "(" in kernel.split("#include \"k6_core.h\"")[1] and "K6_HD" in core[:core.index(" " + fn + "(")].splitlines()[-1], fn
