"""GPU parity of K20's components (models.JaroWinkler.components: the connected components of "Jaro / Jaro-Winkler score >= t"
over one list) against a union-find over the oracle's self-join pairs (oracle/jaro.c == tests/jaro_oracle.py): the labels, the
number of pairs and the number of components are exact."""
import numpy as np
import pytest

from tests.test_jaro_join_gpu import SCORERS, _long_strings, _want
from tests.test_join_gpu import _class_lists, _self_list

pytestmark = pytest.mark.gpu


def _labels(n, i, j):
    """label[k] = the smallest position of k's component under the edges (i, j): a union-find with the smaller root on top"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in zip(i.tolist(), j.tolist()):
        ra, rb = find(a), find(b)
        parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(k) for k in range(n)], np.int32)


def _lists(kind):
    if kind == "titles":
        from polyfuzz_amd import datasets
        return datasets.c3_lists()[1][:1500]
    if kind == "self":
        return _self_list()
    # lengths 0 .. 130 and 255 .. 300 -- all three row classes, the long groups -- with copies and near-copies (over 300 symbols
    # nothing else comes close)
    tl = _class_lists(kind)[1] + _long_strings(kind)
    return tl + [tl[5], tl[100], tl[100][:-1], tl[200][1:], tl[-1][1:], tl[-3][:-2], tl[-3][2:]]


@pytest.fixture(scope="module", params=("ab", "wide", "self", "titles"))
def listed(request, oracle_mod):
    sl = _lists(request.param)
    return request.param, sl, {name: oracle_mod.jaro_matrix(sl, sl, name) for name in SCORERS}


@pytest.mark.parametrize("name", SCORERS)
def test_labels_pairs_and_components(ctx, listed, name):
    """labels == the union-find over the oracle's pairs i < j with score >= t; pairs == the join's total; components == the
    distinct labels; the same bytes twice; the counters are the self-join's"""
    from polyfuzz_amd import _lib
    kind, sl, want_m = listed
    n = len(sl)
    dev = _lib.DeviceStrings.upload(ctx, sl)
    m = want_m[name]
    seen = []
    for thr in (0.9, 0.8, 1.0, 0.95) + ((0.0, 0.5) if kind != "titles" else ()):
        row_ptr, idx, _ = _want(m, thr, self_join=True)
        rows = np.repeat(np.arange(n), np.diff(row_ptr))
        want = _labels(n, rows, idx)
        label, pairs, components, work = _lib.jaro_components(ctx, dev, name, thr, counters=True)
        assert label.dtype == np.int32
        np.testing.assert_array_equal(label, want, err_msg=f"{kind} {name} t={thr}")
        assert pairs == len(idx) and components == len(set(want.tolist()))
        join = _lib.jaro_join(ctx, dev, None, name, thr, counters=True)
        assert len(join[1]) == pairs and join[3] == work
        again = _lib.jaro_components(ctx, dev, name, thr)
        assert again[0].tobytes() == label.tobytes() and again[1:] == (pairs, components)
        seen.append(components)
    assert seen[0] < n and seen[2] >= seen[3] >= seen[0] >= seen[1]         # (fewer components the lower the threshold)
    if kind != "titles":
        assert seen[4] == 1 and seen[5] <= seen[1]                              # t = 0: every pair is a hit, '' included


def test_pool_fill(ctx, listed):
    """the components under the allocator's fill words 0x0, 0x1 and 0x0000000100000001: the same bytes"""
    from polyfuzz_amd import _lib
    kind, sl, want_m = listed
    if kind == "titles":
        sl = sl[:400]
    seen = []
    try:
        for fill in (_lib.Context.POOL_FILL_ZERO, _lib.Context.POOL_FILL_ONE64, _lib.Context.POOL_FILL_ONE32):
            ctx.pool_fill(fill)
            label, pairs, components = _lib.jaro_components(ctx, _lib.DeviceStrings.upload(ctx, sl), "jaro_winkler", 0.85)
            seen.append(label.tobytes() + bytes([pairs % 251, components % 251]))
    finally:
        ctx.pool_fill(0)
    assert seen[0] == seen[1] == seen[2]


def test_matcher_and_connected_components(ctx, listed):
    """JaroWinkler.components returns the labels and sets last_counts / last_timings; linkage.connected_components(strings,
    JaroWinkler(), t) gives the three dicts of those labels"""
    from polyfuzz_amd.linkage import connected_components, dicts_from_labels
    from polyfuzz_amd.models import JaroWinkler
    kind, sl, want_m = listed
    n = len(sl)
    for name, winkler in (("jaro_winkler", True), ("jaro", False)):
        row_ptr, idx, _ = _want(want_m[name], 0.9, self_join=True)
        want = _labels(n, np.repeat(np.arange(n), np.diff(row_ptr)), idx)
        matcher = JaroWinkler(winkler=winkler)
        label = matcher.components(sl)                              # (the default threshold: 0.9)
        assert label.dtype == np.int32
        np.testing.assert_array_equal(label, want)
        assert matcher.last_counts == {"pairs": len(idx), "components": len(set(want.tolist()))}
        assert set(matcher.last_timings) == {"device", "frame"}
        got = connected_components(sl, JaroWinkler(winkler=winkler), 0.9)
        assert got == dicts_from_labels(sl, want)
        clusters, mapping, names = got
        assert len(clusters) >= 1 and all(len(v) >= 1 for v in clusters.values()) and all(names[s] == clusters[c][0] for s, c in mapping.items())
