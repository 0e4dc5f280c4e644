"""GPU parity of K18's components -- RapidFuzz.components / _lib.fuzz_components -- against a union-find over the oracle's
thresholded upper triangle, and against scipy's connected components of the join's own CSR."""
import numpy as np
import pytest

from tests.test_fuzz_join_gpu import expect_join, self_list, self_truth

pytestmark = pytest.mark.gpu


def union_find_labels(n, rows, cols):
    """label[i] = the smallest position of i's component over the edges (rows[k], cols[k])"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in zip(rows.tolist(), cols.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(i) for i in range(n)], np.int32)


@pytest.mark.parametrize("n", [1, 2, 65, 130])
@pytest.mark.parametrize("mode", ["WRatio", "token_ratio", "partial_ratio"])
def test_components_equal_union_find_over_the_oracle(ctx, mode, n):
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    from polyfuzz_amd import _lib
    names = list(self_list())[:n]
    truth = self_truth(mode)[:n, :n]
    dev = _lib.DeviceStrings.upload(ctx, names)
    for t in (0.6, 0.9, 1.0):
        row_ptr, idx, score = expect_join(truth, t * 100.0, self_join=True)
        rows = np.repeat(np.arange(n), np.diff(row_ptr))
        want = union_find_labels(n, rows, idx)
        label, pairs, components = _lib.fuzz_components(ctx, dev, mode, t * 100.0)
        assert label.dtype == np.int32
        np.testing.assert_array_equal(label, want, err_msg=f"{mode} n={n} t={t}")
        j_ptr, j_idx, _ = _lib.fuzz_join(ctx, dev, None, mode, t * 100.0)
        assert pairs == j_ptr[-1] == len(idx) and components == len(np.unique(want))
        g = sp.csr_matrix((np.ones(len(j_idx), np.int8), j_idx, j_ptr), shape=(n, n))
        n_comp, lab = connected_components(g, directed=False)
        first = np.full(n_comp, n, np.int64)
        np.minimum.at(first, lab, np.arange(n))
        np.testing.assert_array_equal(label, first[lab].astype(np.int32))
        assert n_comp == components
    again = _lib.fuzz_components(ctx, dev, mode, 60.0, counters=True)
    assert again[0].tobytes() == _lib.fuzz_components(ctx, dev, mode, 60.0)[0].tobytes() and set(again[3]) == set(_lib.FUZZ_JOIN_COUNTERS)


def test_empty_list_and_matcher_and_linkage(ctx):
    from polyfuzz_amd import _lib, linkage
    from polyfuzz_amd.models import RapidFuzz
    label, pairs, components = _lib.fuzz_components(ctx, _lib.DeviceStrings.upload(ctx, []), "WRatio", 90.0)
    assert label.shape == (0,) and pairs == components == 0
    names = list(self_list())
    labels = RapidFuzz().components(names, 0.9)
    row_ptr, idx, _ = expect_join(self_truth("WRatio"), 0.9 * 100.0, self_join=True)
    np.testing.assert_array_equal(labels, union_find_labels(len(names), np.repeat(np.arange(len(names)), np.diff(row_ptr)), idx))
    assert linkage.connected_components(names, RapidFuzz(), 0.9) == linkage.dicts_from_labels(names, labels)
    with pytest.raises(NotImplementedError):
        RapidFuzz(scorer="QRatio").components(names, 0.9)


def test_components_under_pool_fill(ctx):
    from polyfuzz_amd import _lib
    names = list(self_list())
    want = {}
    try:
        for fill in (1, 2, 3, 0):
            ctx.pool_fill(fill)
            dev = _lib.DeviceStrings.upload(ctx, names)
            for mode in ("WRatio", "partial_ratio"):
                got = _lib.fuzz_components(ctx, dev, mode, 60.0)
                want.setdefault(mode, got)
                assert got[0].tobytes() == want[mode][0].tobytes() and got[1:] == want[mode][1:], (fill, mode)
    finally:
        ctx.pool_fill(0)
    row_ptr, idx, _ = expect_join(self_truth("WRatio"), 60.0, self_join=True)
    np.testing.assert_array_equal(want["WRatio"][0], union_find_labels(len(names), np.repeat(np.arange(len(names)), np.diff(row_ptr)), idx))
