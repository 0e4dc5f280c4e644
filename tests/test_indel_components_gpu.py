"""GPU parity of K13's components (the connected components of "Indel similarity >= t" over one list) against the definition:
tests/indel_oracle.py's LCS table thresholded on the host and united by a plain union-find, label = smallest position.  Every
comparison is exact."""
import numpy as np
import pytest

from tests import indel_oracle
from tests.test_indel_join_gpu import THRESHOLDS
from tests.test_join_gpu import _class_lists, _self_list

pytestmark = pytest.mark.gpu


def _labels(n, pairs):
    """label[i] = the smallest position of i's component under the edges `pairs`"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i, j in pairs:
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)], np.int32)


def _oracle(sl, lcs, thr):
    """(labels int32[n], pairs, components) of the list whose LCS matrix against itself is lcs"""
    keep = (indel_oracle.sim_matrix(sl, sl, lcs) >= thr) & np.triu(np.ones(lcs.shape, bool), 1)
    i, j = np.nonzero(keep)
    labels = _labels(len(sl), zip(i.tolist(), j.tolist()))
    return labels, len(i), int((labels == np.arange(len(sl))).sum())


def _assert_components(got, want, what):
    label, pairs, components = got[:3]
    assert label.dtype == np.int32 and label.shape == want[0].shape, (what, label.dtype, label.shape)
    np.testing.assert_array_equal(label, want[0], err_msg=f"{what}: labels")
    assert (pairs, components) == want[1:], (what, pairs, components, want[1:])


@pytest.mark.parametrize("which", ("self", "ab"))
def test_labels_pairs_components_and_determinism(ctx, which):
    """the self-join list (~200 strings of 0 .. 110 characters: all three launches; > 40 repeats, '' three times) and the 300
    to-strings of the "ab" class list, at every threshold: labels, pair count (== the join's self-join total) and component count;
    the work counters are the join's; three runs give identical labels"""
    from polyfuzz_amd import _lib
    sl = _self_list() if which == "self" else _class_lists("ab")[1]
    n = len(sl)
    lcs = indel_oracle.lcs_matrix(sl, sl)
    f = _lib.DeviceStrings.upload(ctx, sl)
    seen = set()
    for thr in THRESHOLDS:
        want = _oracle(sl, lcs, thr)
        *got, work = _lib.indel_components(ctx, f, thr, counters=True)
        _assert_components(got, want, f"{which} t={thr!r}")
        *join, join_work = _lib.indel_join(ctx, f, None, thr, counters=True)
        assert got[1] == len(join[1]) and work == join_work, (thr, work, join_work)
        for _ in range(2):
            again = _lib.indel_components(ctx, f, thr)
            assert again[0].tobytes() == got[0].tobytes() and again[1:] == tuple(got[1:])
        seen.add(want[2])
        if thr == 0.0:
            assert want[2] == 1 and (want[0] == 0).all() and want[1] == n * (n - 1) // 2
    assert len(seen) >= 3                      # (the thresholds do cut the list differently)
    assert _oracle(sl, lcs, 1.0)[2] == len(set(sl))


def test_tiny_lists(ctx):
    """a list of 1, a list of 0, and a list whose strings are all equal"""
    from polyfuzz_amd import _lib
    for thr in (0.0, 0.5, 1.0):
        label, pairs, components = _lib.indel_components(ctx, _lib.DeviceStrings.upload(ctx, ["solo"]), thr)
        assert label.tolist() == [0] and (pairs, components) == (0, 1)
        label, pairs, components = _lib.indel_components(ctx, _lib.DeviceStrings.upload(ctx, []), thr)
        assert len(label) == 0 and label.dtype == np.int32 and (pairs, components) == (0, 0)
        for s in ("same", ""):
            label, pairs, components, work = _lib.indel_components(ctx, _lib.DeviceStrings.upload(ctx, [s] * 70), thr, counters=True)
            assert label.tolist() == [0] * 70 and (pairs, components) == (70 * 69 // 2, 1)
            assert work["pairs_in_window"] == work["pairs_finished"] == pairs


def test_matcher_and_linkage(ctx):
    """EditDistance(scorer="indel").components == the labels, last_counts, and linkage.connected_components builds its three dicts
    from them"""
    from polyfuzz_amd.linkage import connected_components, dicts_from_labels
    from polyfuzz_amd.models import EditDistance
    sl = _self_list()
    lcs = indel_oracle.lcs_matrix(sl, sl)
    want = _oracle(sl, lcs, 0.8)
    for normalize in (True, False):
        m = EditDistance(scorer="indel", normalize=normalize)
        label = m.components(sl)                        # the default threshold is 0.8
        np.testing.assert_array_equal(label, want[0])
        assert m.last_counts == {"pairs": want[1], "components": want[2]} and set(m.last_timings) == {"device", "frame"}
    got = connected_components(sl, EditDistance(scorer="indel"), 0.8)
    assert got == dicts_from_labels(sl, want[0]) and len(got[0]) > 3
    groups = {}
    for i, s in enumerate(sl):
        groups.setdefault(int(want[0][i]), []).append(s)
    assert sorted(map(sorted, got[0].values())) == sorted(sorted(set(g)) for g in groups.values() if len(g) > 1)
