"""K24's components on the device: pfz_hamming_components_indexed against pfz_hamming_components on the same handle and against the
ten-line union-find over the numpy oracle's pairs; the pair count against the join's total; linkage.connected_components through
a matcher with `index` set."""
import numpy as np
import pytest

from tests import hamming_index_cases as C
from tests import hamming_join_cases as HJ

pytestmark = pytest.mark.gpu

SELF_INDEXABLE = [(name, t) for name, t in C.INDEXABLE if name in HJ.SELF_CASES]


@pytest.mark.parametrize("name,t", SELF_INDEXABLE)
def test_labels_equal_k23_and_the_union_find(ctx, name, t):
    from polyfuzz_amd import _lib
    x, _ = HJ.lists(name)
    dev, _ = HJ.devs(ctx, name)
    hmax = HJ.HMAX[name][t]
    label, pairs, components, counts = _lib.hamming_components_indexed(ctx, dev, hmax, counters=True)
    k_label, k_pairs, k_components = _lib.hamming_components(ctx, dev, hmax)
    rows, cols, _ = HJ.oracle_pairs(HJ.distances(name), hmax)
    assert label.dtype == np.int32 and np.array_equal(label, k_label) and np.array_equal(label, HJ.union_find_labels(len(x), rows, cols))
    assert pairs == k_pairs == HJ.ORACLE_HITS[name][t][0] and components == k_components == HJ.ORACLE_COMPONENTS[name][t]
    assert counts["checks"] == C.CHECKS[name][t] and counts["route"] == 1 and counts["blocks"] == hmax + 1


def test_planted_list_and_auto(ctx):
    from polyfuzz_amd import _lib
    x = C.planted()
    dev = _lib.DeviceDense.upload_bits(ctx, x)
    rows, cols, _ = C.oracle(x, None, 3)
    want = HJ.union_find_labels(len(x), rows, cols)
    k_label, k_pairs, k_components = _lib.hamming_components(ctx, dev, 3)
    for auto in (False, True):
        label, pairs, components, counts = _lib.hamming_components_indexed(ctx, dev, 3, auto=auto, counters=True)
        assert np.array_equal(label, want) and np.array_equal(label, k_label) and pairs == 750 == k_pairs
        assert components == k_components == len(np.unique(want)) and counts["checks"] == 3075 and counts["route"] == 1
    f, _ = HJ.devs(ctx, "300x96")
    hmax = HJ.HMAX["300x96"][0.6]
    label, pairs, components, counts = _lib.hamming_components_indexed(ctx, f, hmax, auto=True, counters=True)
    k_label, k_pairs, k_components = _lib.hamming_components(ctx, f, hmax)
    assert np.array_equal(label, k_label) and (pairs, components) == (k_pairs, k_components) == (1490, 30)
    assert counts["route"] == 0 and counts["checks"] == 50561


def test_connected_components_follow_the_index(ctx):
    from polyfuzz_amd import linkage
    from polyfuzz_amd.models import Hamming
    x, _ = HJ.lists("257x64")
    strings = [f"s{i}" for i in range(len(x))]
    m = Hamming()
    base = linkage.connected_components(strings, m, 0.9, embeddings=x)
    assert set(m.last_counts) == {"pairs", "components"}
    for index in ("blocks", "auto"):
        m.index = index
        assert linkage.connected_components(strings, m, 0.9, embeddings=x) == base
        assert m.last_counts["components"] == HJ.ORACLE_COMPONENTS["257x64"][0.9] and m.last_counts["checks"] == 1587
        assert np.array_equal(m.components(strings, max_distance=3, embeddings=x), Hamming().components(strings, max_distance=3, embeddings=x))
