"""K14 on the GPU: pfz_dense_components (Embeddings.components) -- the labels against a ten-line union-find over the pairs of
the existing path (pfz_dense_topn) and over the float64 oracle's, their invariants, and the facade."""
import numpy as np
import pytest

from tests import dense_join_cases as C

pytestmark = pytest.mark.gpu
_devs, _join, _existing_path = C.devs, C.join, C.existing_path
_cache = {}


def _components(ctx, name, t):
    from polyfuzz_amd import _lib
    if (name, t) not in _cache:
        _cache[name, t] = _lib.dense_components(ctx, _devs(ctx, name)[0], t, counters=True)
    return _cache[name, t]


@pytest.mark.parametrize("t", C.THRESHOLDS)
@pytest.mark.parametrize("name", list(C.SELF_CASES))
def test_labels_equal_a_union_find_over_the_existing_paths_pairs(ctx, name, t):
    f, _ = _devs(ctx, name)
    label, pairs, components, counters = _components(ctx, name, t)
    rows, cols, _ = _existing_path(ctx, f, None, t)
    want = C.union_find_labels(f.n, rows, cols)
    assert label.dtype == np.int32 and label.tobytes() == want.tobytes()
    assert (label <= np.arange(f.n)).all() and (label[label] == label).all()
    assert components == len(np.unique(label)) == int((label == np.arange(f.n)).sum())
    j_counts = _join(ctx, name, t)[4]
    assert pairs == len(rows) == j_counts["pairs"]
    assert counters == {"tiles": j_counts["tiles"], "hit_corners": j_counts["hit_corners"]}


@pytest.mark.parametrize("t", C.THRESHOLDS)
@pytest.mark.parametrize("name", list(C.SELF_CASES))
def test_labels_equal_the_float64_oracles_components(ctx, oracle_mod, name, t):
    """in the cases whose band is empty the hits ARE the oracle's, and so are the components; their number is the issue's"""
    hits, band = C.oracle_counts(name, t)
    assert (hits, band) == C.ORACLE_HITS[name][t]
    cos = C.cosines(name)
    rows, cols = np.nonzero(cos >= t)
    want = C.union_find_labels(cos.shape[0], rows, cols)
    assert len(np.unique(want)) == C.ORACLE_COMPONENTS[name][t]
    label, pairs, components, _ = _components(ctx, name, t)
    print(f"{name} t={t}: device {pairs} pairs in {components} components, oracle {hits} (band {band}) in {len(np.unique(want))}")
    if band == 0:
        assert label.tobytes() == want.tobytes() and pairs == hits and components == C.ORACLE_COMPONENTS[name][t]


@pytest.mark.parametrize("name", list(C.SELF_CASES))
def test_labels_of_a_permuted_list_map_back(ctx, name):
    from polyfuzz_amd import _lib
    x, _ = C.lists(name)
    perm = np.random.default_rng(5).permutation(len(x))
    label = _components(ctx, name, 0.8)[0]
    p_label, p_pairs, p_components = _lib.dense_components(ctx, _lib.DeviceDense.upload(ctx, x[perm]), 0.8)
    assert p_components == _components(ctx, name, 0.8)[2]
    # row r of the permuted list is row perm[r] of the original: two rows share a label there iff they do here
    back = np.empty(len(x), np.int64)
    back[perm] = p_label                                              # the permuted run's label of original row i
    smallest = {}
    for i in range(len(x)):
        smallest.setdefault(int(back[i]), i)
    assert np.array([smallest[int(b)] for b in back], np.int32).tobytes() == label.tobytes()
    assert (p_label <= np.arange(len(x))).all()
    assert abs(p_pairs - _components(ctx, name, 0.8)[1]) <= C.ORACLE_HITS[name][0.8][1]      # ([j][i] for [i][j]: the band's pairs may flip)


def test_edge_inputs(ctx):
    from polyfuzz_amd import _lib
    x = C.gen(257, 40, 20, 8).copy()
    x[200] = x[3]
    x[100] = 0.0
    dev = _lib.DeviceDense.upload(ctx, x)
    label, pairs, components = _lib.dense_components(ctx, dev, 0.9)
    assert label[200] == label[3] <= 3 and label[100] == 100
    rows, cols, _ = _existing_path(ctx, dev, None, 0.9)
    assert label.tobytes() == C.union_find_labels(257, rows, cols).tobytes() and pairs == len(rows)
    label, pairs, components, counters = _lib.dense_components(ctx, _lib.DeviceDense.upload(ctx, x[:1]), 0.5, counters=True)
    assert label.tolist() == [0] and (pairs, components) == (0, 1) and counters == {"tiles": 1, "hit_corners": 0}
    label, pairs, components, counters = _lib.dense_components(ctx, _lib.DeviceDense.upload(ctx, np.zeros((0, 8), np.float32)), 0.5,
                                                               counters=True)
    assert len(label) == 0 and (pairs, components) == (0, 0) and counters == {"tiles": 0, "hit_corners": 0}
    # one direction, every row a positive multiple of it: every pair is a hit at t = 0.9999 (an fp32 sum of 32 products is off by
    # less than 32 * 2^-24 = 2e-6 relative, the three roundings around it by 2e-7) and the list is one component
    same = np.outer(np.arange(1, 141, dtype=np.float32), np.random.default_rng(3).standard_normal(32).astype(np.float32))
    label, pairs, components = _lib.dense_components(ctx, _lib.DeviceDense.upload(ctx, same), 0.9999)
    assert pairs == 140 * 139 // 2 and components == 1 and (label == 0).all()


def test_embeddings_components_and_linkage(ctx):
    from polyfuzz_amd import linkage
    from polyfuzz_amd.models import Embeddings
    x, _ = C.lists("300x96")
    names = [f"s{i}" for i in range(len(x))]
    want = _components(ctx, "300x96", 0.8)
    m = Embeddings()
    label = m.components(names, 0.8, embeddings=x)
    assert label.dtype == np.int32 and label.tobytes() == want[0].tobytes()
    assert m.last_counts == {"pairs": want[1], "components": want[2]} and set(m.last_timings) == {"device", "frame"}
    table = dict(zip(names, x))
    own = Embeddings(embedding_method=lambda strings: np.stack([table[s] for s in strings]))
    assert own.components(names, 0.8).tobytes() == label.tobytes()      # (no cosine of this case is within 1e-5 of 0.8)
    assert own.components(names, 0.8, embeddings=own._embed(names)).tobytes() == label.tobytes()
    dicts = linkage.connected_components(names, m, 0.8, embeddings=x)
    assert dicts == linkage.dicts_from_labels(names, label)
    assert linkage.connected_components(names, own, 0.8) == dicts
    clusters = dicts[0]
    assert len(clusters) == len([r for r in np.unique(label) if (label == r).sum() >= 2])
