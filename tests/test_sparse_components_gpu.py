"""K15's components on the GPU: pfz_cossim_components (TFIDF.components) against a ten-line union-find over the join's CSR, the
pair count and the counters against the join's, determinism, and linkage.connected_components on a TFIDF model."""
import numpy as np
import pytest

from tests import sparse_join_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("t", C.THRESHOLDS)
@pytest.mark.parametrize("name", list(C.SELF_CASES))
def test_labels_equal_a_union_find_over_the_join(ctx, name, t):
    from polyfuzz_amd import _lib
    _, dev, index, _ = C.fitted(ctx, name)
    rows, cols, _, _, counts = C.join(ctx, name, t)
    n = dev.n_rows
    label, pairs, components, work = _lib.sparse_components(ctx, index, dev, t, counters=True)
    want = C.union_find_labels(n, rows, cols)
    assert label.dtype == np.int32 and label.tobytes() == want.tobytes()
    assert pairs == counts["pairs"] == len(rows)
    assert components == len(np.unique(want)) and (label <= np.arange(n)).all()
    assert work == {k: counts[k] for k in _lib.SPARSE_JOIN_COUNTERS}
    again = _lib.sparse_components(ctx, index, dev, t, counters=True)      # the same call twice gives the same bytes
    assert again[0].tobytes() == label.tobytes() and again[1:] == (pairs, components, work)


def test_connected_components_takes_a_tfidf_model(ctx):
    from polyfuzz_amd import _lib, linkage
    from polyfuzz_amd.models import TFIDF
    names = list(C.lists("names2600")[0])
    _, dev, index, _ = C.fitted(ctx, "names2600")
    label = _lib.sparse_components(ctx, index, dev, 0.8)[0]
    m = TFIDF(min_similarity=0.1, top_n=4)                                 # (neither plays a part)
    got = m.components(names, 0.8)
    assert got.dtype == np.int32 and got.tobytes() == label.tobytes()      # (fitted at the default block size: the same labels)
    assert m.last_counts["pairs"] == C.join(ctx, "names2600", 0.8)[4]["pairs"] and set(m.last_timings) == {"device", "frame"}
    clusters, mapping, name_map = linkage.connected_components(names, TFIDF(), 0.8)
    assert (clusters, mapping, name_map) == linkage.dicts_from_labels(names, label)
    assert len(clusters) > 100 and all(len(v) >= 1 for v in clusters.values())
