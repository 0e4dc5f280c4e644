"""K23 on the device: pfz_hamming_components against the union-find over the numpy oracle's pairs, run twice, and the three ways to
the same clusters at the matcher level -- Hamming.components, linkage.connected_components and Hamming.join."""
import numpy as np
import pytest

from tests import hamming_join_cases as HJ

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("t", HJ.THRESHOLDS)
@pytest.mark.parametrize("name", list(HJ.SELF_CASES))
def test_labels_are_the_union_find_of_the_oracles_pairs(ctx, name, t):
    from polyfuzz_amd import _lib
    f, _ = HJ.devs(ctx, name)
    hmax = HJ.HMAX[name][t]
    rows, cols, _ = HJ.oracle_pairs(HJ.distances(name), hmax)
    want = HJ.union_find_labels(f.n, rows, cols)
    label, pairs, components, work = _lib.hamming_components(ctx, f, hmax, counters=True)
    print(name, t, "pairs", pairs, "components", components, work)
    assert label.dtype == np.int32 and np.array_equal(label, want) and (label <= np.arange(f.n)).all()
    assert pairs == HJ.ORACLE_HITS[name][t][0] == len(rows) and components == HJ.ORACLE_COMPONENTS[name][t] == len(np.unique(want))
    tm = -(-f.n // 128)
    assert work["tiles"] == tm * (tm + 1) // 2 and (work["hit_waves"] == 0) == (pairs == 0)
    again = _lib.hamming_components(ctx, f, hmax)
    assert again[0].tobytes() == label.tobytes() and again[1:] == (pairs, components)
    assert HJ.join(ctx, name, t)[4]["hit_waves"] == work["hit_waves"]


@pytest.mark.parametrize("how", ["min_similarity", "max_distance"])
def test_matcher_components_linkage_and_join_agree(ctx, how):
    from polyfuzz_amd import _lib, linkage
    from polyfuzz_amd.models import Hamming
    name, t = "300x96", 0.8
    x, _ = HJ.lists(name)
    strings = [f"s{i}" for i in range(len(x))]
    kw = {"min_similarity": t} if how == "min_similarity" else {"max_distance": _lib.hamming_max_distance(HJ.bits(name), t)}
    m = Hamming()
    label = m.components(strings, embeddings=x, **kw)
    assert m.last_counts == {"pairs": HJ.ORACLE_HITS[name][t][0], "components": HJ.ORACLE_COMPONENTS[name][t]}
    frame = m.join(strings, embeddings_from=x, **kw)
    assert list(frame.columns) == ["From", "To", "Similarity", "Distance"] and m.last_counts == {"pairs": HJ.ORACLE_HITS[name][t][0]}
    rows, cols, dist = HJ.oracle_pairs(HJ.distances(name), HJ.HMAX[name][t])
    assert frame["From"].tolist() == [strings[i] for i in rows] and frame["To"].tolist() == [strings[j] for j in cols]
    assert frame["Distance"].tolist() == dist.tolist() and frame["Similarity"].dtype == np.float64
    assert frame["Similarity"].to_numpy().tobytes() == _lib.hamming_similarity(dist, 96).astype(np.float64).tobytes()
    assert (frame["Similarity"] >= t).all()
    assert np.array_equal(label, HJ.union_find_labels(len(x), rows, cols))
    want = linkage.dicts_from_labels(strings, label)
    if how == "min_similarity":
        assert linkage.connected_components(strings, Hamming(), t, embeddings=x) == want
    # the frame has the columns single_linkage reads
    clusters, _, _ = linkage.single_linkage(frame, t)
    assert sum(len(v) for v in clusters.values()) <= len(x)
    # two lists through the matcher, float codes packed on the device
    y = np.unpackbits(x, axis=1)[:40].astype(np.float32) - 0.5
    two = m.join(strings[:40], strings, embeddings_from=y, embeddings_to=np.ascontiguousarray(2.0 * np.unpackbits(x, axis=1) - 1.0), **kw)
    h = HJ.distances_of(x[:40], x)
    r2, c2, d2 = HJ.oracle_pairs(h, HJ.HMAX[name][t])
    assert two["From"].tolist() == [strings[i] for i in r2] and two["To"].tolist() == [strings[j] for j in c2] and two["Distance"].tolist() == d2.tolist()


def test_matcher_match_is_embeddings_binary(ctx):
    from polyfuzz_amd.models import Embeddings, Hamming
    x, y = HJ.lists(HJ.TWO_LIST_CASE)
    fl, tl = [f"f{i}" for i in range(len(x))], [f"t{i}" for i in range(len(y))]
    e = Embeddings(min_similarity=0.0, top_n=3, cosine_method="hip")
    e.binary = "ubinary"
    want = e.match(fl, tl, embeddings_from=x, embeddings_to=y)
    got = Hamming().match(fl, tl, x, y, top_n=3)
    assert list(got.columns) == list(want.columns) and got.equals(want)


def test_components_do_not_depend_on_what_the_allocator_hands_out(ctx):
    from polyfuzz_amd import _lib
    name = "257x64"
    x, _ = HJ.lists(name)
    hmax = HJ.HMAX[name][0.8]
    runs = []
    try:
        for mode in (0, 1, 2):
            ctx.pool_fill(mode)
            label, pairs, components = _lib.hamming_components(ctx, _lib.DeviceDense.upload_bits(ctx, x), hmax)
            runs.append((label.dtype, label.tobytes(), pairs, components))
    finally:
        ctx.pool_fill(0)
    assert runs[0] == runs[1] == runs[2] and runs[0][2:] == (HJ.ORACLE_HITS[name][0.8][0], HJ.ORACLE_COMPONENTS[name][0.8])
