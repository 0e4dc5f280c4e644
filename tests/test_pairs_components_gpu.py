"""GPU parity of K16's components (pfz_pairs_components) and of BlockedEditDistance.components: one int32 label per string, the
smallest position in its connected component of the graph whose edges are the self-join's hits over the symmetrised candidate table
== a host union-find over the definition restated in tests/pairs_join_cases.py on the CPU oracles' scores, and over the join's own
CSR.  Every comparison is ==."""
import numpy as np
import pytest

from tests import pairs_join_cases as C

pytestmark = pytest.mark.gpu


def _check(ctx, strings, sims, tab, what):
    from polyfuzz_amd import _lib
    n = len(strings)
    f, c = _lib.DeviceStrings.upload(ctx, strings), C.device_table(ctx, tab)
    seen = set()
    for name in C.FOUR:
        for thr in C.THRESHOLDS:
            want = C.expected_join(sims[name], tab, thr, True)
            label, pairs, components, counts = _lib.pairs_components(ctx, f, c, name, thr, counters=True)
            assert label.dtype == np.int32 and label.shape == (n,)
            np.testing.assert_array_equal(label, C.expected_labels(n, want[0], want[1]), err_msg=str((what, name, thr)))
            # ... and over the join's own CSR, whose total is `pairs`
            row_ptr, idx, _ = _lib.pairs_join(ctx, f, None, c, name, thr)
            np.testing.assert_array_equal(label, C.expected_labels(n, row_ptr, idx), err_msg=str((what, name, thr)))
            assert pairs == len(idx) == want[3]["pairs"] and counts == want[3], (what, name, thr, pairs, counts, want[3])
            assert components == len(np.unique(label)) and (label <= np.arange(n)).all()
            again = _lib.pairs_components(ctx, f, c, name, thr)
            assert again[0].tobytes() == label.tobytes() and again[1:] == (pairs, components)
            seen.add(components)
        # t = 0.0: the components of the symmetrised table itself
        i, j, _ = C.candidate_pairs(tab, n, True)
        rp = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(i, minlength=n), out=rp[1:])
        np.testing.assert_array_equal(_lib.pairs_components(ctx, f, c, name, 0.0)[0], C.expected_labels(n, rp, j))
    assert len(seen) > 2, seen                                  # (the thresholds do cut the graph differently)


def test_self_join_fixture(ctx):
    strings, sims, tab = C.self_list()
    _check(ctx, strings, sims, tab, "self")


@pytest.mark.parametrize("position,length", [("first", 20), ("first", 80), ("last", 20)])
def test_hub(ctx, position, length):
    strings, sims, tab = C.hub(position, length)
    _check(ctx, strings, sims, tab, (position, length))


def test_without_a_pair_every_string_is_its_own(ctx):
    from polyfuzz_amd import _lib
    f = _lib.DeviceStrings.upload(ctx, ["ab", "ab", "abc", ""])
    for tab in (np.full((4, 3), -1, np.int32), np.arange(4, dtype=np.int32)[:, None]):      # junk only; own indices only
        label, pairs, components, counts = _lib.pairs_components(ctx, f, C.device_table(ctx, tab), "jaro", 0.0, counters=True)
        assert label.tolist() == [0, 1, 2, 3] and (pairs, components) == (0, 4) and counts == {"candidates": 0, "scored": 0, "pairs": 0}
    label, pairs, components = _lib.pairs_components(ctx, _lib.DeviceStrings.upload(ctx, []), C.device_table(ctx, np.zeros((1, 1), np.int32)), "osa", 0.5)
    assert len(label) == 0 and (pairs, components) == (0, 0)


@pytest.mark.parametrize("name", C.FOUR)
def test_matcher_and_linkage(ctx, name):
    """BlockedEditDistance.components on the 400 titles with repeats == the union-find over the definition on the table an
    identically configured TFIDF leaves; linkage.connected_components builds its dicts from the same labels"""
    from polyfuzz_amd import linkage
    from polyfuzz_amd.models import TFIDF, BlockedEditDistance
    dup, sims = C.titles_self()
    cand = TFIDF(min_similarity=0.0, top_n=16).match_device(dup).download()[0]
    for thr in (0.5, 0.8):
        want = C.expected_join(sims[name], cand, thr, True)
        labels = C.expected_labels(len(dup), want[0], want[1])
        m = BlockedEditDistance(scorer=name, candidates=16)
        got = m.components(dup, thr)
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, labels, err_msg=str((name, thr)))
        assert m.last_counts == dict(want[3], components=len(np.unique(labels))) and set(m.last_timings) == {"tfidf", "k16", "frame"}
        assert 1 < m.last_counts["components"] < len(dup)
        np.testing.assert_array_equal(m.components(dup, thr), got)
        clusters = linkage.connected_components(dup, BlockedEditDistance(scorer=name, candidates=16), thr)
        assert clusters == linkage.dicts_from_labels(dup, got) and len(clusters[0]) > 0
    assert (BlockedEditDistance(scorer=name, candidates=16).components(dup) == C.expected_labels(
        len(dup), *C.expected_join(sims[name], cand, 0.8, True)[:2])).all()
