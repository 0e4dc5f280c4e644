"""GPU parity of K12 (EditDistance.components: the connected components of "Levenshtein / OSA similarity >= t", united on the
device inside K11's self-join walk) against the definition: tests/lev_oracle.py's Wagner-Fischer table, `sim >= t` on the upper
triangle, and a ten-line union-find that hooks the larger root under the smaller (tests/test_components_cpu.py).  Every
comparison is ==: the int32 labels (label[i] = the smallest position in i's component), the pair count, the component count."""
import ctypes

import numpy as np
import pytest

from tests import lev_oracle
from tests.test_components_cpu import union_find_labels
from tests.test_join_gpu import THRESHOLDS, _edited, _rand, _self_list

pytestmark = pytest.mark.gpu

SCORERS = lev_oracle.SCORERS


def _oracle(sl, d, thr):
    """(labels int32[n], pairs, components) of the list whose distance matrix against itself is d"""
    keep = (lev_oracle.sim_matrix(sl, sl, d) >= thr) & np.triu(np.ones(d.shape, bool), 1)
    i, j = np.nonzero(keep)
    labels = union_find_labels(len(sl), zip(i.tolist(), j.tolist()))
    return labels, len(i), int((labels == np.arange(len(sl))).sum())


def _assert_components(got, want, what):
    label, pairs, components = got[:3]
    assert label.dtype == np.int32 and label.shape == want[0].shape, (what, label.dtype, label.shape)
    np.testing.assert_array_equal(label, want[0], err_msg=f"{what}: labels")
    assert (pairs, components) == want[1:], (what, pairs, components, want[1:])


def _labels_from_csr(n, row_ptr, idx):
    return union_find_labels(n, zip(np.repeat(np.arange(n), np.diff(row_ptr)).tolist(), idx.tolist()))


def _launches(ctx, name):
    return ctx.prof_get(name)[1]


@pytest.mark.parametrize("name", SCORERS)
def test_all_classes_duplicates_and_empties(ctx, name):
    """K11's self-join list (~200 strings of 0 .. 70 and one of > 100 characters: all three launches; > 40 repeats, '' three
    times) at its six thresholds: 0.0 is one component, 1.0 the equal strings only, 1 - 1/3 and its float64 successor differ by
    the pairs that score exactly that.  In the same run the pair count is K11's total and the three work counters are K11's."""
    from polyfuzz_amd import _lib
    sl = _self_list()
    n = len(sl)
    assert len(set(sl)) < n - 40 and sl.count("") >= 3 and max(map(len, sl)) > 64 and min(map(len, sl)) == 0
    d = lev_oracle.matrix(sl, sl, name)
    f = _lib.DeviceStrings.upload(ctx, sl)
    seen = set()
    for thr in THRESHOLDS:
        want = _oracle(sl, d, thr)
        *got, work = _lib.lev_components(ctx, f, name, thr, counters=True)
        _assert_components(got, want, f"{name} t={thr!r}")
        *join, join_work = _lib.lev_join(ctx, f, None, name, thr, counters=True)
        assert got[1] == len(join[1]) and work == join_work, (name, thr, got[1], len(join[1]), work, join_work)
        _assert_components(_lib.lev_components(ctx, f, name, thr), want, f"{name} t={thr!r}, no counters")
        seen.add((want[1], want[2]))
        if thr == 0.0:
            assert want[2] == 1 and want[1] == n * (n - 1) // 2 and (want[0] == 0).all()
        if thr == 1.0:
            assert want[2] == len(set(sl)) and np.array_equal(want[0], np.array([sl.index(s) for s in sl]))
    assert len(seen) == len(THRESHOLDS)                        # (every threshold is a different graph: the successor of 1 - 1/3 too)


def _run_lists():
    rng = np.random.default_rng(121)
    return [["a" * int(k) for k in rng.permutation(141)], ["a" * int(k) + "b" * (60 - int(k)) for k in rng.permutation(61)]]


@pytest.mark.parametrize("name", SCORERS)
def test_one_component_across_the_three_launches(ctx, name):
    """'a' * k for k = 0 .. 140, shuffled: at t = 0.9 the strings of 9 and more characters chain into ONE component of 132 whose
    hooks come from the 32-bit, the 64-bit and the general launch, each walking only its own rows' pairs; k = 0 .. 8 stay alone
    and '' besides: 10 components.  Also 0.8 and 0.5, against the oracle's counts."""
    from polyfuzz_amd import _lib
    sl = _run_lists()[0]
    d = lev_oracle.matrix(sl, sl, name)
    f = _lib.DeviceStrings.upload(ctx, sl)
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        for thr in (0.9, 0.8, 0.5):
            want = _oracle(sl, d, thr)
            got = _lib.lev_components(ctx, f, name, thr)
            _assert_components(got, want, f"{name} runs t={thr}")
            if thr == 0.9:
                assert got[2] == 10 and np.bincount(got[0]).max() == 132
                big = int(np.bincount(got[0]).argmax())
                lens = {len(sl[i]) for i in np.nonzero(got[0] == big)[0]}
                assert min(lens) <= 32 and any(32 < x <= 64 for x in lens) and max(lens) > 64
        ctx.sync()
        assert _launches(ctx, "k12_walk") == 3 and _launches(ctx, "k12_walk_general") == 3 and _launches(ctx, "k12_flatten") == 3
    finally:
        ctx.prof_enable(False)


@pytest.mark.parametrize("name", SCORERS)
def test_a_path(ctx, name):
    """'a' * k + 'b' * (60 - k), k = 0 .. 60, shuffled, at t = 0.98 (one edit of 60): only neighbours k, k + 1 are hits, so the
    graph is a path of 60 edges -- the deepest tree 61 nodes can make, hooked in whatever order the workgroups run"""
    from polyfuzz_amd import _lib
    sl = _run_lists()[1]
    d = lev_oracle.matrix(sl, sl, name)
    want = _oracle(sl, d, 0.98)
    assert want[1:] == (60, 1) and ((d == 1).sum() == 120)
    f = _lib.DeviceStrings.upload(ctx, sl)
    _assert_components(_lib.lev_components(ctx, f, name, 0.98), want, f"{name} path")


def _wide_list():
    """~340 strings over 300 symbols (16-bit symbols in the plan), lengths 0 .. 130, with edited copies so that there are hits"""
    from tests.test_join_gpu import _class_lists
    rng = np.random.default_rng(122)
    alpha = "".join(chr(0x400 + k) for k in range(300))
    tl = _class_lists("wide")[1]
    return tl + [_edited(rng, tl[int(k)], alpha, int(rng.integers(0, 4))) for k in rng.integers(0, len(tl), 40)]


@pytest.mark.parametrize("name", SCORERS)
def test_16_bit_symbols(ctx, name):
    from polyfuzz_amd import _lib
    sl = _wide_list()
    assert len({c for s in sl for c in s}) > 256
    d = lev_oracle.matrix(sl, sl, name)
    f = _lib.DeviceStrings.upload(ctx, sl)
    for thr in (0.0, 0.5, 0.8, 1.0):
        want = _oracle(sl, d, thr)
        _assert_components(_lib.lev_components(ctx, f, name, thr), want, f"{name} wide t={thr}")
    assert 20 <= _oracle(sl, d, 0.8)[1] < 500 and _oracle(sl, d, 0.8)[2] < len(sl) - 20


def test_general_kernel_by_table_size(ctx):
    """one code point more than the 60 KiB table holds: every string, however short, is the general kernel's -- the k12_walk_general
    profile scope shows a launch per call"""
    from polyfuzz_amd import _lib
    from tests.test_jaro_gpu import LDS_LIMIT_SYMBOLS, lds_limit_lists
    fl, tl = lds_limit_lists(LDS_LIMIT_SYMBOLS + 1, 100)
    sl = tl + fl
    assert len({c for s in sl for c in s}) == LDS_LIMIT_SYMBOLS + 1 > 7679 and min(map(len, sl)) <= 32
    f = _lib.DeviceStrings.upload(ctx, sl)
    for name in SCORERS:
        d = lev_oracle.matrix(sl, sl, name)
        ctx.prof_enable(True)
        ctx.prof_reset()
        try:
            for thr in (0.0, 0.3, 0.5, 1.0):
                _assert_components(_lib.lev_components(ctx, f, name, thr), _oracle(sl, d, thr), f"{name} table limit t={thr}")
            ctx.sync()
            assert _launches(ctx, "k12_walk") == 4 and _launches(ctx, "k12_walk_general") == 4
        finally:
            ctx.prof_enable(False)
        assert 10 <= _oracle(sl, d, 0.5)[1] and 1 < _oracle(sl, d, 0.5)[2] < len(sl)


@pytest.fixture(scope="module")
def many_rows():
    rng = np.random.default_rng(123)
    sl = _rand(rng, "abc", 4, 12, 2600)
    return sl, {name: lev_oracle.matrix(sl, sl, name) for name in SCORERS}


@pytest.mark.parametrize("name", SCORERS)
def test_a_workgroups_second_row(ctx, many_rows, name):
    """2 600 strings over 'abc' of 4 .. 12 characters: more rows than the 8 x CU-count grid of the one class they fall in, so
    workgroups serve a second row with a match table they cleared.  t = 0.9: hundreds of small components; t = 0.85: one large
    one, whose hooks meet on a few roots from the whole grid."""
    from polyfuzz_amd import _lib
    sl, ds = many_rows
    assert len(sl) > 8 * 256 and max(map(len, sl)) <= 32       # (256 CUs: a grid of 2 048 workgroups for 2 600 rows of one class)
    f = _lib.DeviceStrings.upload(ctx, sl)
    want = {thr: _oracle(sl, ds[name], thr) for thr in (0.9, 0.85)}
    sizes = {thr: np.bincount(want[thr][0]) for thr in want}
    print(f"K12 second row {name}: t=0.9 {want[0.9][1]} pairs, {(sizes[0.9] > 1).sum()} multi-member components (largest {sizes[0.9].max()}); "
          f"t=0.85 {want[0.85][1]} pairs, largest component {sizes[0.85].max()}")
    assert (sizes[0.9] > 1).sum() > 100 and sizes[0.85].max() > 500
    for thr in (0.9, 0.85):
        _assert_components(_lib.lev_components(ctx, f, name, thr), want[thr], f"{name} 2600 rows t={thr}")


def test_determinism(ctx, many_rows):
    """three calls: byte-identical labels -- the hooks race, the smallest position of a component does not -- and they are the
    labels of K11's CSR united on the host"""
    from polyfuzz_amd import _lib
    for sl, thr in ((_self_list(), 0.5), (many_rows[0], 0.85)):
        f = _lib.DeviceStrings.upload(ctx, sl)
        for name in SCORERS:
            runs = [_lib.lev_components(ctx, f, name, thr) for _ in range(3)]
            assert runs[0][1] > 0
            for other in runs[1:]:
                assert other[0].tobytes() == runs[0][0].tobytes() and other[1:] == runs[0][1:]
            row_ptr, idx, _, _ = _lib.lev_join(ctx, f, None, name, thr)
            np.testing.assert_array_equal(runs[0][0], _labels_from_csr(len(sl), row_ptr, idx))
            assert runs[0][1] == len(idx)


def _raw(ctx, f, n, scorer, thr, counters=True):
    from polyfuzz_amd import _lib
    label = np.full(n + 8, -7, np.int32)
    pairs, components = ctypes.c_int64(-7), ctypes.c_int64(-7)
    work = np.full(3 + 8, -7, np.int64) if counters else None
    rc = ctx.lib.pfz_lev_components(ctx.h, f.h, scorer, ctypes.c_double(thr), _lib._ptr(label), ctypes.byref(pairs), ctypes.byref(components),
                                    _lib._ptr(work))
    return rc, label, pairs.value, components.value, work


def test_the_raw_entry(ctx):
    """pfz_lev_components itself: exactly n labels and three counters are written, not a word behind them; out_counters NULL;
    n = 1; n = 0 writes no label and returns 0 / 0; bad arguments are PFZ_ERR_INVALID"""
    from polyfuzz_amd import _lib
    sl = _self_list()
    n = len(sl)
    f = _lib.DeviceStrings.upload(ctx, sl)
    for scorer, name in enumerate(SCORERS):
        want = _oracle(sl, lev_oracle.matrix(sl, sl, name), 0.8)
        rc, label, pairs, components, work = _raw(ctx, f, n, scorer, 0.8)
        assert rc == 0 and (label[n:] == -7).all() and (work[3:] == -7).all() and (work[:3] >= 0).all()
        _assert_components((label[:n].copy(), pairs, components), want, f"{name} raw")
        rc, label, pairs, components, _ = _raw(ctx, f, n, scorer, 0.8, counters=False)
        assert rc == 0 and (label[n:] == -7).all()
        _assert_components((label[:n].copy(), pairs, components), want, f"{name} raw, no counters")
    one = _lib.DeviceStrings.upload(ctx, ["solo"])
    rc, label, pairs, components, work = _raw(ctx, one, 1, 1, 0.0)
    assert rc == 0 and label.tolist() == [0] + [-7] * 8 and (pairs, components) == (0, 1) and work[:3].tolist() == [0, 0, 0]
    empty = _lib.DeviceStrings.upload(ctx, [])
    rc, label, pairs, components, work = _raw(ctx, empty, 0, 0, 0.5)
    assert rc == 0 and (label == -7).all() and (pairs, components) == (0, 0) and work[:3].tolist() == [0, 0, 0] and (work[3:] == -7).all()
    pairs = ctypes.c_int64(0)
    assert ctx.lib.pfz_lev_components(ctx.h, empty.h, 0, ctypes.c_double(0.5), None, ctypes.byref(pairs), ctypes.byref(pairs), None) == 0
    label, p, c = _lib.lev_components(ctx, empty, "osa", 0.3)
    assert label.dtype == np.int32 and len(label) == 0 and (p, c) == (0, 0)
    for scorer, thr in ((2, 0.5), (-1, 0.5), (0, float("nan")), (0, 1.5), (1, -0.25), (0, float("inf"))):
        assert _raw(ctx, f, n, scorer, thr)[0] == -1, (scorer, thr)
    with pytest.raises(KeyError):
        _lib.lev_components(ctx, f, "jaro", 0.5)


def test_matcher_and_linkage(ctx):
    """EditDistance.components == the oracle's labels whatever `normalize` says, last_counts are the pair and component counts;
    linkage.connected_components puts the three acme spellings -- no one of which need be every other's best partner -- in one
    cluster and leaves 'initech', which has no partner, out of every mapping"""
    from polyfuzz_amd.linkage import connected_components, dicts_from_labels
    from polyfuzz_amd.models import EditDistance
    rng = np.random.default_rng(115)
    tl = ["acme holdings ltd", "acme holding ltd", "acme holdings ltd.", "globex corp", "globex corporation", "initech", "", "umbrella"] + \
        _rand(rng, "abcdefgh ", 5, 40, 60)
    acme = {"acme holdings ltd", "acme holding ltd", "acme holdings ltd."}
    for name in SCORERS:
        want = _oracle(tl, lev_oracle.matrix(tl, tl, name), 0.85)
        results = []
        for normalize in (True, False):
            m = EditDistance(scorer=name, normalize=normalize)
            label = m.components(tl, 0.85)
            _assert_components((label, m.last_counts["pairs"], m.last_counts["components"]), want, f"{name} matcher")
            assert set(m.last_counts) == {"pairs", "components"} and m.last_timings["device"] > 0
            results.append(connected_components(tl, m, 0.85))
        assert results[0] == results[1] == dicts_from_labels(tl, want[0])
        clusters, mapping, names = results[0]
        assert len({mapping[s] for s in acme}) == 1 and set(clusters[mapping["acme holdings ltd"]]) == acme
        assert names["acme holding ltd"] == "acme holdings ltd" and mapping["acme holdings ltd"] == 1
        assert "initech" not in mapping and "initech" not in names and all("initech" not in v for v in clusters.values())
        assert np.array_equal(EditDistance(scorer=name).components(tl), _oracle(tl, lev_oracle.matrix(tl, tl, name), 0.8)[0])
