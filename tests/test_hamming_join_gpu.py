"""K23 on the device: pfz_hamming_join against the XOR / popcount matrix of numpy (pairs and distances ==, row-major, at cutoffs
that hundreds of pairs sit exactly on), against the existing route (dense_topn on the same bit handles, every column ranked), at
the two extremes of the distance, under every capacity, and for every form the codes may be handed over in."""
import numpy as np
import pytest

from tests import hamming_join_cases as HJ

pytestmark = pytest.mark.gpu


def _tiles(n_from, n_to, self_join):
    tm, tn = -(-n_from // 128), -(-n_to // 128)
    return tm * (tm + 1) // 2 if self_join else tm * tn


@pytest.mark.parametrize("t", HJ.THRESHOLDS)
@pytest.mark.parametrize("name", HJ.CASES)
def test_pairs_and_distances_are_the_oracles(ctx, name, t):
    x, y = HJ.lists(name)
    rows, cols, dist, row_ptr, counts = HJ.join(ctx, name, t)
    want_rows, want_cols, want_dist = HJ.oracle_pairs(HJ.distances(name), HJ.HMAX[name][t])
    print(name, t, "hits", len(rows), "oracle", len(want_rows), counts)
    assert dist.dtype == np.int32 and cols.dtype == np.int32 and row_ptr.dtype == np.int64
    assert np.array_equal(rows, want_rows) and np.array_equal(cols, want_cols) and np.array_equal(dist, want_dist)      # (row-major)
    assert row_ptr[0] == 0 and row_ptr[-1] == len(cols) and len(row_ptr) == len(x) + 1 and (np.diff(row_ptr) >= 0).all()
    assert counts["pairs"] == HJ.ORACLE_HITS[name][t][0] == len(cols)
    assert int((dist == HJ.HMAX[name][t]).sum()) == HJ.ORACLE_HITS[name][t][1]
    assert counts["tiles"] == _tiles(len(x), len(x if y is None else y), y is None)
    assert (counts["hit_waves"] == 0) == (len(cols) == 0) and counts["hit_waves"] <= 4 * counts["tiles"]


@pytest.mark.parametrize("t", HJ.THRESHOLDS)
@pytest.mark.parametrize("name", HJ.CASES)
def test_agrees_with_the_existing_route(ctx, name, t):
    from polyfuzz_amd import _lib
    f, to = HJ.devs(ctx, name)
    rows, cols, dist, _, _ = HJ.join(ctx, name, t)
    e_rows, e_cols, e_val = HJ.existing_path(ctx, f, to, HJ.HMAX[name][t])
    assert np.array_equal(rows, e_rows) and np.array_equal(cols, e_cols)
    sim = _lib.hamming_similarity(dist, HJ.bits(name))
    assert sim.dtype == e_val.dtype == np.float32 and sim.tobytes() == e_val.tobytes()


def _planted(name):
    """the case's codes with ten exact copies of row 3 planted, and their positions"""
    x = HJ.lists(name)[0].copy()
    at = np.array([0, 5, 17, 40, 64, 77, 100, 127, 128, len(x) - 1])      # (both sides of the tile edge, the last row)
    x[at] = x[3]
    return x, sorted(set(at.tolist()) | {3})


@pytest.mark.parametrize("name", ["130x4104", "257x64"])
def test_distance_zero_finds_exact_copies(ctx, name):
    from polyfuzz_amd import _lib
    x, at = _planted(name)
    dev = _lib.DeviceDense.upload_bits(ctx, x)
    row_ptr, idx, dist, counts = _lib.hamming_join(ctx, dev, None, 0)
    rows, cols = HJ.csr_pairs(row_ptr, idx)
    want_rows, want_cols, _ = HJ.oracle_pairs(HJ.distances_of(x), 0)
    assert np.array_equal(rows, want_rows) and np.array_equal(cols, want_cols) and (dist == 0).all()
    among = [(i, j) for i, j in zip(rows.tolist(), cols.tolist()) if i in at and j in at]
    assert len(at) == 11 and len(among) == 55 and counts["pairs"] >= 55


@pytest.mark.parametrize("name", ["130x4104", "257x64"])
def test_distance_d_is_every_pair_under_every_capacity(ctx, name):
    from polyfuzz_amd import _lib
    f, _ = HJ.devs(ctx, name)
    n, d = f.n, HJ.bits(name)
    total = n * (n - 1) // 2
    iu = np.triu_indices(n, 1)
    h = HJ.distances(name)
    first = None
    for capacity in (1, total, total - 1, None):      # 1: the repeat protocol runs once
        row_ptr, idx, dist, counts = _lib.hamming_join(ctx, f, None, d, capacity=capacity)
        rows, cols = HJ.csr_pairs(row_ptr, idx)
        assert counts["pairs"] == total == len(idx), capacity
        assert np.array_equal(rows, iu[0]) and np.array_equal(cols, iu[1]) and np.array_equal(dist, h[iu]), capacity
        got = (row_ptr.tobytes(), idx.tobytes(), dist.tobytes())
        first = first or got
        assert got == first, capacity


def test_the_same_handle_twice_and_no_handle_are_the_self_join(ctx):
    from polyfuzz_amd import _lib
    name, t = "300x96", 0.8
    f, _ = HJ.devs(ctx, name)
    rows, cols, dist, row_ptr, counts = HJ.join(ctx, name, t)
    for to in (f, None):
        p, i, d, c = _lib.hamming_join(ctx, f, to, HJ.HMAX[name][t], counters=True)
        assert p.tobytes() == row_ptr.tobytes() and i.tobytes() == cols.tobytes() and d.tobytes() == dist.tobytes() and c == counts
    # a second handle of the same codes is two lists: both orders of every pair, and every row with itself
    other = _lib.DeviceDense.upload_bits(ctx, HJ.lists(name)[0])
    p, i, d, c = _lib.hamming_join(ctx, f, other, HJ.HMAX[name][t])
    assert c["pairs"] == 2 * counts["pairs"] + f.n
    r, _ = HJ.csr_pairs(p, i)
    assert np.array_equal(i[r < i], cols) and np.array_equal(d[r < i], dist)


def test_one_row_and_empty_lists(ctx):
    from polyfuzz_amd import _lib
    one = _lib.DeviceDense.upload_bits(ctx, np.array([[0b10110000, 1]], np.uint8))
    row_ptr, idx, dist, counts = _lib.hamming_join(ctx, one, None, 16, counters=True)
    assert row_ptr.tolist() == [0, 0] and len(idx) == 0 and counts == {"pairs": 0, "tiles": 1, "hit_waves": 0}
    flipped = _lib.DeviceDense.upload_bits(ctx, np.array([[0b10110001, 1]], np.uint8))
    for hmax, want in ((0, []), (1, [1]), (16, [1])):
        row_ptr, idx, dist, counts = _lib.hamming_join(ctx, one, flipped, hmax)
        assert row_ptr.tolist() == [0, len(want)] and idx.tolist() == [0] * len(want) and dist.tolist() == want
    none = _lib.DeviceDense.upload_bits(ctx, np.empty((0, 2), np.uint8))
    for f, to, n in ((none, one, 0), (one, none, 1), (none, None, 0), (none, none, 0)):
        row_ptr, idx, dist, counts = _lib.hamming_join(ctx, f, to, 3, counters=True)
        assert row_ptr.tolist() == [0] * (n + 1) and len(idx) == len(dist) == 0 and counts == {"pairs": 0, "tiles": 0, "hit_waves": 0}
    label, pairs, components = _lib.hamming_components(ctx, none, 3)
    assert len(label) == 0 and (pairs, components) == (0, 0)
    label, pairs, components = _lib.hamming_components(ctx, one, 3)
    assert label.tolist() == [0] and (pairs, components) == (0, 1)


def test_library_refusals(ctx):
    from polyfuzz_amd import _lib
    f, _ = HJ.devs(ctx, "257x64")
    narrow = _lib.DeviceDense.upload_bits(ctx, np.zeros((3, 4), np.uint8))
    for bad in (-1, 65, 1 << 40):
        with pytest.raises(_lib.PfzError, match="max_distance"):
            _lib.hamming_join(ctx, f, None, bad)
        with pytest.raises(_lib.PfzError, match="max_distance"):
            _lib.hamming_components(ctx, f, bad)
    with pytest.raises(_lib.PfzError, match="64 bits, to-codes 32"):
        _lib.hamming_join(ctx, f, narrow, 3)
    # the library names the type of an operand that is not binary (the binding's own gate stepped over)
    x32 = _lib.DeviceDense.upload(ctx, np.ones((3, 64), np.float32))
    x32.dtype = _lib.BINARY
    with pytest.raises(_lib.PfzError, match="float32"):
        _lib.hamming_join(ctx, x32, None, 3)
    with pytest.raises(_lib.PfzError, match="float32"):
        _lib.hamming_components(ctx, x32, 3)


def test_every_form_of_the_codes_joins_alike(ctx):
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(23)
    base = rng.standard_normal((6, 200))
    x = (base[rng.integers(0, 6, 150)] + 0.6 * rng.standard_normal((150, 200))).astype(np.float32)
    x[7, :5] = [0.0, -0.0, np.nan, 1e-30, -1e-30]
    packed = np.packbits(x > 0, axis=1)
    hmax = _lib.hamming_max_distance(200, 0.5)
    want = HJ.oracle_pairs(HJ.distances_of(packed), hmax)
    assert len(want[0]) > 500
    results = []
    for codes in (packed, (packed.astype(np.int16) - 128).astype(np.int8), x, x.astype(np.float64)):
        row_ptr, idx, dist, _ = _lib.hamming_join(ctx, _lib.DeviceDense.upload_bits(ctx, codes), None, hmax)
        rows, cols = HJ.csr_pairs(row_ptr, idx)
        assert np.array_equal(rows, want[0]) and np.array_equal(cols, want[1]) and np.array_equal(dist, want[2]), codes.dtype
        results.append((row_ptr.tobytes(), idx.tobytes(), dist.tobytes()))
    assert len(set(results)) == 1


@pytest.mark.parametrize("name", ["257x64", HJ.TWO_LIST_CASE])
def test_join_does_not_depend_on_what_the_allocator_hands_out(ctx, name):
    from polyfuzz_amd import _lib
    x, y = HJ.lists(name)
    hmax = HJ.HMAX[name][0.8]
    runs = []
    try:
        for mode in (0, 1, 2):
            ctx.pool_fill(mode)
            f = _lib.DeviceDense.upload_bits(ctx, x)
            to = None if y is None else _lib.DeviceDense.upload_bits(ctx, y)
            out = []
            for capacity in (len(x) * len(x if y is None else y), 1):
                row_ptr, idx, dist, counts = _lib.hamming_join(ctx, f, to, hmax, capacity=capacity)
                out += [row_ptr, idx, dist, np.array([counts["pairs"]], np.int64)]
            runs.append([(a.dtype, a.shape, a.tobytes()) for a in out])
    finally:
        ctx.pool_fill(0)
    assert runs[0] == runs[1] == runs[2]
    rows, cols, dist, row_ptr, _ = HJ.join(ctx, name, 0.8)
    assert runs[0][0][2] == row_ptr.tobytes() and runs[0][1][2] == cols.tobytes() and runs[0][2][2] == dist.tobytes()
