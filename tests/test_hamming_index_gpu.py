"""K24 on the device: pfz_hamming_join_indexed against pfz_hamming_join on the same handles and against the XOR / popcount matrix of
numpy -- row pointers, indices and distances ==; `checks` == the numpy restatement of the rule; the block shapes that can go wrong;
a bucket of 700 equal codes; the capacity protocol; the route `auto` takes; the matcher's frames."""
import numpy as np
import pytest

from tests import hamming_index_cases as C
from tests import hamming_join_cases as HJ

pytestmark = pytest.mark.gpu


def _equal(got, want_rows, want_cols, want_dist, n_from):
    row_ptr, idx, dist, counts = got
    rows, cols = HJ.csr_pairs(row_ptr, idx)
    assert dist.dtype == np.int32 and idx.dtype == np.int32 and row_ptr.dtype == np.int64 and len(row_ptr) == n_from + 1
    assert np.array_equal(rows, want_rows) and np.array_equal(cols, want_cols) and np.array_equal(dist, want_dist)      # row-major, each once
    assert counts["pairs"] == len(want_rows) == row_ptr[-1]
    return counts


@pytest.mark.parametrize("name,t", C.INDEXABLE)
def test_forced_blocks_equal_k23_and_the_oracle(ctx, name, t):
    from polyfuzz_amd import _lib
    x, y = HJ.lists(name)
    f, to = HJ.devs(ctx, name)
    hmax = HJ.HMAX[name][t]
    got = _lib.hamming_join_indexed(ctx, f, to, hmax, counters=True)
    k_rows, k_cols, k_dist, k_ptr, _ = HJ.join(ctx, name, t)
    counts = _equal(got, *HJ.oracle_pairs(HJ.distances(name), hmax), len(x))
    print(name, t, counts)
    assert np.array_equal(got[0], k_ptr) and np.array_equal(got[1], k_cols) and np.array_equal(got[2], k_dist)
    assert counts["checks"] == C.CHECKS[name][t] and counts["route"] == 1
    assert counts["blocks"] == hmax + 1 and counts["min_block_bits"] == HJ.bits(name) // (hmax + 1)
    assert -(-counts["checks"] // 64) <= counts["items"] <= len(x) * (hmax + 1) + counts["checks"] // 64


@pytest.mark.parametrize("name,t", C.NOT_INDEXABLE)
def test_forced_blocks_refuse_what_has_no_index(ctx, name, t):
    from polyfuzz_amd import _lib
    f, to = HJ.devs(ctx, name)
    with pytest.raises(_lib.PfzError, match="256") as e:
        _lib.hamming_join_indexed(ctx, f, to, HJ.HMAX[name][t])
    assert e.value.code == -4 and isinstance(e.value, _lib.PfzUnsupported)
    with pytest.raises(_lib.PfzUnsupported, match="256"):
        _lib.hamming_components_indexed(ctx, f, HJ.HMAX[name][t])


def test_refuses_a_distance_of_all_bits(ctx):
    from polyfuzz_amd import _lib
    f, _ = HJ.devs(ctx, "257x64")
    with pytest.raises(_lib.PfzUnsupported, match="blocks"):
        _lib.hamming_join_indexed(ctx, f, None, 64)


def test_planted_list(ctx):
    from polyfuzz_amd import _lib
    x, p = C.planted(), C.PLANTED
    dev = _lib.DeviceDense.upload_bits(ctx, x)
    counts = _equal(_lib.hamming_join_indexed(ctx, dev, None, 3, counters=True), *C.oracle(x, None, 3), len(x))
    assert counts["checks"] == 3075 == p["checks"] and counts["pairs"] == 750 and counts["route"] == 1
    y = np.ascontiguousarray(x[::-1])
    to = _lib.DeviceDense.upload_bits(ctx, y)
    counts = _equal(_lib.hamming_join_indexed(ctx, dev, to, 3, counters=True), *C.oracle(x, y, 3), len(x))
    assert counts["pairs"] == 2 * 750 + len(x) and counts["checks"] == C.rule(x, y, 64, 3)[0]


@pytest.mark.parametrize("name", C.SHAPES)
def test_block_shapes(ctx, name):
    from polyfuzz_amd import _lib
    codes, d, hmax = C.shape(name)
    x = C.packed(codes)
    dev = _lib.DeviceDense.upload_bits(ctx, codes)
    assert dev.dim == d
    counts = _equal(_lib.hamming_join_indexed(ctx, dev, None, hmax, counters=True), *C.oracle(x, None, hmax), 512)
    assert counts["checks"] == C.rule(x, None, d, hmax)[0] and counts["route"] == 1 and counts["pairs"] > 0
    back = np.ascontiguousarray(codes[::-1])
    frm = _lib.DeviceDense.upload_bits(ctx, np.ascontiguousarray(codes[:100]))
    to = _lib.DeviceDense.upload_bits(ctx, back)
    counts = _equal(_lib.hamming_join_indexed(ctx, frm, to, hmax, counters=True), *C.oracle(x[:100], C.packed(back), hmax), 100)
    assert counts["checks"] == C.rule(x[:100], C.packed(back), d, hmax)[0]


def test_adversarial_768(ctx):
    from polyfuzz_amd import _lib
    y = C.adversarial768()
    dev = _lib.DeviceDense.upload_bits(ctx, y)
    row_ptr, idx, dist, counts = _lib.hamming_join_indexed(ctx, dev, None, 3, counters=True)
    assert (row_ptr.tolist(), idx.tolist(), dist.tolist(), counts["checks"]) == ([0, 1, 1], [1], [3], 4)
    row_ptr, idx, dist, counts = _lib.hamming_join_indexed(ctx, dev, None, 2, counters=True)
    assert (row_ptr.tolist(), len(idx), counts["checks"]) == ([0, 0, 0], 0, 3)


def test_heavy_bucket(ctx):
    """700 copies of one code: 244 650 pairs that agree on all four blocks, each reported once; runs many slices long"""
    from polyfuzz_amd import _lib
    x = C.heavy()
    dev = _lib.DeviceDense.upload_bits(ctx, x)
    counts = _equal(_lib.hamming_join_indexed(ctx, dev, None, 3, counters=True), *C.oracle(x, None, 3), len(x))
    assert counts["pairs"] >= 244650 and counts["checks"] >= 4 * 244650
    assert counts["items"] > len(x) * 4                                    # more items than probes
    label, pairs, components = _lib.hamming_components_indexed(ctx, dev, 3)
    assert pairs == counts["pairs"]                                        # the components count the join's pairs
    rows, cols, _ = C.oracle(x, None, 3)
    assert np.array_equal(label, HJ.union_find_labels(len(x), rows, cols)) and components == len(np.unique(label))


def test_capacity_protocol(ctx):
    from polyfuzz_amd import _lib
    x = C.planted()
    dev = _lib.DeviceDense.upload_bits(ctx, x)
    want = _lib.hamming_join(ctx, dev, None, 3)
    n = len(x)
    for auto in (False, True):
        mode = _lib.HAMMING_INDEX_AUTO if auto else _lib.HAMMING_INDEX_BLOCKS
        row_ptr = np.full(n + 1, -7, np.int64)
        idx, dist = np.full(750, -7, np.int32), np.full(750, -7, np.int32)
        total = _lib.c_i64(0)
        args = lambda cap, i, d: (ctx.h, dev.h, None, 3, mode, cap, _lib._ptr(row_ptr), _lib._ptr(i), _lib._ptr(d), _lib.ctypes.byref(total), None)
        _lib.check(ctx.lib.pfz_hamming_join_indexed(*args(100, idx, dist)))
        assert total.value == 750 and (idx == -7).all() and (dist == -7).all() and (row_ptr == -7).all()      # untouched
        _lib.check(ctx.lib.pfz_hamming_join_indexed(*args(750, idx, dist)))                                   # the repeat fills them
        assert total.value == 750 and np.array_equal(row_ptr, want[0]) and np.array_equal(idx, want[1]) and np.array_equal(dist, want[2])
        row_ptr[:] = -7
        _lib.check(ctx.lib.pfz_hamming_join_indexed(*args(0, None, None)))                                   # capacity 0, NULL outputs
        assert total.value == 750 and (row_ptr == -7).all()
        got = _lib.hamming_join_indexed(ctx, dev, None, 3, auto=auto, capacity=10)
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3]))
        assert ctx.lib.pfz_hamming_join_indexed(ctx.h, dev.h, None, 3, 0, 0, _lib._ptr(row_ptr), None, None, _lib.ctypes.byref(total), None) != 0
        assert ctx.lib.pfz_hamming_join_indexed(ctx.h, dev.h, None, 3, mode, 5, _lib._ptr(row_ptr), None, None, _lib.ctypes.byref(total), None) != 0


def test_empty_lists(ctx):
    from polyfuzz_amd import _lib
    x = C.planted()[:10]
    dev = _lib.DeviceDense.upload_bits(ctx, x)
    none = _lib.DeviceDense.upload_bits(ctx, np.zeros((0, 8), np.uint8))
    for auto in (False, True):
        row_ptr, idx, dist, counts = _lib.hamming_join_indexed(ctx, dev, none, 3, auto=auto, counters=True)
        assert row_ptr.tolist() == [0] * 11 and len(idx) == len(dist) == 0 and counts["pairs"] == counts["checks"] == 0
        row_ptr, idx, dist, counts = _lib.hamming_join_indexed(ctx, none, dev, 3, auto=auto)
        assert row_ptr.tolist() == [0] and len(idx) == 0 and counts == {"pairs": 0}
        label, pairs, components = _lib.hamming_components_indexed(ctx, none, 3, auto=auto)
        assert len(label) == 0 and pairs == components == 0
    one = _lib.DeviceDense.upload_bits(ctx, x[:1])
    row_ptr, idx, dist, counts = _lib.hamming_join_indexed(ctx, one, None, 3, counters=True)
    assert row_ptr.tolist() == [0, 0] and counts["checks"] == counts["items"] == 0 and counts["route"] == 1


def _implied_route(counts, all_pairs, d, hmax):
    from polyfuzz_amd import _lib
    return int(counts["checks"] * _lib.hamming_index_plan(d, hmax)["ratio"] <= all_pairs)


def test_auto_takes_the_route_its_rule_implies(ctx):
    from polyfuzz_amd import _lib
    x = C.planted()
    dev = _lib.DeviceDense.upload_bits(ctx, x)
    got = _lib.hamming_join_indexed(ctx, dev, None, 3, auto=True, counters=True)
    want = _lib.hamming_join(ctx, dev, None, 3)
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3]))
    assert got[3]["checks"] == 3075 and got[3]["route"] == 1 == _implied_route(got[3], C.PLANTED["all"], 64, 3)      # 1 / 2 727 of all pairs
    f, _ = HJ.devs(ctx, "300x96")
    got = _lib.hamming_join_indexed(ctx, f, None, HJ.HMAX["300x96"][0.6], auto=True, counters=True)
    rows, cols, dist, row_ptr, _ = HJ.join(ctx, "300x96", 0.6)
    assert np.array_equal(got[0], row_ptr) and np.array_equal(got[1], cols) and np.array_equal(got[2], dist)
    assert got[3]["checks"] == 50561 > C.ALL_PAIRS["300x96"]
    assert got[3]["route"] == 0 == _implied_route(got[3], C.ALL_PAIRS["300x96"], 96, 19) and got[3]["pairs"] == len(cols)
    # what has no index goes to the tiles under auto
    f, _ = HJ.devs(ctx, "130x4104")
    got = _lib.hamming_join_indexed(ctx, f, None, HJ.HMAX["130x4104"][0.8], auto=True, counters=True)
    rows, cols, dist, row_ptr, _ = HJ.join(ctx, "130x4104", 0.8)
    assert np.array_equal(got[0], row_ptr) and np.array_equal(got[1], cols) and np.array_equal(got[2], dist)
    assert got[3]["route"] == 0 and got[3]["blocks"] == 0 and got[3]["checks"] == 0


@pytest.mark.parametrize("name", ["257x64", "200x1000"])
def test_matcher_frames_are_the_same_cell_for_cell(ctx, name):
    from polyfuzz_amd.models import Hamming
    x, y = HJ.lists(name)
    names = [f"f{i}" for i in range(len(x))]
    to_names = None if y is None else [f"t{i}" for i in range(len(y))]
    m = Hamming()
    base = m.join(names, to_names, 0.9 if y is None else 0.8, x, y)
    assert set(m.last_counts) == {"pairs"}
    for index in ("blocks", "auto"):
        m.index = index
        frame = m.join(names, to_names, 0.9 if y is None else 0.8, x, y)
        assert list(frame.columns) == ["From", "To", "Similarity", "Distance"] and len(frame) == len(base)
        for col in frame.columns:
            assert frame[col].dtype == base[col].dtype and frame[col].tolist() == base[col].tolist(), (index, col)
        assert m.last_counts["pairs"] == len(base) and m.last_counts["route"] in (0, 1) and m.last_counts["checks"] > 0
        assert index != "blocks" or m.last_counts["route"] == 1
