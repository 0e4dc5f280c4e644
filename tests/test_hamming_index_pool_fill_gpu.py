"""K24 under pfz_pool_fill (tests/test_pool_fill_gpu.py explains the seam): the indexed join and components entries on the 257 x 64 and
200 x 1000 cases with the allocator's blocks handed out as they are (mode 0) and pre-filled with each of the three words (modes 1, 2,
3).  The zero-filled run is held to the numpy oracle, the others to it on their bytes: a result that differs read memory nobody wrote."""
import numpy as np
import pytest

from tests import hamming_index_cases as C
from tests import hamming_join_cases as HJ

pytestmark = pytest.mark.gpu

RUNS = [("257x64", 0.9, False), ("257x64", 0.6, True), ("200x1000", 0.9, False), ("200x1000", 0.8, True)]


def _run(ctx, name, t, auto):
    """the arrays of one battery: the handles are uploaded under the fill too"""
    from polyfuzz_amd import _lib
    x, y = HJ.lists(name)
    hmax = HJ.HMAX[name][t]
    f = _lib.DeviceDense.upload_bits(ctx, x)
    to = None if y is None else _lib.DeviceDense.upload_bits(ctx, y)
    row_ptr, idx, dist, counts = _lib.hamming_join_indexed(ctx, f, to, hmax, auto=auto, counters=True)
    out = [row_ptr, idx, dist, np.array([counts[k] for k in ("pairs",) + _lib.HAMMING_INDEX_COUNTERS], np.int64)]
    row_ptr, idx, dist, _ = _lib.hamming_join_indexed(ctx, f, to, hmax, auto=auto, capacity=1)      # through the repeat
    out += [row_ptr, idx, dist]
    label, pairs, components, counts = _lib.hamming_components_indexed(ctx, f, hmax, auto=auto, counters=True)
    out += [label, np.array([pairs, components] + [counts[k] for k in _lib.HAMMING_INDEX_COUNTERS], np.int64)]
    return out


@pytest.mark.parametrize("name,t,auto", RUNS)
def test_results_do_not_depend_on_what_the_allocator_hands_out(ctx, name, t, auto):
    x, y = HJ.lists(name)
    hmax = HJ.HMAX[name][t]
    try:
        runs = {}
        for mode in (1, 0, 2, 3):
            ctx.pool_fill(mode)
            runs[mode] = _run(ctx, name, t, auto)
    finally:
        ctx.pool_fill(0)
    base = runs[1]
    rows, cols, dist = HJ.oracle_pairs(HJ.distances(name), hmax)
    got_rows, got_cols = HJ.csr_pairs(base[0], base[1])
    assert np.array_equal(got_rows, rows) and np.array_equal(got_cols, cols) and np.array_equal(base[2], dist)
    assert base[3][0] == len(rows) and base[3][3] == C.CHECKS[name][t]
    fx = HJ.distances_of(x)
    r2, c2 = np.nonzero(fx <= hmax)
    assert np.array_equal(base[7], HJ.union_find_labels(len(x), r2, c2)) and base[8][0] == len(r2)
    for mode in (0, 2, 3):
        for k, (a, b) in enumerate(zip(runs[mode], base)):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (mode, k)
