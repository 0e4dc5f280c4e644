"""K25 under pfz_pool_fill (tests/test_pool_fill_gpu.py explains the seam): _lib.simhash and SimHash.join / .components on the list of
257 strings with the allocator's blocks handed out as they are (mode 0) and pre-filled with each of the three words (modes 1, 2, 3).
The zero-filled run is held to the Python oracle, the others to it on their bytes: a result that differs read memory nobody wrote --
the symbol line in front of a string, a lane beyond a step's symbols, the padding of the handle's rows."""
import numpy as np
import pytest

from tests import simhash_cases as C
from tests import simhash_oracle as O

pytestmark = pytest.mark.gpu

RUNS = [(64, (3, 3), None), (128, (2, 4), "auto"), (192, (3, 3), "blocks")]      # (192 bits: half of the handle's last piece is padding)


def _run(ctx, bits, grams, index):
    """the arrays of one battery: the strings are uploaded under the fill too"""
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import SimHash
    strings = list(C.list257())
    dev = _lib.DeviceStrings.upload_packed(ctx, *_lib.pack_strings(strings))
    handle, row, windows, code = _lib.simhash(ctx, dev, _lib.TfidfParams(grams[0], grams[1], 1, 1), bits, want_bytes=True)
    out = [code, row, windows, np.array([handle.n], np.int64)]
    m = SimHash(bits=bits, n_gram_range=grams)
    m.index = index
    frame = m.join(strings, max_distance=bits // 8)
    out += [frame["Distance"].to_numpy(), frame["Similarity"].to_numpy(), np.array(frame["From"].tolist() + frame["To"].tolist()),
            np.array([m.last_counts["pairs"], m.last_counts["windowless"]], np.int64)]
    out += [m.components(strings, max_distance=bits // 8), np.array([m.last_counts["pairs"], m.last_counts["components"]], np.int64)]
    return out


@pytest.mark.parametrize("bits,grams,index", RUNS)
def test_results_do_not_depend_on_what_the_allocator_hands_out(ctx, bits, grams, index):
    strings = list(C.list257())
    try:
        runs = {}
        for mode in (1, 0, 2, 3):
            ctx.pool_fill(mode)
            runs[mode] = _run(ctx, bits, grams, index)
    finally:
        ctx.pool_fill(0)
    base = runs[1]
    code, windows, row, _ = O.fingerprints(strings, bits, grams)
    assert np.array_equal(base[0], code) and np.array_equal(base[1], row) and np.array_equal(base[2], windows)
    pos = np.flatnonzero(windows > 0)
    h = C.popcounts(code[pos], code[pos])
    r, c = np.nonzero(np.triu(h <= bits // 8, 1))
    assert len(r) > 0 and base[3][0] == len(pos) and base[4].tolist() == h[r, c].tolist()
    assert base[6].tolist() == [strings[i] for i in pos[r]] + [strings[j] for j in pos[c]]
    assert base[7].tolist() == [len(r), len(strings) - len(pos)]
    want = C.union_find_labels(len(strings), pos[r], pos[c])
    assert np.array_equal(base[8], want) and base[9].tolist() == [len(r), len(np.unique(want))]
    for mode in (0, 2, 3):
        for k, (a, b) in enumerate(zip(runs[mode], base)):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (mode, k)
