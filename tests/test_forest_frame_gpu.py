"""The forest every components entry runs on (csrc/pfz_internal.h ForestRun: parent and label, begin, flatten, the labels' download)
at the sizes where its two kernels change shape, through each of the five entries: n = 1, 65 (one lane in a second group of 64) and
257 (one thread in a second block of 256 of begin and flatten).  Two lists whose answer needs no oracle: all items equal -- one
component, label 0 everywhere, every unordered pair a hit -- and all items mutually below the threshold -- n components,
label[i] = i, no pair."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 65, 257)


def _equal_strings(n):
    return ["same"] * n


def _apart_strings(n):
    """no two share a character (nor, so, an n-gram): every similarity is 0"""
    return [chr(0x4E00 + i) * 4 for i in range(n)]


def _strings_entry(call, t_equal):
    def run(ctx, n, equal):
        from polyfuzz_amd import _lib
        dev = _lib.DeviceStrings.upload(ctx, _equal_strings(n) if equal else _apart_strings(n))
        return call(_lib, ctx, dev, t_equal if equal else 0.5)
    return run


def _dense(ctx, n, equal):
    from polyfuzz_amd import _lib
    d = max(n, 8)
    x = np.tile(np.random.default_rng(n).standard_normal(d).astype(np.float32), (n, 1)) if equal else np.eye(n, d, dtype=np.float32)
    # equal rows: an fp32 cosine of a row with itself is within a few 2^-24 of 1
    return _lib.dense_components(ctx, _lib.DeviceDense.upload(ctx, x), 0.9999 if equal else 0.5)


def _sparse(ctx, n, equal):
    from polyfuzz_amd import _lib
    from tests import sparse_join_cases
    # apart: distinct strings of three letters, each its own single 3-gram (the vectoriser keeps ASCII only)
    apart = ["".join(chr(ord("a") + i // 26 ** k % 26) for k in range(3)) for i in range(n)]
    m, dev = sparse_join_cases._fit(_equal_strings(n) if equal else apart, None, None)
    return _lib.sparse_components(ctx, m._dev_index, dev, 0.999 if equal else 0.5)


def _pairs(ctx, n, equal):
    """every other position is a row's candidate"""
    from polyfuzz_amd import _lib
    from tests import pairs_join_cases
    dev = _lib.DeviceStrings.upload(ctx, _equal_strings(n) if equal else _apart_strings(n))
    table = pairs_join_cases.device_table(ctx, np.tile(np.arange(n, dtype=np.int32), (n, 1)))
    return _lib.pairs_components(ctx, dev, table, "levenshtein", 1.0 if equal else 0.5)


ENTRIES = {
    "lev": _strings_entry(lambda _lib, ctx, dev, t: _lib.lev_components(ctx, dev, "levenshtein", t), 1.0),
    "indel": _strings_entry(lambda _lib, ctx, dev, t: _lib.indel_components(ctx, dev, t), 1.0),
    "dense": _dense,
    "sparse": _sparse,
    "pairs": _pairs,
}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_all_equal_and_all_apart(ctx, entry, n):
    label, pairs, components = ENTRIES[entry](ctx, n, True)
    assert label.dtype == np.int32 and label.tolist() == [0] * n and (pairs, components) == (n * (n - 1) // 2, 1)
    label, pairs, components = ENTRIES[entry](ctx, n, False)
    assert label.dtype == np.int32 and label.tolist() == list(range(n)) and (pairs, components) == (0, n)
