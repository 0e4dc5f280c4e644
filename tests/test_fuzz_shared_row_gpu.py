"""K7, K18 and K19 read the set-up of a from-string, the bound of a pair (first and second look), the to-string's record and the
work-counter reduction from ONE header, polyfuzz_amd/csrc/k7_row.h.  This holds the three kernels to each other and to
oracle.native.fuzz_matrix on one pair of lists that takes every piece of that header through every word class (from-strings of
one, two and four 64-bit words): the arg-max, column 0 of the top-n and the join at cutoff 0 -- int32 indices and the float64
scores' bits, compared with ==."""
import functools

import numpy as np
import pytest

from tests.test_fuzz_join_gpu import assert_join_equals, expect_join

pytestmark = pytest.mark.gpu

SCORERS = ["WRatio", "token_set_ratio", "partial_ratio", "partial_token_sort_ratio"]
WORDS = ["new", "york", "mets", "braves", "the", "atlanta", "vs", "a", "bb", "inc", "llc", "co", "yankees", "red", "sox", "x", "of",
         "los", "angeles", "dodgers", "internationalisation", "incorporated", "pharmaceuticals", "telecommunications"]
CLASSES = ((0, 64), (65, 128), (129, 256))             # characters: one, two, four words per form


def _string(rng, lo, hi):
    """tokens of WORDS joined by one or two spaces, lo <= length <= hi; now and then a letter replaced by one no word has"""
    want = int(rng.integers(max(lo, 3), hi + 1))
    s = str(rng.choice(WORDS))
    while True:
        t = s + " " * int(rng.integers(1, 3)) + str(rng.choice(WORDS))
        if len(t) > want and len(s) >= lo:
            break
        if len(t) > hi:
            continue
        s = t
    if rng.random() < 0.2:
        p = int(rng.integers(0, len(s)))
        s = s[:p] + "q" + s[p + 1:]
    return s


@functools.lru_cache(maxsize=None)
def lists():
    rng = np.random.default_rng(19)
    fl = [_string(rng, lo, hi) for lo, hi in CLASSES for _ in range(15)]
    tl = [_string(rng, lo, hi) for lo, hi in CLASSES for _ in range(46)]
    fl += ["mets mets mets new york mets", "", "   "]                     # a repeated token, the empty string, only spaces
    tl += ["new mets", "", "  "]
    return tuple(fl), tuple(tl)


def _class_counts(strings):
    return [sum(lo <= len(s) <= hi for s in strings) for lo, hi in CLASSES]


def _coarse_candidates(fl, tl):
    """to-strings with more than four distinct tokens, one of them a token of some from-string: bounded as coarse entries by the
    scorers that read tokens, and bounded again when popped"""
    from_tokens = set(t for s in fl for t in s.split())
    return [s for s in tl if len(set(s.split())) > 4 and set(s.split()) & from_tokens]


@functools.lru_cache(maxsize=None)
def truth(mode):
    import oracle
    oracle.build_native()
    fl, tl = lists()
    return oracle.native.fuzz_matrix(list(fl), list(tl), mode)


def test_the_lists_reach_every_piece():
    """plain Python on the lists themselves: no check below is vacuous"""
    fl, tl = lists()
    assert (len(fl), len(tl)) == (48, 141)
    assert _class_counts(fl) == [18, 15, 15] and _class_counts(tl) == [49, 46, 46]
    assert len(_coarse_candidates(fl, tl)) >= 20
    assert any(len(s.split()) > len(set(s.split())) for s in fl)                       # a repeated token
    assert "" in fl and "" in tl and any(s and not s.strip() for s in fl) and any(s and not s.strip() for s in tl)
    # every string is the fast kernels': at most 256 characters and 32 distinct tokens
    assert all(len(s) <= 256 and len(set(s.split())) <= 32 for s in fl + tl)


@pytest.mark.parametrize("parts", ["1", "3"])
@pytest.mark.parametrize("mode", SCORERS)
def test_three_kernels_one_answer(ctx, monkeypatch, mode, parts):
    from polyfuzz_amd import _lib
    fl, tl = map(list, lists())
    want = truth(mode)
    assert want.shape == (len(fl), len(tl))
    best = np.argmax(want, axis=1).astype(np.int32)                                    # (the first of equal maxima)
    best_bits = want[np.arange(len(fl)), best].view(np.int64)
    monkeypatch.setenv("PFZ_K7_PARTS", parts)
    f_dev, t_dev = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    idx, score = _lib.fuzz_extract_one(ctx, f_dev, t_dev, mode)
    np.testing.assert_array_equal(idx, best, err_msg=f"{mode} parts={parts} arg-max idx")
    np.testing.assert_array_equal(score.view(np.int64), best_bits, err_msg=f"{mode} parts={parts} arg-max score")
    idx, score = _lib.fuzz_topn(ctx, f_dev, t_dev, mode, 1)
    np.testing.assert_array_equal(idx[:, 0], best, err_msg=f"{mode} parts={parts} top-1 idx")
    np.testing.assert_array_equal(score[:, 0].view(np.int64), best_bits, err_msg=f"{mode} parts={parts} top-1 score")
    got = _lib.fuzz_join(ctx, f_dev, t_dev, mode, 0.0)
    assert int(got[0][-1]) == len(fl) * len(tl)
    assert_join_equals(got, expect_join(want, 0.0), f"{mode} parts={parts} join")


def test_counters_of_the_join(ctx):
    """the shared reduction: at cutoff 0 every pair is a candidate, every candidate is bounded and every bounded pair is scored"""
    from polyfuzz_amd import _lib
    fl, tl = map(list, lists())
    f_dev, t_dev = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    row_ptr, idx, score, work = _lib.fuzz_join(ctx, f_dev, t_dev, "WRatio", 0.0, counters=True)
    assert int(row_ptr[-1]) == len(fl) * len(tl)
    assert work["bounded"] == len(fl) * len(tl) and work["scored"] == work["bounded"] and work["steps"] > 0, work
