"""The work fingerprint of the Jaro pair sweep (k8_sweep.h), which K20 (JaroWinkler.join) and K21 (JaroWinkler.match(top_n=)) share:
the four work counters of either kernel == the integers tests/golden/jaro_sweep_counters.json holds, recorded with the build in
which each kernel carried its own copy of the sweep (the file names the commit).

K20's counters are a function of the input alone.  K21's are too while no list fills -- the floor then stays at the cutoff --, which
`ntop` = 64 with fewer than 64 choices at or above the cutoff in every row guarantees; the test asserts that on the oracle's matrix.
A dword's difference in where a lane is abandoned, or a sweep 2 run or skipped differently, changes `steps` or `pairs_scored`: this
holds the sweep itself, not only its results (which the parity tests of either kernel hold to the oracle)."""
import json
import os

import pytest

from tests.test_jaro_join_gpu import SCORERS, class_lists
from tests.test_join_gpu import _abandon_lists

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jaro_sweep_counters.json")
LISTS = ("ab", "wide", "abandon")
JOIN_THRESHOLDS = (0.5, 0.8, 0.9, 0.95)
TOPN = 64
# (list, scorer, cutoff) of cutoffs 0.8 and 0.9 with fewer than TOPN choices at or above the cutoff in every row; left out, because
# a row has more (the oracle's count): "ab" at 0.8 under either scorer (148, 171), "abandon" at 0.8 under Jaro-Winkler (85)
TOPN_SETTINGS = tuple((which, name, cutoff) for which in LISTS for name in SCORERS for cutoff in (0.8, 0.9)
                      if (which, cutoff) != ("ab", 0.8) and (which, name, cutoff) != ("abandon", "jaro_winkler", 0.8))


def sweep_lists(which):
    return _abandon_lists() if which == "abandon" else class_lists(which)


def join_counters(ctx, f, t, name, thr, capacity):
    from polyfuzz_amd import _lib
    work = _lib.jaro_join(ctx, f, t, name, thr, capacity=capacity, counters=True)[-1]
    return [work[k] for k in _lib.JARO_JOIN_COUNTERS]


def topn_counters(ctx, f, t, name, cutoff):
    from polyfuzz_amd import _lib
    work = _lib.jaro_topn(ctx, f, t, name, TOPN, score_cutoff=cutoff, counters=True)[-1]
    return [work[k] for k in _lib.JARO_TOPN_COUNTERS]


def measure(ctx, oracle_mod):
    """{"k20": {"list scorer t": [4 counters]}, "k21": {"list scorer cutoff": [4 counters]}} of this build"""
    from polyfuzz_amd import _lib
    out = {"k20": {}, "k21": {}}
    for which in LISTS:
        fl, tl = sweep_lists(which)
        f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
        for name in SCORERS:
            for thr in JOIN_THRESHOLDS:
                out["k20"][f"{which} {name} {thr}"] = join_counters(ctx, f, t, name, thr, len(fl) * len(tl))
            m = None
            for w, n, cutoff in TOPN_SETTINGS:
                if (w, n) != (which, name):
                    continue
                m = oracle_mod.jaro_matrix(fl, tl, name) if m is None else m
                assert (m >= cutoff).sum(axis=1).max() < TOPN, (which, name, cutoff)      # no list can fill: the floor is the cutoff
                out["k21"][f"{which} {name} {cutoff}"] = topn_counters(ctx, f, t, name, cutoff)
    return out


def test_sweep_work_is_the_recorded_work(ctx, oracle_mod):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = measure(ctx, oracle_mod)
    assert len(got["k20"]) == len(LISTS) * len(SCORERS) * len(JOIN_THRESHOLDS) and len(got["k21"]) == len(TOPN_SETTINGS) >= 8
    for kernel in ("k20", "k21"):
        assert got[kernel].keys() == want[kernel].keys()
        for key, counters in got[kernel].items():
            print(f"{kernel} {key}: {counters}")
            assert counters == want[kernel][key], (kernel, key)
            assert counters[3] > 0 and counters[2] <= counters[1] <= counters[0]
