"""K17 (pfz_cossim_join_dev, pfz_pairs_join_keys / pfz_pairs_components_keys, BlockedEditDistance(blocking_similarity=...)) without
a GPU: the constructor's validation, the refusals before any device call, pickling, the bindings' own refusals, the test helpers on
a hand-worked case, and the item arithmetic of polyfuzz_amd/csrc/k17_core.h compiled for the host (tests/k17_core_host.cpp) and
held to a numpy restatement."""
import inspect
import os
import pickle
import subprocess

import numpy as np
import pytest

from tests import blocked_threshold_cases as C
from tests import pairs_join_cases as P

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NAMES = ["apple inc", "apple incorporated", "pear ltd"]


def _no_device(*a, **k):
    raise AssertionError("the device was reached")


def test_constructor_validates_blocking_similarity():
    from polyfuzz_amd.models import BlockedEditDistance
    sig = inspect.signature(BlockedEditDistance.__init__)
    assert list(sig.parameters)[-1] == "blocking_similarity" and sig.parameters["blocking_similarity"].default is None
    assert list(sig.parameters)[:10] == ["self", "scorer", "candidates", "top_n", "min_similarity", "n_gram_range", "clean_string",
                                         "remove_space_ngrams", "normalize", "model_id"]      # the positional signature did not move
    assert BlockedEditDistance("jaro").blocking_similarity is None
    for good in (0, 1, 0.0, 1.0, 0.6, np.float64(0.5), np.float32(0.25), np.int64(1)):
        b = BlockedEditDistance("jaro", blocking_similarity=good).blocking_similarity
        assert type(b) is float and b == float(good)
    for bad in (True, False, float("nan"), float("inf"), "0.6", -0.1, 1.5, np.nextafter(1.0, 2.0), -1e-300, [0.6]):
        with pytest.raises(ValueError, match="blocking_similarity"):
            BlockedEditDistance("jaro", blocking_similarity=bad)
    # "ratio" ranks with the keyword as without it (match needs the table); its threshold forms stay refused
    assert BlockedEditDistance(blocking_similarity=0.6)._scorer_name == "ratio"


def test_refusals_come_before_the_device(monkeypatch):
    from polyfuzz_amd import _lib, linkage
    from polyfuzz_amd.models import BlockedEditDistance
    monkeypatch.setattr(_lib.Context, "default", classmethod(_no_device))
    m = BlockedEditDistance("ratio", blocking_similarity=0.6)
    for call in (lambda: m.join(NAMES, NAMES, 0.5), lambda: m.join(NAMES), lambda: m.components(NAMES, 0.5),
                 lambda: linkage.connected_components(NAMES, m, 0.5), lambda: m.join(NAMES, NAMES, float("nan"))):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert not isinstance(e.value, _lib.PfzError) and all(name in str(e.value) for name in P.FOUR)
    for scorer in P.FOUR:
        m = BlockedEditDistance(scorer, blocking_similarity=0.6, candidates=5000)
        for bad in (float("nan"), float("inf"), -0.1, 1.5, "0.8", None, True, [0.8]):
            with pytest.raises(ValueError, match="min_similarity"):
                m.join(NAMES, NAMES, bad)
            with pytest.raises(ValueError, match="min_similarity"):
                m.join(NAMES, None, bad, re_train=False)
            with pytest.raises(ValueError, match="min_similarity"):
                m.components(NAMES, bad)
            with pytest.raises(ValueError, match="min_similarity"):
                linkage.connected_components(NAMES, m, bad)
        # accepted -- also with more `candidates` than a table may have, which play no part: the device is what stops these
        for call in (lambda: m.join(NAMES, NAMES, 0.8), lambda: m.join(NAMES), lambda: m.components(NAMES, 1)):
            with pytest.raises(AssertionError, match="the device was reached"):
                call()
        assert m.last_counts is None and m.last_timings is None
        with pytest.raises(_lib.PfzUnsupported, match="candidates"):      # the table path keeps its limit
            BlockedEditDistance(scorer, candidates=5000).join(NAMES, [str(i) for i in range(2000)], 0.8)


def test_pickling_keeps_the_value_and_an_old_state_reads_as_none():
    from polyfuzz_amd.models import BlockedEditDistance
    m = BlockedEditDistance("jaro_winkler", candidates=8, blocking_similarity=0.6)
    m._to_dev, m._to_names = object(), ("a",)
    state = m.__getstate__()
    assert state["blocking_similarity"] == 0.6 and "_to_dev" not in state
    m._to_dev = m._to_names = None
    back = pickle.loads(pickle.dumps(m))
    assert back.blocking_similarity == 0.6 and back._scorer_name == "jaro_winkler" and back.candidates == 8 and back._to_dev is None
    old = BlockedEditDistance("jaro_winkler", candidates=8)
    state = old.__getstate__()
    del state["blocking_similarity"]                      # what a matcher pickled before the attribute existed holds
    fresh = BlockedEditDistance.__new__(BlockedEditDistance)
    fresh.__setstate__(state)
    assert fresh.blocking_similarity is None and fresh.candidates == 8


def test_bindings_refuse_without_a_library_call():
    from polyfuzz_amd import _lib
    assert _lib.PAIR_KEYS_COUNTERS == ("candidates", "scored", "pairs", "items") and _lib.PAIR_KEYS_COUNTERS[:3] == _lib.PAIR_JOIN_COUNTERS
    assert isinstance(_lib.PAIR_SLICE, int) and _lib.PAIR_SLICE >= 64
    for f, names in ((_lib.sparse_join_dev, ["ctx", "index", "from_dev", "min_similarity", "self_join", "capacity_hint", "counters"]),
                     (_lib.pairs_join_keys, ["ctx", "from_dev", "to_dev", "pairs", "scorer", "min_similarity", "capacity", "counters"]),
                     (_lib.pairs_components_keys, ["ctx", "dev", "pairs", "scorer", "min_similarity", "counters"])):
        assert list(inspect.signature(f).parameters) == names
    assert all(hasattr(_lib.DevicePairs, a) for a in ("download", "free")) and _lib.DevicePairs._free == "pfz_pairs_free"
    for bad in (float("nan"), -0.1, 1.5, "0.8", None, True):
        with pytest.raises(ValueError, match="min_similarity"):
            _lib.sparse_join_dev(None, None, None, bad)
        with pytest.raises(ValueError, match="min_similarity"):
            _lib.pairs_join_keys(None, None, None, None, "jaro", bad)
        with pytest.raises(ValueError, match="min_similarity"):
            _lib.pairs_components_keys(None, None, None, "jaro", bad)
    with pytest.raises(ValueError, match="capacity_hint"):
        _lib.sparse_join_dev(None, None, None, 0.5, capacity_hint=-1)
    for f in (lambda s: _lib.pairs_join_keys(None, None, None, None, s, 0.5), lambda s: _lib.pairs_components_keys(None, None, None, s, 0.5)):
        for bad in ("ratio", "indel", "WRatio"):
            with pytest.raises(KeyError):
                f(bad)
    from polyfuzz_amd.models import TFIDF
    assert list(inspect.signature(TFIDF.join_device).parameters) == ["self", "from_list", "to_list", "min_similarity", "re_train"]
    with pytest.raises(ValueError, match="min_similarity"):
        TFIDF().join_device(NAMES, NAMES, float("nan"))


def test_header_and_docstrings_state_the_contract():
    from polyfuzz_amd import linkage
    from polyfuzz_amd.models import BlockedEditDistance
    header = open(os.path.join(REPO, "include", "polyfuzz_hip.h")).read()
    doc = " ".join(header[header.index("---- K17"):header.index("int pfz_cossim_join_dev(")].replace("\n * ", "\n").split())
    for phrase in ("exactly ONE repeat", "a valid handle with count 0", "2^31 pairs or more", "byte for byte", "int64[4]",
                   "WORK ITEMS", "decided per item", "scored exactly once", "no key kernel, no sort", "PFZ_PAIR_RATIO is refused",
                   "a two-list handle without a to-list", "max(4096, 4 per from-row)"):
        assert phrase in doc, phrase
    assert f"at most {__import__('polyfuzz_amd')._lib.PAIR_SLICE} partners" in doc
    assert "blocking_similarity" in BlockedEditDistance.__doc__ and "blocking_similarity" in BlockedEditDistance.join.__doc__
    assert "blocking_similarity" in linkage.connected_components.__doc__


# ---- the helpers' own check ------------------------------------------------------------------------------------------------------

def test_helpers_on_a_hand_worked_case():
    sim = np.array([[0.1 * (i + j) for j in range(5)] for i in range(3)])
    row_ptr, idx = np.array([0, 2, 2, 5], np.int64), np.array([1, 4, 0, 2, 3], np.int32)
    got = C.expected_keys_join(sim, row_ptr, idx, 0.4)
    assert got[0].tolist() == [0, 1, 1, 3] and got[1].tolist() == [4, 2, 3] and got[2].tolist() == [sim[0, 4], sim[2, 2], sim[2, 3]]
    assert C.expected_keys_join(sim, row_ptr, idx, sim[2, 2])[1].tolist() == [4, 2, 3]          # equal is kept
    assert C.items_of(np.array([0, 0, 1, 257, 513, 1025]), 256) == 0 + 1 + 1 + 1 + 2
    assert C.padded_table(row_ptr, idx).tolist() == [[1, 4, -1], [-1, -1, -1], [0, 2, 3]]
    assert C.border_sizes(256) == [0, 1, 63, 64, 65, 256, 257, 512, 513] and C.border_sizes(64)[5:] == [64, 65, 128, 129]


def test_the_cases_have_the_pairs_they_are_there_for():
    """their own assertions, which read the oracle vectoriser alone (the score matrices are left to the GPU tests' session)"""
    from polyfuzz_amd import _lib
    S = _lib.PAIR_SLICE
    names, at = C.copies()
    assert len(names) == 100 and len(at) == 40
    for position, length in (("first", 20), ("last", 50), ("first", 80)):
        strings, h, partners = C.hub(position, length, S)
        assert partners == 2 * S + 40 and len(strings[h]) == length and h == (0 if position == "first" else len(strings) - 1)
    strings, h, _ = C.hub("first", 20, S, True)
    assert len(strings[-1]) >= 300


# ---- k17_core.h on the host ------------------------------------------------------------------------------------------------------

def _host_program():
    exe = os.path.join(REPO, "oracle", "_build", "k17_core_host")
    src = [os.path.join(HERE, "k17_core_host.cpp"), os.path.join(REPO, "polyfuzz_amd", "csrc", "k17_core.h"),
           os.path.join(REPO, "polyfuzz_amd", "csrc", "k16_core.h")]
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                               src[0], "-o", exe])
    return exe


def _items_by_numpy(row_ptr, S):
    out = []
    for r in range(len(row_ptr) - 1):
        p0, p1 = int(row_ptr[r]), int(row_ptr[r + 1])
        if S <= 0:
            out += [(r, p0, p1)] if p1 > p0 else []
            continue
        starts = np.arange(p0, p1, S)
        out += [(r, int(q), int(min(q + S, p1))) for q in starts]
    return out


def test_item_arithmetic_on_the_host():
    from polyfuzz_amd import _lib
    exe = _host_program()
    rng = np.random.default_rng(17)
    for S in (_lib.PAIR_SLICE, 64, 1, 7, 0):
        for n in (0, 1, 5, 300):
            unit = max(S, 1)
            lens = rng.choice(np.array([0, 0, 1, unit - 1, unit, unit + 1, 2 * unit, 2 * unit + 1, 3 * unit, 5 * unit + 3]), size=n)
            row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            text = f"{S} {n}\n" + " ".join(map(str, row_ptr.tolist())) + "\n"
            out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
            assert out.returncode == 0, out.stdout + out.stderr
            lines = out.stdout.split("\n")
            assert int(lines[0]) == _lib.PAIR_SLICE                      # the binding's constant is the header's
            items, bound = map(int, lines[1].split())
            want = _items_by_numpy(row_ptr, S)
            got = [tuple(map(int, ln.split())) for ln in lines[2:] if ln]
            assert got == want and items == len(want) <= bound, (S, n)
            if S > 0 and n:
                assert items == C.items_of(row_ptr, S)
                per = np.diff(row_ptr)
                assert all(p1 - p0 == S for r, p0, p1 in got if p1 != row_ptr[r + 1]) and all(0 < p1 - p0 <= S for _, p0, p1 in got)
                if n == 300:
                    assert (per == 0).any() and ((per > 0) & (per % S == 0)).any()      # empty rows, exact multiples of S
    # near the 32-bit end: one row of 2^31 - 1 keys
    text = f"{2 ** 20} 1\n0 {2 ** 31 - 1}\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")
    assert int(lines[1].split()[0]) == 2 ** 11 and lines[-2].split() == ["0", str(2 ** 31 - 2 ** 20), str(2 ** 31 - 1)]
