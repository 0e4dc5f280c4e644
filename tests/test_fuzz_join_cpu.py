"""K18 -- the threshold join over K7's scorers (RapidFuzz.join / .components, _lib.fuzz_join / fuzz_components) -- without a GPU:
  * a FIXED floor loses no hit: k7_core.h's fz_score and fz_upper_bound (compiled for the host by tests/k7_core_host.cpp) with the
    same constant as every row's `cur` -- what k7_join_kernel hands them -- against oracle/fuzz_scorers.c;
  * k18_core.h (tests/k18_core_host.cpp): the packed hit at its borders, the hit rule and the prune rule around an attained score;
  * _lib.fuzz_join's capacity protocol against a fake library;
  * the matcher's argument checks and documents with the device unreachable."""
import ctypes
import math
import os
import pickle
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from polyfuzz_amd import _lib
from tests import k7_prep
from tests.test_join_capacity_cpu import N_FROM, FakeLib, _strings
from tests.test_k7_core_cpu import CASES, MODES, SLACK, _lists, host, run_pairs      # noqa: F401  (host: the fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

# the constant floors of the check: 0.29 * 100 is 28.999999999999996 -- the Python layer's expression, as it stands
FLOORS = (0.0, 0.29 * 100, 60.0, 85.5, 90.0, 95.0, 100.0)


def _case_lists(W, seed, long_words):
    """the lists of tests/test_k7_core_cpu.py::test_score_and_bound_vs_oracle for one of its CASES"""
    from polyfuzz_amd import datasets
    fl, tl = _lists(seed, 40, 90, long_words)
    titles_f, titles_t = datasets.c3_lists(60)
    fl += titles_f[:25] + ["this is a test", "fuzzy was a bear", "", "a", "mets mets mets new", "zzz", "  ", " "]
    tl += titles_t[:50] + ["this is a new test!!!", "fuzzy fuzzy was a bear", "", "this is a test!", "new mets", "a\tb  a", " ", "   ", "\t "]
    if W == 1:
        fl = [s for s in fl if len(s) <= 64]
    fl = [s for s in fl if len(s) <= 64 * W and len(set(s.split())) <= 32]
    return fl, tl


@pytest.mark.parametrize("W,seed,long_words", CASES)
def test_a_fixed_floor_loses_no_hit(host, oracle_mod, W, seed, long_words):     # noqa: F811
    """cur[i] = c for every row: {score >= c} == {oracle >= c}, the score bits of every hit are the oracle's, and the bound (with
    its slack, against the float32 of c -- the kernel's comparison) keeps every hit.  All seven scorers, the window sweeps in one
    piece and shared out in runs of 16 W, the seven constant floors and every twelfth attained score."""
    fl, tl = _case_lists(W, seed, long_words)
    alpha = k7_prep.Alphabet(tl)
    A, B = k7_prep.prepare(fl, alpha, False), k7_prep.prepare(tl, alpha, True)
    for mode in MODES:
        truth = oracle_mod.fuzz_matrix(fl, tl, mode)
        floors = list(FLOORS) + np.unique(truth)[::12].tolist()
        for share in (0, 16 * W):
            for c in floors:
                score, ub = run_pairs(host, W, alpha, A, B, mode, np.full(len(fl), c), share)
                hit = truth >= c
                np.testing.assert_array_equal(score >= c, hit, err_msg=f"{mode} share {share} floor {c!r}")
                np.testing.assert_array_equal(score[hit], truth[hit], err_msg=f"{mode} share {share} floor {c!r}")
                assert (ub[hit] + np.float32(SLACK) >= np.float32(c)).all(), (mode, share, c)


@pytest.fixture(scope="module")
def k18():
    so = os.path.join(REPO, "oracle", "_build", "k18_core_host.so")
    src = [os.path.join(HERE, "k18_core_host.cpp"), os.path.join(REPO, "polyfuzz_amd", "csrc", "k18_core.h")]
    os.makedirs(os.path.dirname(so), exist_ok=True)
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", src[0], "-o", so])
    lib = ctypes.CDLL(so)
    lib.k18_host_pack.restype, lib.k18_host_pack.argtypes = ctypes.c_uint64, [ctypes.c_int32, ctypes.c_int32]
    for f in (lib.k18_host_row, lib.k18_host_col):
        f.restype, f.argtypes = ctypes.c_int32, [ctypes.c_uint64]
    lib.k18_host_hit.restype, lib.k18_host_hit.argtypes = ctypes.c_int, [ctypes.c_double, ctypes.c_double]
    lib.k18_host_go.restype, lib.k18_host_go.argtypes = ctypes.c_int, [ctypes.c_float, ctypes.c_double]
    lib.k18_host_slack.restype = ctypes.c_float
    lib.k18_host_max_capacity.restype = ctypes.c_int64
    return lib


def test_k18_core_key_hit_and_prune_rules(k18, oracle_mod):
    edge = (0, 1, 2 ** 26 - 1)
    for r in edge:
        for c in edge:
            key = k18.k18_host_pack(r, c)
            assert key == r << 32 | c and k18.k18_host_row(key) == r and k18.k18_host_col(key) == c
    assert k18.k18_host_pack(0, 2 ** 26 - 1) < k18.k18_host_pack(1, 0)          # keys sort by (row, to-index)
    assert k18.k18_host_slack() == np.float32(SLACK) and k18.k18_host_max_capacity() == 2 ** 32 - 1
    # attained scores: the published 85.5, and one that is no short decimal
    s2 = float(oracle_mod.fuzz_matrix(["this is a word"], ["THIS IS A WORD"], "WRatio")[0, 0])
    assert abs(s2 - 21.42857142857143) < 1e-12
    for s in (85.5, s2):
        below, above = math.nextafter(s, -math.inf), math.nextafter(s, math.inf)
        assert [k18.k18_host_hit(s, c) for c in (0.0, below, s, above, 100.0)] == [1, 1, 1, 0, 0]
        # the prune rule is the kernel's float32 comparison, and a bound that holds (>= the score, as float32) keeps every hit
        for c in (0.0, below, s, above, 100.0):
            for ub in (np.float32(s), np.float32(s - 1.0), np.float32(0.0), np.float32(100.0)):
                want = not (np.float32(ub + np.float32(SLACK)) < np.float32(c))
                assert k18.k18_host_go(ub, c) == int(want), (s, c, ub)
        assert all(k18.k18_host_go(np.float32(s), c) for c in (0.0, below, s))
        assert not k18.k18_host_go(np.float32(s - 1.0), s)
    assert k18.k18_host_hit(100.0, 100.0) == 1 and k18.k18_host_hit(0.0, 0.0) == 1
    assert k18.k18_host_hit(28.999999999999996, 0.29 * 100) == 1 and k18.k18_host_hit(28.999999999999993, 0.29 * 100) == 0


def test_k18_core_stand_alone_program(tmp_path):
    """the same header as a program of its own (-DK18_HOST_MAIN): what a sanitizer run of K18 builds, with
    -fsanitize=address,undefined added -- k18_core.h is all of K18 that runs on a host"""
    exe = str(tmp_path / "k18_core_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-DK18_HOST_MAIN", os.path.join(HERE, "k18_core_host.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "0 violations" in out.stdout, out.stdout + out.stderr


# ---- _lib.fuzz_join / fuzz_components against a fake library -------------------------------------------------------------------

DTYPES = (np.int32, np.float64)


def _fuzz_join(totals, **kw):
    lib = FakeLib(len(DTYPES), DTYPES, totals)
    out = _lib.fuzz_join(SimpleNamespace(lib=lib, h=object()), _strings(), None, "token_ratio", 0.29 * 100, **kw)
    assert all(c.name == "pfz_fuzz_join" for c in lib.calls)
    return lib, out


def _check(lib, out, total, n_out=3):
    assert len(out) == n_out
    row_ptr, idx, score = out[:3]
    assert row_ptr.dtype == np.int64 and row_ptr.shape == (N_FROM + 1,) and row_ptr[-1] == total
    for a, dt, address in zip((idx, score), DTYPES, lib.calls[-1].hit_addresses):
        assert a.dtype == dt and a.shape == (total,) and a.flags.owndata
        np.testing.assert_array_equal(a, np.arange(total).astype(dt))
        assert total == 0 or not address <= a.ctypes.data < address + max(lib.calls[-1].cap, 1) * a.itemsize
    # (ctx handle, from handle, to handle (NULL: the self-join), scorer id, cutoff) -- the cutoff as it was computed
    head = lib.calls[-1].head
    assert head[2] is None and head[3] == _lib.FUZZ_SCORERS["token_ratio"] == 3 and head[4] == 28.999999999999996


@pytest.mark.parametrize("capacity,total", ((8, 5), (8, 8), (8, 0), (0, 0), (None, 4095), (None, 4096)))
def test_fuzz_join_one_call_while_the_total_fits(capacity, total):
    lib, out = _fuzz_join([total], capacity=capacity)
    assert [c.cap for c in lib.calls] == [max(4096, 4 * N_FROM) if capacity is None else capacity]
    _check(lib, out, total)


@pytest.mark.parametrize("capacity,total", ((8, 9), (0, 3), (None, 4097)))
def test_fuzz_join_one_repeat_with_room_for_the_exact_total(capacity, total):
    lib, out = _fuzz_join([total, total], capacity=capacity)
    assert [c.cap for c in lib.calls] == [max(4096, 4 * N_FROM) if capacity is None else capacity, total]
    assert lib.calls[0].head == lib.calls[1].head
    _check(lib, out, total)


def test_fuzz_join_a_second_overflow_raises_and_counters_are_the_last_calls():
    lib = FakeLib(len(DTYPES), DTYPES, [9, 10, 10])
    with pytest.raises(AssertionError):
        _lib.fuzz_join(SimpleNamespace(lib=lib, h=object()), _strings(), _strings(), "WRatio", 90.0, capacity=8)
    assert [c.cap for c in lib.calls] == [8, 9]                            # never a third call
    assert _lib.FUZZ_JOIN_COUNTERS == ("bounded", "scored", "steps")
    lib, out = _fuzz_join([9, 9], capacity=8, counters=True)
    assert len(lib.calls) == 2
    _check(lib, out, 9, n_out=4)
    assert out[3] == {"bounded": 10, "scored": 11, "steps": 12} and list(out[3]) == list(_lib.FUZZ_JOIN_COUNTERS)


def test_fuzz_components_wrapper():
    calls = []

    def entry(*args):
        calls.append(args)
        label, pairs, components, work = args[-4:]
        (ctypes.c_int32 * N_FROM).from_address(label.value)[:] = [0, 0, 2, 0, 4, 4, 6]
        pairs._obj.value, components._obj.value = 3, 4
        if work is not None:
            (ctypes.c_int64 * 3).from_address(work.value)[:] = [5, 6, 7]
        return 0
    ctx = SimpleNamespace(lib=SimpleNamespace(pfz_fuzz_components=entry), h=object())
    label, pairs, components = _lib.fuzz_components(ctx, _strings(), "partial_ratio", 85.5)
    assert label.dtype == np.int32 and label.tolist() == [0, 0, 2, 0, 4, 4, 6] and (pairs, components) == (3, 4)
    assert calls[0][2:4] == (_lib.FUZZ_SCORERS["partial_ratio"], 85.5)
    out = _lib.fuzz_components(ctx, _strings(), "WRatio", 90.0, counters=True)
    assert out[3] == {"bounded": 5, "scored": 6, "steps": 7}


def test_ctypes_table_has_the_two_entries():
    assert len(_lib.SIGNATURES["pfz_fuzz_join"][1]) == 11 and len(_lib.SIGNATURES["pfz_fuzz_components"][1]) == 8
    header = open(os.path.join(REPO, "include", "polyfuzz_hip.h")).read()
    assert "int pfz_fuzz_join(" in header and "int pfz_fuzz_components(" in header and "_rapidfuzz.py:99-113" in header


# ---- the matcher's surface, the device unreachable ----------------------------------------------------------------------------

@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a device call before the arguments were checked")
    monkeypatch.setattr(_lib.Context, "default", staticmethod(refuse))


BAD = [float("nan"), float("inf"), -float("inf"), -0.1, -1, 1.0000001, 2, "0.8", None, True, False, [0.8], (0.8,), np.array([0.8])]


@pytest.mark.parametrize("bad", BAD, ids=[repr(b) for b in BAD])
def test_bad_min_similarity_raises_before_any_device_call(no_device, bad):
    from polyfuzz_amd.models import RapidFuzz
    m = RapidFuzz()
    with pytest.raises(ValueError, match="min_similarity"):
        m.join(["a b", "b a"], ["a"], bad)
    with pytest.raises(ValueError, match="min_similarity"):
        m.join(["a b", "b a"], min_similarity=bad)
    with pytest.raises(ValueError, match="min_similarity"):
        m.components(["a b", "b a"], bad)


@pytest.mark.parametrize("scorer", ["ratio", "QRatio", "token_sort_ratio"])
def test_k4_scorers_have_no_threshold_form(no_device, scorer):
    from polyfuzz_amd.models import RapidFuzz
    m = RapidFuzz(scorer=scorer)
    for call in (lambda: m.join(["a"], ["a"], 0.9), lambda: m.join(["a", "a"]), lambda: m.components(["a", "a"], 0.9)):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert not isinstance(e.value, _lib.PfzError)
        assert all(name in str(e.value) for name in _lib.FUZZ_SCORERS) and "indel" in str(e.value) and scorer in str(e.value)


def test_empty_lists_need_no_device(no_device):
    from polyfuzz_amd.models import RapidFuzz
    m = RapidFuzz()
    for df in (m.join([], ["a"]), m.join(["a"], []), m.join([]), m.join([], [], 0.0)):
        assert list(df.columns) == ["From", "To", "Similarity"] and len(df) == 0 and df["Similarity"].dtype == np.float64
    label = m.components([], 0.9)
    assert label.dtype == np.int32 and label.shape == (0,)


def test_pickle_round_trip_and_documents(no_device):
    from polyfuzz_amd import linkage
    from polyfuzz_amd.models import RapidFuzz
    m = RapidFuzz(scorer="token_set_ratio", score_cutoff=0.4)
    m._to_dev, m._to_names = object(), ("a",)                     # (device handles stay behind)
    m2 = pickle.loads(pickle.dumps(m))
    assert m2._scorer_name == "token_set_ratio" and m2.score_cutoff == 40 and m2._to_dev is None and m2._to_names is None
    assert len(m2.join([], ["a"])) == 0
    assert "join" in RapidFuzz.__doc__ and "components" in RapidFuzz.__doc__
    for doc in (RapidFuzz.join.__doc__, RapidFuzz.components.__doc__):
        assert "85.5" in doc and "0.855" in doc and "token" in doc and "earlier position" in doc.lower()
    assert 'WRatio("", "")' in RapidFuzz.join.__doc__
    assert "RapidFuzz" in linkage.connected_components.__doc__ and "K18" in linkage.connected_components.__doc__
