"""K16 (pfz_pairs_join / pfz_pairs_components, BlockedEditDistance.join / .components) without a GPU: the entry points in header,
library and ctypes table, the header's contract, the refusals before any device call, the matcher's signature, the test helpers
held to a hand-worked case, the symmetry of the scorers' definitions on the test lists, and polyfuzz_amd/csrc/k16_core.h -- key
packing, the sentinel's order, the unique rule, the row pointers -- compiled for the host as a stand-alone program
(tests/k16_core_host.cpp) and run, once plain and once under the host's address and undefined-behaviour sanitizers."""
import ctypes
import inspect
import math
import os
import subprocess

import numpy as np
import pytest

from tests import pairs_join_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def _no_device(*a, **k):
    raise AssertionError("the device was reached")


def _header():
    return open(os.path.join(REPO, "include", "polyfuzz_hip.h")).read()


def _arg_names(header, name):
    decl = header[header.index(f"int {name}("):]
    decl = decl[:decl.index(";")]
    return [a.strip().split()[-1].lstrip("*") for a in decl[decl.index("(") + 1:decl.rindex(")")].split(",")]


def test_entry_points_in_header_library_and_table():
    from polyfuzz_amd import _build, _lib
    if _build.is_stale():
        _build.build()
    header = _header()
    so = ctypes.CDLL(_lib.lib_path())
    for name in ("pfz_pairs_join", "pfz_pairs_components"):
        assert f"int {name}(" in header and hasattr(so, name) and name in _lib.SIGNATURES
    assert _arg_names(header, "pfz_pairs_join") == ["ctx", "from_strings", "to_strings", "candidates", "scorer", "min_similarity", "capacity",
                                                    "out_row_ptr", "out_idx", "out_sim", "out_total", "out_counters"]
    assert _arg_names(header, "pfz_pairs_components") == ["ctx", "strings", "candidates", "scorer", "min_similarity", "out_label",
                                                          "out_pairs", "out_components", "out_counters"]
    restype, argtypes = _lib.SIGNATURES["pfz_pairs_join"]
    assert restype is ctypes.c_int and len(argtypes) == 12 and argtypes[4] is ctypes.c_int32 and argtypes[5] is ctypes.c_double \
        and argtypes[6] is ctypes.c_int64
    restype, argtypes = _lib.SIGNATURES["pfz_pairs_components"]
    assert restype is ctypes.c_int and len(argtypes) == 9 and argtypes[3] is ctypes.c_int32 and argtypes[4] is ctypes.c_double
    assert _lib.PAIR_JOIN_SCORERS == {"levenshtein": 1, "osa": 2, "jaro": 3, "jaro_winkler": 4}
    assert all(_lib.PAIR_SCORERS[k] == v for k, v in _lib.PAIR_JOIN_SCORERS.items()) and "ratio" not in _lib.PAIR_JOIN_SCORERS
    assert _lib.PAIR_JOIN_COUNTERS == ("candidates", "scored", "pairs")
    for f, names in ((_lib.pairs_join, ["ctx", "from_dev", "to_dev", "candidates", "scorer", "min_similarity", "capacity", "counters"]),
                     (_lib.pairs_components, ["ctx", "dev", "candidates", "scorer", "min_similarity", "counters"])):
        assert list(inspect.signature(f).parameters) == names
    p = inspect.signature(_lib.pairs_join).parameters
    assert p["capacity"].default is None and p["counters"].default is False


def test_header_states_the_semantics_the_capacity_rule_and_the_limits():
    header = _header()
    doc = header[header.index("---- K16"):header.index("int pfz_pairs_join(")]
    doc = " ".join(doc.replace("\n * ", "\n").split())
    for phrase in ("*out_total is always the exact number of hits", "returns PFZ_OK, has written NONE of the three output arrays",
                   "repeated with capacity >= *out_total", "never writes a hit past the capacity", "ascending within a row",
                   "equal inputs give equal bytes", "an index that occurs twice in a row counts once", "SYMMETRISED",
                   "the lower position is the from-string", "A row's own index in its row is skipped",
                   "equal strings at different positions are a pair", "equal is kept", "bit for bit", "PFZ_PAIR_RATIO (0) is refused",
                   "0 .. 100", "more than 1024 candidates per row", "a list of 2^31 strings or more", "2^31 table cells",
                   "PFZ_ERR_UNSUPPORTED", "PFZ_ERR_INVALID", "no window, no abandon rule, no bound", "int64[3]", "8 B per table cell",
                   "SMALLEST position", "no launch", "fewer candidate rows than from-strings"):
        assert phrase in doc, phrase
    prof = header[header.index("int pfz_prof_enable("):header.index("int pfz_prof_get(")]
    assert all(scope in prof for scope in ("`k16_pairs_join`", "`k16_pairs_join_general`"))


RATIO_LIKE = ("ratio", None, "default")      # (None: the reference's default scorer; "default": the default-constructed matcher)


def _matcher(scorer):
    from polyfuzz_amd.models import BlockedEditDistance
    if scorer == "default":
        return BlockedEditDistance()
    if scorer == "fuzz.ratio":          # a callable that names rapidfuzz.fuzz.ratio, as EditDistance resolves callables
        def ratio(a, b):
            raise AssertionError("the scorer is never called on the host")
        ratio.__module__ = "rapidfuzz.fuzz"
        return BlockedEditDistance(scorer=ratio)
    return BlockedEditDistance(scorer=scorer)


@pytest.mark.parametrize("scorer", RATIO_LIKE + ("fuzz.ratio",))
def test_ratio_has_no_threshold_form_and_says_so_before_any_device_call(scorer, monkeypatch):
    from polyfuzz_amd import _lib, linkage
    monkeypatch.setattr(_lib.Context, "default", classmethod(_no_device))
    m = _matcher(scorer)
    assert m._scorer_name == "ratio"
    names = ["apple inc", "apple incorporated", "pear ltd"]
    calls = (lambda: m.join(names, names, 0.5), lambda: m.join(names), lambda: m.join(names, None, 0.9, re_train=False),
             lambda: m.components(names, 0.5), lambda: linkage.connected_components(names, m, 0.5),
             lambda: m.join(names, names, float("nan")))          # (the scorer is refused first)
    for call in calls:
        with pytest.raises(NotImplementedError) as e:
            call()
        assert not isinstance(e.value, _lib.PfzError)
        for name in C.FOUR:
            assert name in str(e.value)


@pytest.mark.parametrize("scorer", C.FOUR)
def test_min_similarity_must_be_a_number_in_0_1(scorer, monkeypatch):
    from polyfuzz_amd import _lib, linkage
    from polyfuzz_amd.models import BlockedEditDistance
    monkeypatch.setattr(_lib.Context, "default", classmethod(_no_device))
    names = ["apple inc", "apple incorporated", "pear ltd"]
    m = BlockedEditDistance(scorer=scorer)
    for bad in (float("nan"), float("inf"), -float("inf"), -1e-300, np.nextafter(1.0, 2.0), 1.5, -0.1, "0.8", None, True, [0.8]):
        with pytest.raises(ValueError, match="min_similarity"):
            m.join(names, names, bad)
        with pytest.raises(ValueError, match="min_similarity"):
            m.join(names, min_similarity=bad)
        with pytest.raises(ValueError, match="min_similarity"):
            m.join(names, None, bad, re_train=False)
        with pytest.raises(ValueError, match="min_similarity"):
            m.components(names, bad)
        with pytest.raises(ValueError, match="min_similarity"):
            linkage.connected_components(names, m, bad)
        with pytest.raises(ValueError, match="min_similarity"):      # the binding refuses too, without a library call
            _lib.pairs_join(None, None, None, None, scorer, bad)
        with pytest.raises(ValueError, match="min_similarity"):
            _lib.pairs_components(None, None, None, scorer, bad)
    for good in (0, 1, 0.0, 1.0, 0.8, np.float64(0.5), np.float32(0.25), np.int64(1)):      # accepted: the device is what stops these
        with pytest.raises(AssertionError, match="the device was reached"):
            m.join(names, names, good)
        with pytest.raises(AssertionError, match="the device was reached"):
            m.join(names, min_similarity=good)
        with pytest.raises(AssertionError, match="the device was reached"):
            m.components(names, good)
    assert m.last_counts is None and m.last_timings is None


def test_signatures_and_docstrings():
    from polyfuzz_amd import linkage
    from polyfuzz_amd.models import BlockedEditDistance
    assert list(inspect.signature(BlockedEditDistance.join).parameters) == ["self", "from_list", "to_list", "min_similarity", "re_train"]
    p = inspect.signature(BlockedEditDistance.join).parameters
    assert p["to_list"].default is None and p["min_similarity"].default == 0.8 and p["re_train"].default is True
    assert list(inspect.signature(BlockedEditDistance.components).parameters) == ["self", "from_list", "min_similarity"]
    assert inspect.signature(BlockedEditDistance.components).parameters["min_similarity"].default == 0.8
    assert "NOT applied" in BlockedEditDistance.join.__doc__ and "normalize" in BlockedEditDistance.components.__doc__
    for word in ("SYMMETRISED", "own index", "ratio", "join(", "components("):
        assert word in BlockedEditDistance.__doc__, word
    assert "BlockedEditDistance" in linkage.connected_components.__doc__


def test_pickling_is_unchanged():
    import pickle
    from polyfuzz_amd.models import BlockedEditDistance
    m = BlockedEditDistance(scorer="jaro_winkler", candidates=8)
    m._to_dev, m._to_names = object(), ("a",)
    state = m.__getstate__()
    assert "_to_dev" not in state and "_to_names" not in state and "last_counts" not in state
    m._to_dev = m._to_names = None
    back = pickle.loads(pickle.dumps(m))
    assert back._scorer_name == "jaro_winkler" and back.candidates == 8 and back._to_dev is None and back.last_counts is None


# ---- the helpers' own check ------------------------------------------------------------------------------------------------------

def test_helpers_on_a_hand_worked_case():
    """six strings; sim[i, j] = 1 - |i - j| / 10 above the diagonal and a value of its own below it, so that a look-up at [max, min]
    would show"""
    n = 6
    sim = np.array([[1.0 - abs(i - j) / 10.0 if j >= i else 0.01 * (i * n + j) for j in range(n)] for i in range(n)])
    tab = np.array([[1, 1, -1],        # (0, 1) twice: counts once
                    [0, 5, 6],         # 0: the other direction of (0, 1); (1, 5); 6 is outside
                    [2, -7, 2],        # the row's own index, twice: no pair
                    [-1, -1, -1],      # nothing
                    [2, 3, 0],         # listed only in the higher row: (2, 4), (3, 4), (0, 4)
                    [4, 1, 4]], np.int32)      # (4, 5) twice, (1, 5) again
    i, j, cells = C.candidate_pairs(tab, n, True)
    assert list(zip(i.tolist(), j.tolist())) == [(0, 1), (0, 4), (1, 5), (2, 4), (3, 4), (4, 5)] and cells == 10
    row_ptr, idx, s, counts = C.expected_join(sim, tab, 0.8, True)
    assert row_ptr.tolist() == [0, 1, 1, 2, 3, 4, 4] and idx.tolist() == [1, 4, 4, 5] and s.tolist() == [0.9, 0.8, 0.9, 0.9]      # equal is kept
    assert counts == {"candidates": 10, "scored": 6, "pairs": 4} and idx.dtype == np.int32 and row_ptr.dtype == np.int64
    assert C.expected_labels(n, row_ptr, idx).tolist() == [0, 0, 2, 2, 2, 2]
    assert C.expected_join(sim, tab, np.nextafter(0.8, 1.0), True)[1].tolist() == [1, 4, 5]
    # two lists: the same table against a to-list of 6 -- no folding, the own index is a pair like any other
    i, j, cells = C.candidate_pairs(tab, n, False)
    assert list(zip(i.tolist(), j.tolist())) == [(0, 1), (1, 0), (1, 5), (2, 2), (4, 0), (4, 2), (4, 3), (5, 1), (5, 4)] and cells == 12
    row_ptr, idx, s, counts = C.expected_join(sim, tab, 0.0, False)
    assert row_ptr.tolist() == [0, 1, 3, 4, 4, 7, 9] and s[1] == sim[1, 0] != sim[0, 1]
    assert counts == {"candidates": 12, "scored": 9, "pairs": 9}
    assert C.expected_labels(4, np.array([0, 0, 0, 0, 0]), np.zeros(0, np.int32)).tolist() == [0, 1, 2, 3]
    frame = C.frame_of(list("abcdef"), list("abcdef"), *C.expected_join(sim, tab, 0.8, True)[:3])
    assert frame["From"].tolist() == ["a", "c", "d", "e"] and frame["To"].tolist() == ["b", "e", "e", "f"]


def test_the_definitions_are_symmetric_on_the_test_lists():
    """score(a, b) == score(b, a), bit for bit, under all four scorers on the self-join lists: a mismatch on the GPU is then the
    kernel's, not the definition's"""
    for strings, sims in (C.self_list()[:2], C.hub("first", 20)[:2]):
        for name in C.FOUR:
            np.testing.assert_array_equal(sims[name], sims[name].T, err_msg=name)


# ---- k16_core.h on the host ------------------------------------------------------------------------------------------------------

def _host_program(tag, flags):
    exe = os.path.join(REPO, "oracle", "_build", f"k16_core_host_{tag}")
    csrc = os.path.join(REPO, "polyfuzz_amd", "csrc")
    src = [os.path.join(HERE, "k16_core_host.cpp"), os.path.join(HERE, "rows_fill_host.h")] + [os.path.join(csrc, h) for h in (
        "k16_core.h", "k11_core.h", "k9_core.h")]
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + [src[0], "-o", exe])
    return exe


def _run_host_program(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    words = out.stdout.split()
    assert words[:2] == ["k16_core_host", "ok"] and int(words[2]) == 240 and int(words[3]) > 1000, out.stdout
    # the shared row-pointer fill: every ascending sequence of 1 .. 5 rows over 0 .. 4 rows (and the row behind the last), both widths
    assert int(words[4]) == 2 * sum(math.comb(n_rows + total, total) for n_rows in range(5) for total in range(1, 6)), out.stdout


def test_keys_sentinel_unique_rule_and_row_pointers_on_the_host():
    _run_host_program(_host_program("plain", ["-O2"]))


def test_the_same_program_under_the_host_sanitizers():
    try:
        exe = _host_program("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    except subprocess.CalledProcessError:
        pytest.skip("this g++ cannot link -fsanitize=address,undefined")
    _run_host_program(exe)


def test_kernel_budget():
    """K16's kernels: no scratch anywhere (Jaro's flag words stay in registers), the register kernels' static LDS no larger than
    K10's (the match table is dynamic), and every instance the host dispatches is there: 2 word widths x 3 families x 2 sinks, and
    the general kernel once per sink"""
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_budget
    from polyfuzz_amd import _build
    for exe in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(kernel_budget.LLVM, exe)):
            pytest.skip(f"{exe} not in {kernel_budget.LLVM}")
    md = kernel_budget.kernel_metadata(_build.build())
    pretty = dict(zip(md, kernel_budget.demangled(list(md))))
    k10_lds = max(v["lds"] for k, v in md.items() if "k10_pairs_kernel" in pretty[k])
    k16 = {pretty[k]: v for k, v in md.items() if "k16_" in pretty[k]}
    reg = {n: v for n, v in k16.items() if "k16_pairs_kernel" in n}
    assert len(reg) == 12 and sum("k16_pairs_general_kernel" in n for n in k16) == 2, sorted(k16)
    assert all(any(f"k16_{name}" in n for n in k16) for name in ("keys", "rows", "compact"))
    for name, k in k16.items():
        assert k["scratch"] == 0, (name, k)
    for name, k in reg.items():
        assert k["lds"] <= k10_lds, (name, k)
