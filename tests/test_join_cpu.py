"""K11 (EditDistance.join: all pairs at or above a Levenshtein / OSA similarity) without a GPU: what the threshold lets a lane leave
out (polyfuzz_amd/csrc/k11_core.h, compiled for the host by tests/k11_core_host.cpp) held to the definition exhaustively -- the
integer cutoff kmax against the float64 formula, the walk's lower bound against the final distance, no hit lost to the window or
to the abandon rule, in one- and multi-word form, under both scorers --, the packed hit, the scorer gate and the argument checks of
EditDistance.join, the entry point in header / library / ctypes table, the kernels' register and LDS budget, and the title-width
fixture (tests/golden/c3_lev_join_oracle.npz) against the oracle it was made from."""
import ctypes
import importlib.util
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import lev_oracle

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

# the issue's thresholds and their float64 neighbours (inside [0, 1])
BASE = (0.0, 0.25, 1.0 / 3.0, 0.5, 2.0 / 3.0, 0.8, 1.0)
THRESHOLDS = np.array(sorted({v for t in BASE for v in (np.nextafter(t, -1.0), t, np.nextafter(t, 2.0)) if 0.0 <= v <= 1.0}))
MAX_LEN = 6


@pytest.fixture(scope="module")
def host():
    so = os.path.join(REPO, "oracle", "_build", "k11_core_host.so")
    csrc = os.path.join(REPO, "polyfuzz_amd", "csrc")
    src = [os.path.join(HERE, "k11_core_host.cpp"), os.path.join(HERE, "rows_fill_host.h"), os.path.join(csrc, "k11_core.h"),
           os.path.join(csrc, "k9_core.h")]
    os.makedirs(os.path.dirname(so), exist_ok=True)
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", src[0], "-o", so])
    lib = ctypes.CDLL(so)
    lib.k11_host_exhaustive.restype = lib.k11_host_long.restype = ctypes.c_int
    lib.k11_host_kmax.restype = ctypes.c_int32
    lib.k11_host_kmax.argtypes = [ctypes.c_double, ctypes.c_int32, ctypes.c_int32]
    return lib


def _all_strings(max_len):
    """the host program's order: by length, then the binary number with 'b' = 1, first character lowest"""
    return ["".join("b" if bits >> p & 1 else "a" for p in range(n)) for n in range(max_len + 1) for bits in range(1 << n)]


def _p(x):
    return x.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("osa", (0, 1), ids=lev_oracle.SCORERS)
@pytest.mark.parametrize("word_bits", (32, 64, 0), ids=("word32", "word64", "multiword"))
def test_threshold_logic_exhaustively(host, word_bits, osa):
    """every pair of strings over {a, b} of up to 6 characters (127 x 127), every threshold of THRESHOLDS: kmax agrees with the
    formula at every d, dist_j - (lb - j) never exceeds the final distance (the horizontal deltas stay within +-1, under OSA
    too), no hit is outside the window or abandoned -- and the abandon rule does fire, on misses; the distances are the oracle's.
    Then seeded pairs with from-strings of 31 .. 130 characters, edited copies among them: the same, across the word borders."""
    strings = _all_strings(MAX_LEN)
    n = len(strings)
    assert n == 127
    report = np.zeros(7, np.int64)
    d = np.empty((n, n), np.int32)
    assert host.k11_host_exhaustive(word_bits, osa, MAX_LEN, ctypes.c_int64(len(THRESHOLDS)), _p(THRESHOLDS), _p(report), _p(d)) == 0
    assert report[0] == n * n and report[1:5].tolist() == [0, 0, 0, 0] and report[6] == 0, report.tolist()
    assert report[5] > 10_000                                  # (pair, threshold) combinations the rule abandoned
    np.testing.assert_array_equal(d, lev_oracle.matrix(strings, strings, lev_oracle.SCORERS[osa]))
    long_report = np.zeros(7, np.int64)
    assert host.k11_host_long(word_bits, osa, ctypes.c_int64(600), ctypes.c_int64(len(THRESHOLDS)), _p(THRESHOLDS), _p(long_report)) == 0
    assert long_report[0] >= {32: 100, 64: 250, 0: 600}[word_bits]      # (2, 5 and 10 of the 10 border lengths fit the word)
    assert long_report[1:5].tolist() == [0, 0, 0, 0] and long_report[6] == 0, long_report.tolist()
    assert long_report[5] > 0, long_report.tolist()            # (the rule is at work here too)


def test_kmax_is_the_formula_not_the_floor(host):
    """kmax(t, la, lb) == #{d in 0 .. M : 1 - d / M >= t} - 1 in numpy's float64 for every M <= 300 and threshold; it depends on
    the lengths through M alone (the kernels' table); and floor((1 - t) * M) alone is NOT it: at t = 0.8, M = 5, d = 1 scores
    exactly 0.8 and is a hit, while (1 - 0.8) * 5 < 1"""
    differs = 0
    for t in THRESHOLDS.tolist() + [0.9, 0.6, 0.1, 0.7]:
        for m in range(0, 301):
            want = int((lev_oracle.similarity(np.arange(m + 1), m, m) >= t).sum()) - 1
            got = {host.k11_host_kmax(t, m, other) for other in {0, m // 2, m}} | {host.k11_host_kmax(t, m // 3, m)}
            assert got == {want}, (t, m, got, want)
            differs += want != int(np.floor((1.0 - t) * m))
    assert host.k11_host_kmax(0.8, 5, 5) == 1 and int(np.floor((1.0 - 0.8) * 5)) == 0 and differs > 20
    assert host.k11_host_kmax(1.0, 0, 0) == 0 and host.k11_host_kmax(np.nextafter(1.0, 0.0), 7, 3) == 0
    assert host.k11_host_kmax(0.0, 9, 4) == 9


def test_row_pointer_fill_exhaustively(host):
    """rows_fill (k11_core.h), which every join's unpack and K16's segments share: for every ascending sequence of 1 .. 5 hit rows
    over 0 .. 4 rows -- rows without a hit in front, in the middle and at the end, and K16's row behind the last -- and both
    pointer widths, every row pointer is written exactly once and equals the hits counted in the rows before it"""
    cases = ctypes.c_int64(0)
    assert host.k11_host_rows_fill(ctypes.byref(cases)) == 0
    assert cases.value == 2 * sum(math.comb(n_rows + total, total) for n_rows in range(5) for total in range(1, 6))


def test_packed_hit_round_trip(host):
    out = np.empty(3, np.int32)
    for row, to, d in ((0, 0, 0), ((1 << 24) - 1, (1 << 24) - 1, 65535), (5, (1 << 24) - 1, 0), ((1 << 24) - 1, 0, 1), (123456, 654321, 4321)):
        host.k11_host_unpack(row, to, d, _p(out))
        assert out.tolist() == [row, to, d]
    header = open(os.path.join(REPO, "include", "polyfuzz_hip.h")).read()
    k11 = header[header.index("K11: all pairs"):header.index("int pfz_lev_join(")]
    assert "2^24" in k11 and "65 535" in k11 and "PFZ_ERR_UNSUPPORTED" in k11        # the limits the packing implies, stated


def _no_device(*a, **k):
    raise AssertionError("the device was reached")


@pytest.mark.parametrize("scorer", ["ratio", "QRatio", "jaro", "jaro_winkler", "WRatio", "token_set_ratio"])
def test_scorers_without_a_join_raise_before_any_device_call(scorer, monkeypatch):
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import EditDistance
    monkeypatch.setattr(_lib.Context, "default", classmethod(_no_device))
    with pytest.raises(NotImplementedError) as e:
        EditDistance(scorer=scorer).join(["a", "b"], ["a", "c", "d"], 0.5)
    assert not isinstance(e.value, _lib.PfzError)
    for name in ("levenshtein", "osa"):
        assert name in str(e.value)


@pytest.mark.parametrize("scorer", lev_oracle.SCORERS)
def test_min_similarity_must_be_a_number_in_0_1(scorer, monkeypatch):
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import EditDistance
    monkeypatch.setattr(_lib.Context, "default", classmethod(_no_device))
    m = EditDistance(scorer=scorer)
    for bad in (float("nan"), float("inf"), -float("inf"), -1e-300, np.nextafter(1.0, 2.0), 1.5, -0.1, "0.8", None, True, [0.8]):
        with pytest.raises(ValueError):
            m.join(["a", "b"], ["a"], bad)
        with pytest.raises(ValueError):
            m.join(["a", "b"], min_similarity=bad)
    for good in (0, 1, 0.0, 1.0, 0.8, np.float64(0.5), np.float32(0.25), np.int64(1)):      # accepted: the device is what stops these
        with pytest.raises(AssertionError, match="the device was reached"):
            m.join(["a", "b"], ["a"], good)
    assert "normalize" in EditDistance.join.__doc__ and "NOT applied" in EditDistance.join.__doc__


def test_entry_point_in_header_library_and_table():
    from polyfuzz_amd import _build, _lib
    if _build.is_stale():
        _build.build()
    header = open(os.path.join(REPO, "include", "polyfuzz_hip.h")).read()
    so = ctypes.CDLL(_lib.lib_path())
    assert "int pfz_lev_join(" in header and hasattr(so, "pfz_lev_join") and "pfz_lev_join" in _lib.SIGNATURES
    decl = header[header.index("int pfz_lev_join("):]
    decl = decl[:decl.index(";")]
    assert [a.strip().split()[-1].lstrip("*") for a in decl[decl.index("(") + 1:decl.rindex(")")].split(",")] == [
        "ctx", "from_strings", "to_strings", "scorer", "min_similarity", "capacity", "out_row_ptr", "out_idx", "out_dist", "out_sim",
        "out_total", "out_counters"]
    restype, argtypes = _lib.SIGNATURES["pfz_lev_join"]
    assert restype is ctypes.c_int and len(argtypes) == 12 and argtypes[4] is ctypes.c_double and argtypes[5] is ctypes.c_int64
    assert _lib.LEV_SCORERS == {"levenshtein": 0, "osa": 1} and callable(_lib.lev_join)
    assert _lib.LEV_JOIN_COUNTERS == ("pairs_in_window", "pairs_finished", "steps")


def test_no_device_no_fallback():
    import polyfuzz_amd
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import EditDistance
    if polyfuzz_amd.device_count() > 0:
        pytest.skip("a GPU is visible: the no-device failure path cannot be exercised")
    for name in lev_oracle.SCORERS:
        with pytest.raises(_lib.PfzNoDevice):
            EditDistance(scorer=name).join(["a"], ["b"], 0.5)


def test_kernel_budget():
    """the eight register-kernel instances (32- / 64-bit words x 8- / 16-bit symbols x Levenshtein / OSA) are held to K9's own
    limits: no scratch, static LDS no larger than K8's (the match table is dynamic), at most 64 registers -- eight waves per SIMD
    (measured: 39 .. 43 in 32-bit words, 45 .. 50 in 64-bit words; the threshold reaches them as a table of integer cutoffs, no
    lane divides); the general kernel, the cutoff table and the unpacking (edit_walk.h's, K11's instances) are held to no scratch.  No kernel of K11 carries one
    of the names tests/test_levenshtein_cpu.py counts K9's kernels by."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_budget
    from polyfuzz_amd import _build
    for exe in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(kernel_budget.LLVM, exe)):
            pytest.skip(f"{exe} not in {kernel_budget.LLVM}")
    md = kernel_budget.kernel_metadata(_build.build())
    pretty = dict(zip(md, kernel_budget.demangled(list(md))))
    k8_lds = max(v["lds"] for k, v in md.items() if "k8_jaro_kernel" in pretty[k])
    hits = {pretty[k].split("(")[0]: v for k, v in md.items() if "k11_join_kernel" in pretty[k]}
    assert sorted(hits) == sorted(f"void pfz::k11_join_kernel<unsigned {w}, {idb}, {osa}>" for w in ("int", "long") for idb in (8, 16)
                                  for osa in ("false", "true")), sorted(hits)
    for name, k in hits.items():
        assert k["scratch"] == 0 and k["lds"] <= k8_lds and k["lds"] % 16 == 0, (name, k)
        assert k["vgpr"] <= (56 if "unsigned int" in name else 64), (name, k)
    k11 = {pretty[k]: v for k, v in md.items() if "k11_" in pretty[k] or "walk_begin_kernel<pfz::KmaxByM>" in pretty[k]
           or "edit_unpack_kernel<pfz::LevScore>" in pretty[k]}
    assert len(k11) == 8 + 4 + 2 and sum("k11_join_general_kernel" in n for n in k11) == 4, sorted(k11)
    assert any("walk_begin_kernel<pfz::KmaxByM>" in n for n in k11) and any("edit_unpack_kernel<pfz::LevScore>" in n for n in k11)
    for name, k in k11.items():
        assert k["scratch"] == 0, (name, k)
        assert "k9_lev_kernel" not in name and "k9_lev_general_kernel" not in name


# ---- the title-width fixture ----

@pytest.fixture(scope="module")
def maker():
    spec = importlib.util.spec_from_file_location("make_golden_c3_lev_join", os.path.join(HERE, "golden", "make_golden_c3_lev_join.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_fixture_is_made_on_these_lists_and_rows(maker):
    fl, tl = maker.lists()
    assert os.path.getsize(maker.PATH) < (1 << 20)
    g = np.load(maker.PATH)
    assert str(g["lists_sha256"]) == maker.lists_sha256(fl, tl) and str(g["source"]) == "oracle"
    rows, floor = g["rows"], float(g["floor"])
    np.testing.assert_array_equal(rows, np.load(maker.ROWS_PATH)["rows"])
    assert rows.dtype == np.int32 and len(rows) == 2000 and maker.FLOOR <= floor <= 0.8
    la, lb = lev_oracle.lengths(fl)[rows], lev_oracle.lengths(tl)
    n = {}
    for scorer in lev_oracle.SCORERS:
        i, j, d = (g[f"{k}_{scorer}"] for k in ("from", "to", "distance"))
        assert i.dtype == j.dtype == d.dtype == np.int32 and len(i) == len(j) == len(d) > 1000
        assert ((i >= 0) & (i < 2000) & (j >= 0) & (j < 20_000)).all()
        key = i.astype(np.int64) * 20_000 + j
        assert (np.diff(key) > 0).all()                            # row-major, every pair once
        assert (d >= np.abs(la[i] - lb[j])).all() and (lev_oracle.similarity(d, la[i], lb[j]) >= floor).all()
        n[scorer] = set(key.tolist())
    assert n["levenshtein"] < n["osa"]                             # (OSA's d is no larger: its pairs include Levenshtein's)


@pytest.mark.parametrize("scorer", lev_oracle.SCORERS)
def test_a_seeded_sample_of_fixture_rows_recomputed_live(maker, scorer):
    """24 seeded fixture rows -- half of them rows WITH pairs, so that the sample is not mostly empty -- through the oracle against
    the whole to-list (4.8e5 pairs): the same pairs and distances"""
    fl, tl = maker.lists()
    g = np.load(maker.PATH)
    i, j, d = (g[f"{k}_{scorer}"] for k in ("from", "to", "distance"))
    rng = np.random.default_rng(20 + lev_oracle.SCORERS.index(scorer))
    pick = np.unique(np.concatenate([rng.choice(2000, 12, replace=False), rng.choice(np.unique(i), 12, replace=False)]))
    gi, gj, gd = maker.hits([fl[r] for r in g["rows"][pick]], tl, scorer, float(g["floor"]))
    keep = np.isin(i, pick)
    assert keep.sum() >= 12
    np.testing.assert_array_equal(pick[gi], i[keep], err_msg=scorer)
    np.testing.assert_array_equal(gj, j[keep], err_msg=scorer)
    np.testing.assert_array_equal(gd, d[keep], err_msg=scorer)
