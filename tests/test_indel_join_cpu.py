"""K13 (EditDistance(scorer="indel"): match, top_n, join, components under rapidfuzz.distance.Indel.normalized_similarity) without
a GPU: the oracle (tests/indel_oracle.py) pinned to oracle/indel.c; what the threshold lets a lane leave out
(polyfuzz_amd/csrc/k13_core.h on k10_core.h, compiled for the host by tests/k13_core_host.cpp) held to the definition -- the
integer cutoff lmin against the float64 formula, the window against the formula and as one interval around la, the walk's upper
bound against the final LCS in one- and multi-word form; that the 0..1 and the 0..100 formula order all pairs alike, and that the
host recovers the integer LCS from K4's ratio; the packed hit; the scorer's resolution, the argument checks of join / components
and the entry points in header / library / ctypes table."""
import ctypes
import functools
import os
import pickle
import subprocess

import numpy as np
import pytest

from tests import indel_oracle

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def host():
    so = os.path.join(REPO, "oracle", "_build", "k13_core_host.so")
    csrc = os.path.join(REPO, "polyfuzz_amd", "csrc")
    src = [os.path.join(HERE, "k13_core_host.cpp")] + [os.path.join(csrc, h) for h in ("k13_core.h", "k10_core.h", "k11_core.h", "k9_core.h")]
    os.makedirs(os.path.dirname(so), exist_ok=True)
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", src[0], "-o", so])
    lib = ctypes.CDLL(so)
    for f in ("k13_host_walk", "k13_host_lmin_check", "k13_host_window_check", "k13_host_order"):
        getattr(lib, f).restype = ctypes.c_int
    lib.k13_host_lmin.restype = ctypes.c_int32
    lib.k13_host_lmin.argtypes = [ctypes.c_double, ctypes.c_int32]
    lib.k13_host_similarity.restype = lib.k13_host_ratio.restype = ctypes.c_double
    lib.k13_host_similarity.argtypes = lib.k13_host_ratio.argtypes = [ctypes.c_int32] * 3
    return lib


def _p(x):
    return x.ctypes.data_as(ctypes.c_void_p)


@functools.lru_cache(None)
def _thresholds():
    """every value indel_similarity attains for S <= 60, each one's float64 neighbours, 0.0, 1.0 and 50 seeded doubles"""
    att = {float(v) for s in range(61) for v in indel_oracle.similarity(np.arange(s // 2 + 1), s, 0)}
    ts = att | {float(np.nextafter(v, 2.0)) for v in att} | {float(np.nextafter(v, -1.0)) for v in att} | {0.0, 1.0}
    ts |= set(np.random.default_rng(130).random(50).tolist())
    return np.array(sorted(t for t in ts if 0.0 <= t <= 1.0))


def _all_strings(max_len):
    """the host program's order: by length, then the binary number with 'b' = 1, first character lowest"""
    return ["".join("b" if bits >> p & 1 else "a" for p in range(n)) for n in range(max_len + 1) for bits in range(1 << n)]


def test_oracle_is_pinned_to_the_c_oracle():
    """(1 - d / S) * 100 of tests/indel_oracle.py == oracle/indel.c's ratio matrix, bit for bit, on ~300 mixed pairs with both-empty
    and one-empty pairs among them; the vectorised table == the plain one"""
    import oracle
    oracle.build_native()
    rng = np.random.default_rng(131)
    mk = lambda alpha, lo, hi: "".join(rng.choice(list(alpha), size=int(rng.integers(lo, hi + 1))))
    fl = ["", "a", "abab", "ababab"] + [mk("ab", 0, 12) for _ in range(5)] + [mk("abcdefgh ", 3, 80) for _ in range(5)] + \
        [mk("".join(chr(0x400 + k) for k in range(300)), 1, 40) for _ in range(3)]
    tl = ["", "b", "abab"] + [mk("ab", 0, 12) for _ in range(6)] + [mk("abcdefgh ", 3, 80) for _ in range(6)] + fl[-3:]
    assert len(fl) * len(tl) >= 300
    lcs = indel_oracle.lcs_matrix(fl, tl)
    assert all(lcs[i, j] == indel_oracle.lcs(a, b) for i, a in enumerate(fl) for j, b in enumerate(tl))
    la, lb = indel_oracle.lengths(fl)[:, None], indel_oracle.lengths(tl)[None, :]
    s = (la + lb).astype(np.float64)
    mine = np.where(s > 0, (1.0 - indel_oracle.distance(lcs, la, lb) / np.where(s > 0, s, 1.0)) * 100.0, 100.0)
    native = oracle.native.indel_argmax(fl, tl, want_matrix=True)[2]
    assert mine.tobytes() == native.tobytes()
    assert (indel_oracle.sim_matrix(fl, tl, lcs) * 100.0).tobytes() == native.tobytes()
    assert indel_oracle.similarity(0, 0, 0) == 1.0 and indel_oracle.similarity(0, 3, 0) == 0.0 and indel_oracle.similarity(4, 6, 4) == 0.8


def test_lmin_is_the_formula_not_the_ceiling(host):
    """for every S <= 600 and every threshold of _thresholds(): lcs >= lmin[S] <=> indel_similarity(lcs, S) >= t at every lcs in
    0 .. S / 2, and the similarity rises strictly with lcs; spot values in numpy's float64; ceil(t * S / 2) alone is NOT it"""
    ts = _thresholds()
    assert len(ts) > 1000
    report = np.zeros(3, np.int64)
    assert host.k13_host_lmin_check(ctypes.c_int64(len(ts)), _p(ts), 600, _p(report)) == 0
    assert report.tolist() == [601 * len(ts), 0, 0], report.tolist()
    differs = 0
    for t in ts[::37].tolist() + [0.8, 0.9, 0.6, 1.0, 0.0]:
        for s in (0, 1, 2, 5, 10, 59, 60, 333, 600):
            sim = indel_oracle.similarity(np.arange(s // 2 + 1), s, 0)
            want = int((sim < t).sum())
            assert host.k13_host_lmin(t, s) == want, (t, s)
            differs += want != int(np.ceil(t * s / 2))
    assert differs > 0
    assert host.k13_host_lmin(0.8, 10) == 4 and host.k13_host_lmin(float(np.nextafter(0.8, 2.0)), 10) == 5
    assert host.k13_host_lmin(1.0, 0) == 0 and host.k13_host_lmin(1.0, 7) == 4 and host.k13_host_lmin(0.0, 9) == 0
    for lcs, la, lb in ((0, 0, 0), (4, 6, 4), (0, 5, 0), (3, 3, 3), (7, 20, 9)):
        assert host.k13_host_similarity(lcs, la, lb) == float(indel_oracle.similarity(lcs, la, lb))


def test_window_is_the_formula_and_one_interval_around_la(host):
    """for every la, lb <= 300 and every threshold: min(la, lb) >= lmin[la + lb] <=> indel_similarity(min(la, lb), la, lb) >= t;
    for a fixed la the lb inside are one interval, and it contains la whenever it is not empty"""
    ts = _thresholds()
    report = np.zeros(5, np.int64)
    assert host.k13_host_window_check(ctypes.c_int64(len(ts)), _p(ts), 300, _p(report)) == 0
    assert report[0] == len(ts) * 301 * 301 and report[1:4].tolist() == [0, 0, 0], report.tolist()
    assert report[4] > len(ts) * 100          # (the window does leave lengths out)


@pytest.mark.parametrize("word_bits,pad_to", [(32, 0), (64, 0), (0, 0), (64, 64), (0, 64), (0, 65), (0, 130)],
                         ids=("word32", "word64", "multiword", "word64-pad64", "multiword-pad64", "multiword-pad65", "multiword-pad130"))
def test_walk_reaches_the_lcs_and_abandon_never_kills_a_hit(host, word_bits, pad_to):
    """every pair of strings over {a, b} of 0 .. 7 characters (255 x 255): the recurrence reaches the table's LCS, and after every
    prefix j, l_j + (lb - j) >= lcs -- indel_abandon can fire only on a pair whose lcs is below lmin.  Padded in front with a third
    character to 64, 65 and 130 from-characters the two strings' bits straddle a word border: the carry crosses it."""
    strings = _all_strings(7)
    n = len(strings)
    assert n == 255
    report = np.zeros(4, np.int64)
    lcs = np.empty((n, n), np.int32)
    assert host.k13_host_walk(word_bits, 7, pad_to, _p(report), _p(lcs)) == 0
    assert report.tolist() == [n * n, 0, 0, 0], report.tolist()
    np.testing.assert_array_equal(lcs, _lcs_of_all_strings())
    # the rule does fire on misses: "aaaaaaa" against "bbbbbbb" at lmin = 1 is dead after the first character
    host.k13_host_abandon.restype = ctypes.c_int32
    assert host.k13_host_abandon(0, 1, 7, 7) == 1 and host.k13_host_abandon(1, 1, 7, 7) == 0 and host.k13_host_abandon(0, 0, 7, 7) == 0


@functools.lru_cache(None)
def _lcs_of_all_strings():
    strings = _all_strings(7)
    return indel_oracle.lcs_matrix(strings, strings)


def test_both_scales_order_every_two_pairs_alike(host):
    """all (lcs1, S1), (lcs2, S2) with S <= 160, lcs <= S / 2: indel_similarity and K4's ratio_of compare the same way -- <, == or >
    -- so K4's arg-max and top-n order ARE this scorer's"""
    report = np.zeros(2, np.int64)
    assert host.k13_host_order(160, _p(report)) == 0
    n = sum(s // 2 + 1 for s in range(161))
    assert report.tolist() == [n * n, 0], report.tolist()


def test_lcs_recovered_from_the_ratio_bits(host):
    """_lib.indel_lcs_of_ratio returns the right integer for every (lcs, S) with S <= 2000 (the ratio by K4's formula, both in
    numpy and in k10_core.h's ratio_of), indel_similarity is the oracle's, and a ratio that is nobody's raises"""
    from polyfuzz_amd import _lib
    s = np.repeat(np.arange(2001), np.arange(2001) // 2 + 1)
    lcs = np.concatenate([np.arange(k // 2 + 1) for k in range(2001)])
    sf = np.where(s > 0, s, 1).astype(np.float64)
    ratio = np.where(s > 0, (1.0 - (s - 2 * lcs) / sf) * 100.0, 100.0)
    np.testing.assert_array_equal(_lib.indel_lcs_of_ratio(ratio, s), lcs)
    assert _lib.indel_similarity(lcs, s).tobytes() == indel_oracle.similarity(lcs, s, 0).tobytes()
    for x, la, lb in ((0, 0, 0), (4, 6, 4), (17, 20, 31), (1, 1, 1), (0, 9, 0), (999, 1000, 1000)):
        r = host.k13_host_ratio(x, la, lb)
        assert int(_lib.indel_lcs_of_ratio(r, la + lb)) == x
        assert float(_lib.indel_similarity(x, la + lb)) == host.k13_host_similarity(x, la, lb)
    got = _lib.indel_lcs_of_ratio(np.array([[100.0, 80.0]]), np.array([[0, 10]]))
    assert got.shape == (1, 2) and got.tolist() == [[0, 4]]
    for bad, total in ((80.1, 10), (float(np.nextafter(80.0, 100.0)), 10), (50.0, 0), (101.0, 4)):
        with pytest.raises(ValueError):
            _lib.indel_lcs_of_ratio(bad, total)


def test_indel_scores_from_k4_rows():
    """the host conversion `match` / `top_n` use: ratios of given pairs -> the definition's float64, idx < 0 keeps 0.0; 1-D and 2-D"""
    from polyfuzz_amd.models._rapidfuzz import indel_scores
    fl, tl = ["ababab", "", "xyz"], ["abab", "", "zzzz", "xy"]
    lcs = indel_oracle.lcs_matrix(fl, tl)
    sim = indel_oracle.sim_matrix(fl, tl, lcs)
    idx = np.array([[0, 3, -1], [1, 0, 2], [3, 2, -1]], np.int32)
    ratio = np.where(idx >= 0, sim[np.arange(3)[:, None], np.maximum(idx, 0)] * 100.0, 0.0)
    got = indel_scores(fl, tl, idx, ratio)
    assert got.tobytes() == np.where(idx >= 0, sim[np.arange(3)[:, None], np.maximum(idx, 0)], 0.0).tobytes()
    assert got[1, 0] == 1.0 and got[0, 0] == indel_oracle.similarity(4, 6, 4)
    assert indel_scores(fl, tl, idx[:, 0], ratio[:, 0]).tobytes() == got[:, 0].tobytes()
    with pytest.raises(ValueError):
        indel_scores(fl, tl, idx[:, 0], ratio[:, 0] + 0.001)


def test_packed_hit_round_trip(host):
    out = np.empty(3, np.int32)
    for row, to, lcs in ((0, 0, 0), ((1 << 24) - 1, (1 << 24) - 1, 65535), (5, (1 << 24) - 1, 0), ((1 << 24) - 1, 0, 1), (123456, 654321, 4321)):
        host.k13_host_unpack(row, to, lcs, _p(out))
        assert out.tolist() == [row, to, lcs]
    header = open(os.path.join(REPO, "include", "polyfuzz_hip.h")).read()
    k13 = header[header.index("K13: all pairs"):header.index("int pfz_indel_join(")]
    assert "2^24" in k13 and "65 535" in k13 and "PFZ_ERR_UNSUPPORTED" in k13        # the limits the packing implies, stated
    core = open(os.path.join(REPO, "polyfuzz_amd", "csrc", "k13_core.h")).read()
    assert "2^24" in core and "65 535" in core and "131 070" in core


def _stand_in(name, module):          # looks like a compiled function of that module
    return type("builtin_function", (), {"__name__": name, "__module__": module, "__call__": lambda self, a, b: 1.0})()


def test_scorer_resolution():
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import BlockedEditDistance, EditDistance, RapidFuzz
    for name in ("indel", "indel_normalized_similarity"):
        assert EditDistance(scorer=name)._scorer_name == "indel"
    for module in ("Indel", "Indel_py"):
        assert EditDistance(scorer=_stand_in("normalized_similarity", "rapidfuzz.distance." + module))._scorer_name == "indel"
    try:
        from rapidfuzz.distance import Indel
        assert EditDistance(scorer=Indel.normalized_similarity)._scorer_name == "indel"
    except ImportError:
        pass
    for bad in ("Indel", "indel_distance", "indel_similarity", "lcs",
                functools.partial(_stand_in("normalized_similarity", "rapidfuzz.distance.Indel"), score_cutoff=0.5),
                _stand_in("normalized_distance", "rapidfuzz.distance.Indel"), _stand_in("distance", "rapidfuzz.distance.Indel"),
                _stand_in("similarity", "rapidfuzz.distance.Indel"), _stand_in("normalized_similarity", "rapidfuzz.distance"),
                _stand_in("normalized_similarity", "rapidfuzz.distance.LCSseq"), _stand_in("normalized_similarity", "rapidfuzz.distance.Hamming"),
                _stand_in("normalized_similarity", "rapidfuzz.distance.DamerauLevenshtein"),
                _stand_in("normalized_similarity", "notrapidfuzz.distance.Indel"), _stand_in("normalized_similarity", "rapidfuzz.distance.Indel.x")):
        with pytest.raises(NotImplementedError):
            EditDistance(scorer=bad)
    for cls in (RapidFuzz, BlockedEditDistance):          # K7's and K10's matchers do not learn the name
        for s in ("indel", _stand_in("normalized_similarity", "rapidfuzz.distance.Indel")):
            with pytest.raises(NotImplementedError):
                cls(scorer=s)
    assert "indel" not in _lib.LEV_SCORERS and "indel" not in _lib.PAIR_SCORERS
    m = EditDistance(scorer="indel", normalize=False)
    m.top_n = 5
    back = pickle.loads(pickle.dumps(m))
    assert back._scorer_name == "indel" and back.top_n == 5 and back.normalize is False and back.scorer == "indel"
    for doc in (EditDistance.__doc__, EditDistance.join.__doc__, EditDistance.components.__doc__):
        assert "indel" in doc and "K13" in doc


def _no_device(*a, **k):
    raise AssertionError("the device was reached")


def test_min_similarity_must_be_a_number_in_0_1(monkeypatch):
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import EditDistance
    monkeypatch.setattr(_lib.Context, "default", classmethod(_no_device))
    m = EditDistance(scorer="indel")
    for bad in (float("nan"), float("inf"), -float("inf"), -1e-300, np.nextafter(1.0, 2.0), 1.5, -0.1, "0.8", None, True, [0.8]):
        with pytest.raises(ValueError):
            m.join(["a", "b"], ["a"], bad)
        with pytest.raises(ValueError):
            m.join(["a", "b"], min_similarity=bad)
        with pytest.raises(ValueError):
            m.components(["a", "b"], bad)
    for good in (0, 1, 0.0, 1.0, 0.8, np.float64(0.5), np.float32(0.25), np.int64(1)):      # accepted: the device is what stops these
        with pytest.raises(AssertionError, match="the device was reached"):
            m.join(["a", "b"], ["a"], good)
        with pytest.raises(AssertionError, match="the device was reached"):
            m.components(["a", "b"], good)


def test_entry_points_in_header_library_and_table():
    from polyfuzz_amd import _build, _lib
    if _build.is_stale():
        _build.build()
    header = open(os.path.join(REPO, "include", "polyfuzz_hip.h")).read()
    so = ctypes.CDLL(_lib.lib_path())
    want = {"pfz_indel_join": ["ctx", "from_strings", "to_strings", "min_similarity", "capacity", "out_row_ptr", "out_idx", "out_dist",
                               "out_sim", "out_total", "out_counters"],
            "pfz_indel_components": ["ctx", "strings", "min_similarity", "out_label", "out_pairs", "out_components", "out_counters"]}
    for name, args in want.items():
        assert f"int {name}(" in header and hasattr(so, name) and name in _lib.SIGNATURES
        decl = header[header.index(f"int {name}("):]
        decl = decl[:decl.index(";")]
        assert [a.strip().split()[-1].lstrip("*") for a in decl[decl.index("(") + 1:decl.rindex(")")].split(",")] == args
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(args) and argtypes[args.index("min_similarity")] is ctypes.c_double
    assert _lib.SIGNATURES["pfz_indel_join"][1][4] is ctypes.c_int64
    assert callable(_lib.indel_join) and callable(_lib.indel_components)
    assert _lib.LEV_SCORERS == {"levenshtein": 0, "osa": 1}


def test_kernel_budget():
    """K13's register kernels (32- / 64-bit words x 8- / 16-bit symbols, join and components): no scratch, at most 64 registers --
    eight waves per SIMD; the general kernels and K13's instances of edit_walk.h's begin and unpack kernels: no scratch"""
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_budget
    from polyfuzz_amd import _build
    for exe in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(kernel_budget.LLVM, exe)):
            pytest.skip(f"{exe} not in {kernel_budget.LLVM}")
    md = kernel_budget.kernel_metadata(_build.build())
    pretty = dict(zip(md, kernel_budget.demangled(list(md))))
    k13 = {pretty[k].split("(")[0]: v for k, v in md.items() if "k13_" in pretty[k] or "walk_begin_kernel<pfz::LminByS>" in pretty[k]
           or "edit_unpack_kernel<pfz::IndelScore>" in pretty[k]}
    reg = {n: v for n, v in k13.items() if "k13_join_kernel" in n or "k13_comp_kernel" in n}
    assert sorted(reg) == sorted(f"void pfz::k13_{kind}_kernel<unsigned {w}, {idb}>" for kind in ("join", "comp") for w in ("int", "long")
                                 for idb in (8, 16)), sorted(reg)
    assert len(k13) == 8 + 4 + 2, sorted(k13)      # (the flattening is K12's)
    assert any("walk_begin_kernel<pfz::LminByS>" in n for n in k13) and any("edit_unpack_kernel<pfz::IndelScore>" in n for n in k13)
    for name, k in k13.items():
        assert k["scratch"] == 0, (name, k)
    for name, k in reg.items():
        print(name, k)
        assert k["vgpr"] <= 64 and k["lds"] % 16 == 0, (name, k)
