"""K9 (Levenshtein / OSA similarity) without a GPU: the oracle the GPU tests compare with (tests/lev_oracle.py) against the values
every write-up publishes, its numpy form == the plain table, the kernel's bit logic (polyfuzz_amd/csrc/k9_core.h, compiled for the
host: one word and several) against that oracle, the float64 formula, the scorer gate of EditDistance, the three entry points in
header / library / ctypes table, the register and LDS budget of the kernels, and the live pin against rapidfuzz itself wherever it
is installed (PARITY UNPINNED otherwise)."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import lev_oracle

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def _rand(rng, alpha, lo, hi, n):
    return ["".join(rng.choice(list(alpha), size=int(rng.integers(lo, hi + 1)))) for _ in range(n)]


def test_oracle_published_values():
    d = lev_oracle.distance
    for a, b, lev, osa in (("kitten", "sitting", 3, 3), ("lewenstein", "levenshtein", 2, 2), ("flaw", "lawn", 2, 2), ("CA", "ABC", 3, 3),
                           ("ab", "ba", 2, 1), ("", "", 0, 0), ("", "abc", 3, 3), ("abc", "", 3, 3), ("abcd", "acbd", 2, 1)):
        assert (d(a, b, "levenshtein"), d(a, b, "osa")) == (lev, osa), (a, b)
        m = {s: lev_oracle.matrix([a], [b], s) for s in lev_oracle.SCORERS}
        assert (int(m["levenshtein"][0, 0]), int(m["osa"][0, 0])) == (lev, osa), (a, b)
    sim = lev_oracle.similarity
    assert sim(0, 0, 0) == 1.0 and sim(3, 0, 3) == 0.0 and sim(3, 3, 0) == 0.0
    assert sim(3, 6, 7) == 1.0 - 3.0 / 7.0 and sim(1, 2, 2) == 0.5 and sim(0, 5, 5) == 1.0
    idx, score = lev_oracle.argmax(np.array([[0.5, 0.75, 0.75], [1.0, 0.0, 1.0]]))
    assert idx.tolist() == [1, 0] and score.tolist() == [0.75, 1.0]
    idx, score = lev_oracle.argmax(np.array([[0.5, 0.75, 0.75], [1.0, 0.0, 1.0]]), np.array([1, -4], np.int32))
    assert idx.tolist() == [2, -1] and score.tolist() == [0.75, 0.0]


@pytest.mark.parametrize("scorer", lev_oracle.SCORERS)
def test_numpy_matrix_equals_the_plain_table(scorer):
    """5 400 seeded pairs per scorer: alphabets of 2 and 9 letters, lengths 0 .. 70 on either side"""
    rng = np.random.default_rng(91)
    pairs = 0
    for alpha in ("ab", "abcdefghi"):
        fl = _rand(rng, alpha, 0, 70, 43) + ["", "ab"]
        tl = _rand(rng, alpha, 0, 70, 58) + ["", "ba"]
        got = lev_oracle.matrix(fl, tl, scorer)
        want = np.array([[lev_oracle.distance(a, b, scorer) for b in tl] for a in fl], np.int32)
        np.testing.assert_array_equal(got, want)
        pairs += got.size
    assert pairs >= 5000
    if scorer == "osa":
        assert (got < lev_oracle.matrix(fl, tl, "levenshtein")).any()


@pytest.fixture(scope="module")
def host():
    so = os.path.join(REPO, "oracle", "_build", "k9_core_host.so")
    src = [os.path.join(HERE, "k9_core_host.cpp"), os.path.join(REPO, "polyfuzz_amd", "csrc", "k9_core.h")]
    os.makedirs(os.path.dirname(so), exist_ok=True)
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", src[0], "-o", so])
    lib = ctypes.CDLL(so)
    lib.k9_host_pairs.restype = ctypes.c_int
    return lib


def _symbols(strings, rank):
    off = np.zeros(len(strings) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in strings])
    sym = np.array([rank.get(c, 0) for s in strings for c in s] + [0], np.int32)
    return sym, off


def _host_distances(lib, word_bits, fl, tl, osa):
    rank = {c: k + 1 for k, c in enumerate(sorted({c for s in tl for c in s}))}      # the to-list's alphabet, as K4's plan ranks it
    (a, a_off), (b, b_off) = _symbols(fl, rank), _symbols(tl, rank)
    out = np.empty((len(fl), len(tl)), np.int32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    rc = lib.k9_host_pairs(word_bits, int(osa), ctypes.c_int64(len(fl)), p(a), p(a_off), ctypes.c_int64(len(tl)), p(b), p(b_off),
                           len(rank) + 1, p(out))
    assert rc == 0
    return out


BORDER_LENGTHS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)


def _border_lists():
    """from-strings of every border length of the word classes over 2 and 9 letters, transposition-heavy ones, characters the
    to-list never uses; to-strings of 0 .. 300"""
    rng = np.random.default_rng(92)
    fl = [s for n in BORDER_LENGTHS for s in _rand(rng, "ab", n, n, 2) + _rand(rng, "abcdefghi", n, n, 2)]
    fl += ["ab" * 16, "ba" * 16, "ab" * 32, "ab" * 64 + "a", "CA", "zq", "azbq" * 9, "abcdefghi" * 20] + _rand(rng, "abc", 1, 40, 20)
    tl = _rand(rng, "ab", 0, 70, 40) + _rand(rng, "abcdefghi", 0, 140, 50) + ["", "ba" * 16, "ab" * 16, "ba" * 32, "ba" * 64, "ABC", "ab"]
    tl += [fl[k][1:] for k in range(8, len(fl), 5)] + [fl[k][:-2] + "ba" for k in range(9, len(fl), 5)] + _rand(rng, "ab", 250, 300, 3)
    return fl, tl


def test_bit_logic_matches_the_definition(host):
    """the single-word recurrence (32 and 64 bits, with the padding steps a group's longest string makes the other lanes take) and
    the multi-word one (the carry of the addition and the bits shifted out of HP, HN and OSA's operand, from word to word) over the
    same pairs: == the table, and == each other"""
    fl, tl = _border_lists()
    assert set(BORDER_LENGTHS) <= {len(s) for s in fl}
    for osa, scorer in enumerate(lev_oracle.SCORERS):
        want = lev_oracle.matrix(fl, tl, scorer)
        multi = _host_distances(host, 0, fl, tl, osa)
        np.testing.assert_array_equal(multi, want, err_msg=scorer)
        for word_bits in (64, 32):
            keep = [i for i, s in enumerate(fl) if len(s) <= word_bits]
            assert max(len(fl[i]) for i in keep) == word_bits
            got = _host_distances(host, word_bits, [fl[i] for i in keep], tl, osa)
            np.testing.assert_array_equal(got, want[keep], err_msg=f"{scorer} {word_bits}")
            np.testing.assert_array_equal(got, multi[keep])
    lev, osa = lev_oracle.matrix(fl, tl, "levenshtein"), lev_oracle.matrix(fl, tl, "osa")
    assert (osa <= lev).all() and (osa < lev).sum() > 50


COLUMN_FROM_LENGTHS = (0, 1, 63, 64, 65, 128, 129, 200)
COLUMN_TO_LENGTHS = (0, 1, 70)


@pytest.mark.parametrize("stride", (64, 256))
def test_shared_column_walk_matches_the_definition(host, stride):
    """lev_column_begin / lev_column_step -- the one multi-word column all four general kernels walk -- at both lane strides (256:
    K9, K11, K12; 64: K10), both scorers, from-lengths at every word border, to-lengths 0, 1 and 70 on more lanes than one stride
    holds, and a match table of WA = 4 words per symbol: W < WA for every from-string but the longest, W == WA for that one
    (the words beyond W must stay untouched: the host program poisons and checks them)"""
    rng = np.random.default_rng(94)
    fl = [s for n in COLUMN_FROM_LENGTHS for s in _rand(rng, "ab", n, n, 2) + _rand(rng, "abcdefghi", n, n, 2)] + ["zq" * 35, "ab" * 100]
    tl = [""] + list("abz") + _rand(rng, "ab", 70, 70, 30) + _rand(rng, "abcdefghi", 70, 70, 30) + ["ba" * 35, "ab" * 35]
    tl += [s[:70] for s in fl if len(s) >= 128] + [""]
    assert set(COLUMN_FROM_LENGTHS) <= {len(s) for s in fl} and {len(s) for s in tl} == set(COLUMN_TO_LENGTHS) and len(tl) > 64
    rank = {c: k + 1 for k, c in enumerate(sorted({c for s in tl for c in s}))}
    (a, a_off), (b, b_off) = _symbols(fl, rank), _symbols(tl, rank)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    WA = (max(map(len, fl)) + 63) // 64
    assert WA == 4 and {(len(s) + 63) // 64 for s in fl} >= {0, 1, 2, 3, 4}
    for osa, scorer in enumerate(lev_oracle.SCORERS):
        out = np.empty((len(fl), len(tl)), np.int32)
        host.k9_host_column.restype = ctypes.c_int
        rc = host.k9_host_column(osa, stride, WA, ctypes.c_int64(len(fl)), p(a), p(a_off), ctypes.c_int64(len(tl)), p(b), p(b_off),
                                 len(rank) + 1, p(out))
        assert rc == 0, rc
        np.testing.assert_array_equal(out, lev_oracle.matrix(fl, tl, scorer), err_msg=f"{scorer} stride {stride}")
        np.testing.assert_array_equal(out, _host_distances(host, 0, fl, tl, osa))


def test_similarity_formula_and_length_bound(host):
    """k9_core.h's float64 similarity == numpy's for every d <= M < 400; distinct d / M give distinct scores and equal fractions
    equal ones (what lets the kernel order pairs by the float64 values); the length bound is the score of d = | |a| - |b| |, and no
    score of that pair of lengths is above it"""
    la, lb, d = [], [], []
    for m in range(0, 400):
        for other in {0, m // 2, m}:
            for dd in range(abs(m - other), m + 1):
                la.append(m), lb.append(other), d.append(dd)
                la.append(other), lb.append(m), d.append(dd)
    la, lb, d = (np.array(x, np.int32) for x in (la, lb, d))
    sim, bound = np.empty(len(d)), np.empty(len(d))
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    host.k9_host_similarity(ctypes.c_int64(len(d)), p(d), p(la), p(lb), p(sim), p(bound))
    np.testing.assert_array_equal(sim, lev_oracle.similarity(d, la, lb))
    np.testing.assert_array_equal(bound, lev_oracle.similarity(np.abs(la - lb), la, lb))
    assert (sim <= bound).all() and sim.min() == 0.0 and sim.max() == 1.0
    import fractions
    import math
    by_fraction = {}
    for s, dd, m in zip(sim.tolist(), d.tolist(), np.maximum(la, lb).tolist()):
        g = math.gcd(dd, m) or 1
        by_fraction.setdefault((dd // g, m // g if dd else 1), set()).add(s)
    assert all(len(v) == 1 for v in by_fraction.values()) and len(by_fraction) > 40_000
    order = sorted(by_fraction, key=lambda f: fractions.Fraction(*f))
    values = [next(iter(by_fraction[f])) for f in order]
    assert all(x > y for x, y in zip(values, values[1:]))          # a larger d / M is a strictly smaller float64 score


def _stand_in(name, module):          # looks like a compiled function of that module
    return type("builtin_function", (), {"__name__": name, "__module__": module, "__call__": lambda self, a, b: 1.0})()


def test_scorer_gate():
    from polyfuzz_amd.models import EditDistance, RapidFuzz
    for name, k9 in (("levenshtein", "levenshtein"), ("levenshtein_normalized_similarity", "levenshtein"), ("osa", "osa"),
                     ("osa_normalized_similarity", "osa")):
        assert EditDistance(scorer=name)._scorer_name == k9
    for module, k9 in (("Levenshtein", "levenshtein"), ("Levenshtein_py", "levenshtein"), ("OSA", "osa"), ("OSA_py", "osa")):
        assert EditDistance(scorer=_stand_in("normalized_similarity", "rapidfuzz.distance." + module))._scorer_name == k9

    def normalized_similarity(a, b):   # somebody else's function of that name
        return 1.0
    refused = [normalized_similarity,
               functools.partial(_stand_in("normalized_similarity", "rapidfuzz.distance.Levenshtein"), weights=(1, 1, 2)),
               functools.partial(_stand_in("normalized_similarity", "rapidfuzz.distance.OSA"), score_cutoff=0.5),
               _stand_in("normalized_distance", "rapidfuzz.distance.Levenshtein"), _stand_in("distance", "rapidfuzz.distance.Levenshtein"),
               _stand_in("similarity", "rapidfuzz.distance.OSA"), _stand_in("distance", "rapidfuzz.distance.OSA"),
               _stand_in("normalized_similarity", "rapidfuzz.distance.DamerauLevenshtein"),
               _stand_in("normalized_similarity", "rapidfuzz.distance.Hamming"), _stand_in("normalized_similarity", "rapidfuzz.distance"),
               _stand_in("normalized_similarity", "notrapidfuzz.distance.Levenshtein"),
               _stand_in("levenshtein_distance", "jellyfish"), _stand_in("levenshtein_distance", "jellyfish._rustyfish"),
               _stand_in("damerau_levenshtein_distance", "jellyfish"),
               _stand_in("ratio", "Levenshtein"), _stand_in("ratio", "Levenshtein._levenshtein"), _stand_in("distance", "Levenshtein"),
               "levenshtein_distance", "levenshtein_normalized_distance", "osa_distance", "damerau_levenshtein", "hamming", "Levenshtein"]
    for scorer in refused:
        with pytest.raises(NotImplementedError):
            EditDistance(scorer=scorer)
    for name in ("levenshtein", "osa", "levenshtein_normalized_similarity", "osa_normalized_similarity"):
        with pytest.raises(NotImplementedError):
            RapidFuzz(scorer=name)           # its contract is rapidfuzz's 0..100 scale / 100
    with pytest.raises(NotImplementedError):
        RapidFuzz(scorer=_stand_in("normalized_similarity", "rapidfuzz.distance.Levenshtein"))
    # what was accepted before still is, under its own name
    assert EditDistance()._scorer_name == "ratio" and EditDistance(scorer="jaro_winkler")._scorer_name == "jaro_winkler"
    assert EditDistance(scorer=_stand_in("WRatio", "rapidfuzz.fuzz"))._scorer_name == "WRatio"


def test_entry_points_in_header_library_and_table():
    from polyfuzz_amd import _build, _lib
    if _build.is_stale():
        _build.build()
    header = open(os.path.join(REPO, "include", "polyfuzz_hip.h")).read()
    so = ctypes.CDLL(_lib.lib_path())
    for sym in ("pfz_lev_argmax", "pfz_lev_argmax_dev", "pfz_lev_matrix_host"):
        assert f"int {sym}(" in header and hasattr(so, sym) and sym in _lib.SIGNATURES
        assert _lib.SIGNATURES[sym] == _lib.SIGNATURES[sym.replace("_lev_", "_jaro_")]
    assert _lib.LEV_SCORERS == {"levenshtein": 0, "osa": 1}
    assert "_distance.py:89-102" in header[header.index("K9: all-pairs Levenshtein"):header.index("int pfz_lev_argmax(")]
    for f in (_lib.lev_argmax, _lib.lev_argmax_dev, _lib.lev_matrix):
        assert callable(f)


def test_no_device_no_fallback():
    import polyfuzz_amd
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import EditDistance
    if polyfuzz_amd.device_count() > 0:
        pytest.skip("a GPU is visible: the no-device failure path cannot be exercised")
    for name in lev_oracle.SCORERS:
        with pytest.raises(_lib.PfzNoDevice):
            EditDistance(scorer=name).match(["a"], ["b"])


def test_kernel_budget():
    """the eight register-kernel instances (32- / 64-bit words x 8- / 16-bit symbols x Levenshtein / OSA): no scratch, static LDS
    within K8's 48 bytes (the match table and the workgroup's best are dynamic), and at most 64 registers -- eight waves per SIMD
    (measured: 42 .. 45 in 32-bit words, 47 .. 54 in 64-bit words); the general kernel is held to no scratch"""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_budget
    from polyfuzz_amd import _build
    for exe in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(kernel_budget.LLVM, exe)):
            pytest.skip(f"{exe} not in {kernel_budget.LLVM}")
    md = kernel_budget.kernel_metadata(_build.build())
    pretty = dict(zip(md, kernel_budget.demangled(list(md))))
    k8_lds = max(v["lds"] for k, v in md.items() if "k8_jaro_kernel" in pretty[k])
    hits = {pretty[k].split("(")[0]: v for k, v in md.items() if "k9_lev_kernel" in pretty[k]}
    assert sorted(hits) == sorted(f"void pfz::k9_lev_kernel<unsigned {w}, {idb}, {osa}>" for w in ("int", "long") for idb in (8, 16)
                                  for osa in ("false", "true")), sorted(hits)
    for name, k in hits.items():
        assert k["scratch"] == 0 and k["lds"] <= k8_lds and k["lds"] % 16 == 0, (name, k)
        assert k["vgpr"] <= (56 if "unsigned int" in name else 64), (name, k)
    general = [v for k, v in md.items() if "k9_lev_general_kernel" in pretty[k]]
    assert len(general) == 4 and all(k["scratch"] == 0 for k in general)


def test_live_rapidfuzz_pin():
    """the oracle against rapidfuzz itself on the titles sample, and rapidfuzz's own functions through the scorer gate.  PARITY
    UNPINNED where rapidfuzz is not importable."""
    pytest.importorskip("rapidfuzz")
    from rapidfuzz.distance import OSA, Levenshtein
    from polyfuzz_amd import datasets
    from polyfuzz_amd.models import EditDistance, RapidFuzz
    rng = np.random.default_rng(3)
    fl, tl = datasets.c3_lists(120)
    rnd = _rand(rng, "ab", 1, 70, 80)
    fl, tl = fl[:60] + rnd[:40] + ["", "a", "CA", "ab"], tl[:60] + rnd[40:] + ["", "a", "ABC", "ba", "é" * 5, "\U0001f600b"]
    for name, mod in (("levenshtein", Levenshtein), ("osa", OSA)):
        d = lev_oracle.matrix(fl, tl, name)
        np.testing.assert_array_equal(d, np.array([[mod.distance(a, b) for b in tl] for a in fl], np.int32))
        want = np.array([[mod.normalized_similarity(a, b) for b in tl] for a in fl])
        np.testing.assert_array_equal(lev_oracle.sim_matrix(fl, tl, d), want)
        assert EditDistance(scorer=mod.normalized_similarity)._scorer_name == name
        for refused in (mod.distance, mod.normalized_distance, mod.similarity, functools.partial(mod.normalized_similarity, score_cutoff=0.5)):
            with pytest.raises(NotImplementedError):
                EditDistance(scorer=refused)
        with pytest.raises(NotImplementedError):
            RapidFuzz(scorer=mod.normalized_similarity)
