"""K8 (Jaro / Jaro-Winkler) without a GPU: the oracle the GPU tests compare with against the values every Jaro write-up
publishes, its C restatement (oracle/jaro.c, what the GPU tests of more than a few thousand pairs use) == the Python statement,
the kernel's bit logic (polyfuzz_amd/csrc/k8_core.h, compiled for the host) against that oracle, the scorer gate
of EditDistance, the three entry points in header / library / ctypes table, and the live pin against jellyfish itself
wherever it is installed (PARITY UNPINNED otherwise)."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import jaro_oracle

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def test_oracle_published_values():
    """Winkler's examples, as exact fractions evaluated in float64"""
    j, w = jaro_oracle.jaro_similarity, jaro_oracle.jaro_winkler_similarity
    assert j("MARTHA", "MARHTA") == (6 / 6 + 6 / 6 + 5 / 6) / 3                  # 17/18 = 0.9444...
    assert w("MARTHA", "MARHTA") == 17 / 18 + (3 * 0.1) * (1.0 - 17 / 18)        # 0.9611...
    assert abs(j("MARTHA", "MARHTA") - 17 / 18) < 1e-15
    assert j("DWAYNE", "DUANE") == (4 / 6 + 4 / 5 + 4 / 4) / 3                   # 0.8222...
    assert abs(w("DWAYNE", "DUANE") - 0.84) < 1e-15
    assert j("DIXON", "DICKSONX") == (4 / 5 + 4 / 8 + 4 / 4) / 3                 # 0.7666...
    assert abs(w("DIXON", "DICKSONX") - (0.8 + 1 / 75)) < 1e-15                  # 0.8133...
    assert j("CRATE", "TRACE") == (3 / 5 + 3 / 5 + 3 / 3) / 3                    # 0.7333...
    for f in (j, w):
        assert f("", "") == 0.0 and f("", "abc") == 0.0 and f("abc", "") == 0.0
        assert f("a", "a") == 1.0 and f("polyfuzz", "polyfuzz") == 1.0 and f("abc", "xyz") == 0.0


@pytest.fixture(scope="module")
def host():
    so = os.path.join(REPO, "oracle", "_build", "k8_core_host.so")
    src = [os.path.join(HERE, "k8_core_host.cpp"), os.path.join(REPO, "polyfuzz_amd", "csrc", "k8_core.h")]
    os.makedirs(os.path.dirname(so), exist_ok=True)
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", src[0], "-o", so])
    lib = ctypes.CDLL(so)
    lib.k8_host_pairs.restype = ctypes.c_int
    return lib


def _symbols(strings, rank):
    off = np.zeros(len(strings) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in strings])
    sym = np.array([rank.get(c, 0) for s in strings for c in s] + [0], np.int32)
    return sym, off


def _host_scores(lib, word_bits, fl, tl, winkler):
    rank = {c: k + 1 for k, c in enumerate(sorted({c for s in tl for c in s}))}      # the to-list's alphabet, as K4's plan ranks it
    (a, a_off), (b, b_off) = _symbols(fl, rank), _symbols(tl, rank)
    out, ub = np.empty((len(fl), len(tl))), np.empty((len(fl), len(tl), 2), np.float32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    rc = lib.k8_host_pairs(word_bits, ctypes.c_int64(len(fl)), p(a), p(a_off), ctypes.c_int64(len(tl)), p(b), p(b_off), len(rank) + 1, int(winkler),
                           p(out), p(ub))
    assert rc == 0
    return out, ub


def _mixed_lists():
    """about 130 x 190: dense random strings over two, three and nine letters up to 64 characters, real titles, the published
    pairs, the edges of the 32- and 64-bit words, the empty string"""
    from polyfuzz_amd import datasets
    rng = np.random.default_rng(8)
    mk = lambda alpha, lo, hi, n: ["".join(rng.choice(list(alpha), size=int(rng.integers(lo, hi + 1)))) for _ in range(n)]
    titles_f, titles_t = datasets.c3_lists(200)
    fl = mk("ab", 1, 64, 40) + mk("abc", 1, 12, 20) + mk("abcdefgh ", 20, 64, 10) + [s for s in titles_f if len(s) <= 64][:40]
    tl = mk("ab", 1, 64, 60) + mk("abc", 1, 12, 30) + mk("abcdefgh ", 20, 64, 20) + [s for s in titles_t if len(s) <= 64][:60]
    edge = ["", "a", "b", "ab", "ba", "a" * 64, "ab" * 32, "a" * 63, "b" + "a" * 63, "MARTHA", "MARHTA", "DWAYNE", "DUANE", "DIXON",
            "DICKSONX", "CRATE", "TRACE", "x" * 31, "x" * 32, "x" * 33, "zq", "abcdefgh" * 8]
    return fl + edge, tl + edge[:-2]          # ("zq": from-characters the to-list never uses)


def test_c_oracle_published_values(oracle_mod):
    """test_oracle_published_values through oracle/jaro.c's entry"""
    pairs = [("MARTHA", "MARHTA"), ("DWAYNE", "DUANE"), ("DIXON", "DICKSONX"), ("CRATE", "TRACE"), ("", ""), ("", "abc"), ("abc", ""),
             ("a", "a"), ("polyfuzz", "polyfuzz"), ("abc", "xyz")]
    fl, tl = [a for a, _ in pairs], [b for _, b in pairs]
    j, w = (np.diag(oracle_mod.jaro_matrix(fl, tl, name)) for name in ("jaro", "jaro_winkler"))
    assert j[0] == (6 / 6 + 6 / 6 + 5 / 6) / 3 and w[0] == 17 / 18 + (3 * 0.1) * (1.0 - 17 / 18)
    assert j[1] == (4 / 6 + 4 / 5 + 4 / 4) / 3 and abs(w[1] - 0.84) < 1e-15
    assert j[2] == (4 / 5 + 4 / 8 + 4 / 4) / 3 and abs(w[2] - (0.8 + 1 / 75)) < 1e-15
    assert j[3] == (3 / 5 + 3 / 5 + 3 / 3) / 3
    for s in (j, w):
        assert s[4:].tolist() == [0.0, 0.0, 0.0, 1.0, 1.0, 0.0]


def test_c_oracle_equals_the_python_oracle(oracle_mod):
    """oracle/jaro.c == tests/jaro_oracle.py, float64 bit for bit: every pair of the mixed list of the bit-logic test; strings beyond
    64 and beyond 256 characters on either side and on both, empty strings, code points above 0xFFFF; the matrix on a row shard; the
    arg-max under the three skip forms (none, one choice, "up to"), rows without a choice included"""
    rng = np.random.default_rng(18)
    mk = lambda alpha, lo, hi, n: ["".join(rng.choice(list(alpha), size=int(rng.integers(lo, hi + 1)))) for _ in range(n)]
    fl, tl = _mixed_lists()
    assert len(fl) >= 130 and len(tl) >= 180 and "" in fl and "" in tl
    base = "the quick brown fox jumps over the lazy dog and runs far away from home again "
    astral = ["\U0001f600\U0001f601", "na\u00efve caf\u00e9 \u03a9mega \U0001f600 smile", "\U00010000\uffff\U0010ffff", "qqq\u4e2d\u6587"]
    fl = fl + mk("ab", 65, 300, 4) + mk("abcdefgh ", 250, 400, 2) + [(base * 6)[:n] for n in (65, 256, 257, 400)] + astral
    tl = tl + mk("ab", 65, 300, 4) + mk("abcdefgh ", 250, 400, 2) + [(base * 6)[3:3 + n] for n in (65, 256, 257, 400)] + astral[::-1] + \
        ["\U0001f601\U0001f600", "\uffff\U00010000"]
    assert max(map(len, fl)) > 256 and max(map(len, tl)) > 256
    n = len(fl)
    up_to = (-2 - rng.integers(0, len(tl) - 1, n)).astype(np.int32)
    up_to[::7] = -1
    up_to[-3:] = -2 - (len(tl) - 1)                      # no choice left
    for name in ("jaro", "jaro_winkler"):
        want = jaro_oracle.matrix(fl, tl, name)
        np.testing.assert_array_equal(oracle_mod.jaro_matrix(fl, tl, name), want, err_msg=name)
        np.testing.assert_array_equal(oracle_mod.jaro_matrix(fl, tl, name, rows=(17, 60)), want[17:60])
        one = jaro_oracle.argmax(want)[0].copy()         # the row's own best: the next one must win
        one[::5] = -1
        for skip in (None, one, up_to):
            e_idx, e_score = jaro_oracle.argmax(want, skip)
            idx, score = oracle_mod.jaro_argmax(fl, tl, name, skip)
            assert idx.dtype == np.int32 and score.dtype == np.float64
            np.testing.assert_array_equal(idx, e_idx, err_msg=name)
            np.testing.assert_array_equal(score, e_score, err_msg=name)
            idx, score = oracle_mod.jaro_argmax(fl, tl, name, skip, rows=(n - 40, n))
            np.testing.assert_array_equal(idx, e_idx[-40:])
            np.testing.assert_array_equal(score, e_score[-40:])
        assert (oracle_mod.jaro_argmax(fl, tl, name, up_to)[0][-3:] == -1).all()
    assert oracle_mod.jaro_matrix(fl, [], "jaro").shape == (n, 0) and (oracle_mod.jaro_argmax(fl, [], "jaro")[0] == -1).all()


def test_bit_logic_matches_the_definition(host):
    """one flag word per side (the kernel's two classes: 32 and 64 bits), to-major: window masks at every length up to the
    word, lowest-bit flagging, the transposition sweep, the prefix, the float64 formula -- exactly the from-major definition;
    and the two float32 bounds the kernel skips exact scores with (bound + 1e-4 below the running best: from m alone, and
    with t) never fall short of the score, the second never by more than the margin above it"""
    fl, tl = _mixed_lists()
    for word_bits in (64, 32):
        fw, tw = [s for s in fl if len(s) <= word_bits], [s for s in tl if len(s) <= word_bits]
        assert max(map(len, fw)) == word_bits == max(map(len, tw))
        ok = np.array([[len(a) > 0 and len(b) > 0 for b in tw] for a in fw])
        for name, winkler in (("jaro", 0), ("jaro_winkler", 1)):
            got, ub = _host_scores(host, word_bits, fw, tw, winkler)
            want = jaro_oracle.matrix(fw, tw, name)
            np.testing.assert_array_equal(got, want)
            assert (ub[ok][:, 0] + 1e-4 >= want[ok]).all()
            hit = want > 0                            # (m = 0 scores 0 whatever the bound says: (m - t) / m is 0 / 0, not a number)
            assert (ub[hit][:, 1] + 1e-4 >= want[hit]).all() and (ub[hit][:, 1] <= want[hit] + 1e-4).all()
            assert (ub[hit][:, 1] <= ub[hit][:, 0] + 1e-6).all()


def test_scorer_gate():
    from polyfuzz_amd.models import EditDistance, RapidFuzz
    for name, k8 in (("jaro", "jaro"), ("jaro_similarity", "jaro"), ("jaro_winkler", "jaro_winkler"),
                     ("jaro_winkler_similarity", "jaro_winkler")):
        assert EditDistance(scorer=name)._scorer_name == k8

    def stand_in(name, module):          # looks like a compiled function of that module
        return type("builtin_function", (), {"__name__": name, "__module__": module, "__call__": lambda self, a, b: 1.0})()
    assert EditDistance(scorer=stand_in("jaro_winkler_similarity", "jellyfish._rustyfish"))._scorer_name == "jaro_winkler"
    assert EditDistance(scorer=stand_in("jaro_similarity", "jellyfish"))._scorer_name == "jaro"

    def jaro_winkler_similarity(a, b):   # somebody else's function of that name
        return 1.0
    with pytest.raises(NotImplementedError):
        EditDistance(scorer=jaro_winkler_similarity)
    with pytest.raises(NotImplementedError):
        EditDistance(scorer=stand_in("jaro_similarity", "notjellyfish.x"))
    with pytest.raises(NotImplementedError):
        EditDistance(scorer=stand_in("hamming_distance", "jellyfish"))
    with pytest.raises(NotImplementedError):
        EditDistance(scorer=functools.partial(stand_in("jaro_winkler_similarity", "jellyfish"), long_tolerance=True))
    with pytest.raises(NotImplementedError):
        EditDistance(scorer="jaro_winkler_distance")
    with pytest.raises(NotImplementedError):
        RapidFuzz(scorer="jaro")             # its contract is rapidfuzz's 0..100 scale / 100
    with pytest.raises(NotImplementedError):
        RapidFuzz(scorer="jaro_winkler_similarity")


def test_entry_points_in_header_library_and_table():
    from polyfuzz_amd import _build, _lib
    if _build.is_stale():
        _build.build()
    header = open(os.path.join(REPO, "include", "polyfuzz_hip.h")).read()
    so = ctypes.CDLL(_lib.lib_path())
    for sym in ("pfz_jaro_argmax", "pfz_jaro_argmax_dev", "pfz_jaro_matrix_host"):
        assert f"int {sym}(" in header and hasattr(so, sym) and sym in _lib.SIGNATURES
    assert _lib.JARO_SCORERS == {"jaro": 0, "jaro_winkler": 1}


def test_no_device_no_fallback():
    import polyfuzz_amd
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import EditDistance
    if polyfuzz_amd.device_count() > 0:
        pytest.skip("a GPU is visible: the no-device failure path cannot be exercised")
    with pytest.raises(_lib.PfzNoDevice):
        EditDistance(scorer="jaro_winkler").match(["a"], ["b"])


def test_live_jellyfish_pin():
    """the oracle (the Python statement and oracle/jaro.c) against jellyfish itself, and jellyfish's own functions through the scorer
    gate.  PARITY UNPINNED where jellyfish is not importable."""
    jellyfish = pytest.importorskip("jellyfish")
    import oracle
    from polyfuzz_amd import datasets
    from polyfuzz_amd.models import EditDistance
    rng = np.random.default_rng(3)
    fl, tl = datasets.c3_lists(120)
    rnd = ["".join(rng.choice(list("ab"), size=int(rng.integers(1, 71)))) for _ in range(80)]
    fl, tl = fl[:60] + rnd[:40] + ["", "a"], tl[:60] + rnd[40:] + ["", "a", "é" * 5, "\U0001f600b"]
    for name, f in (("jaro", jellyfish.jaro_similarity), ("jaro_winkler", jellyfish.jaro_winkler_similarity)):
        want = np.array([[f(a, b) for b in tl] for a in fl])
        np.testing.assert_array_equal(jaro_oracle.matrix(fl, tl, name), want)
        np.testing.assert_array_equal(oracle.jaro_matrix(fl, tl, name), want)
        assert EditDistance(scorer=f)._scorer_name == name
    with pytest.raises(NotImplementedError):
        EditDistance(scorer=functools.partial(jellyfish.jaro_winkler_similarity, long_tolerance=True))
