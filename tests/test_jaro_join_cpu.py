"""K20 (all pairs at or above a Jaro / Jaro-Winkler score) without a GPU: every dismissal a fixed threshold allows
(polyfuzz_amd/csrc/k8_core.h, compiled for the host by tests/k20_core_host.cpp) against jaro_score, exhaustively; the whole
decision on one pair as the register kernels take it against the from-major definition thresholded; the symmetry of the score the
self-join's ownership rule rests on; the gates of models.JaroWinkler; the entry points in header, library and ctypes table."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

from tests import jaro_oracle

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
TWO_THIRDS = 2.0 / 3.0
THRESHOLDS = (0.0, 0.5, TWO_THIRDS, 0.7, 0.8, 0.9, 0.95, 1.0)
SCORERS = (("jaro", 0), ("jaro_winkler", 1))


def host_lib():
    """tests/k20_core_host.cpp as a shared library (built the way tests/test_jaro_cpu.py builds K8's)"""
    so = os.path.join(REPO, "oracle", "_build", "k20_core_host.so")
    src = [os.path.join(HERE, "k20_core_host.cpp"), os.path.join(REPO, "polyfuzz_amd", "csrc", "k8_core.h")]
    os.makedirs(os.path.dirname(so), exist_ok=True)
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", src[0], "-o", so + ".tmp"])
        os.replace(so + ".tmp", so)
    lib = ctypes.CDLL(so)
    lib.k20_host_dismissals.restype = ctypes.c_int64
    lib.k20_host_pairs.restype = ctypes.c_int
    lib.k20_host_len_ok.restype = ctypes.c_int
    lib.k20_host_len_ok.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.c_int32]
    lib.k20_host_len_run.restype = None
    return lib


def window_pairs(lib, from_lengths, to_lengths, thr, winkler):
    """how many pairs of these lengths the host-compiled length bound admits"""
    memo = {}
    n = 0
    for la in from_lengths:
        for lb in to_lengths:
            if (la, lb) not in memo:
                memo[la, lb] = lib.k20_host_len_ok(la, lb, thr, winkler)
            n += memo[la, lb]
    return n


@pytest.fixture(scope="module")
def host():
    return host_lib()


def _p(x):
    return x.ctypes.data_as(ctypes.c_void_p)


def _attained():
    """a handful of scores pairs DO attain, under either scorer, and the next float64 above each"""
    pairs = [("MARTHA", "MARHTA"), ("DWAYNE", "DUANE"), ("DIXON", "DICKSONX"), ("CRATE", "TRACE"), ("abab", "ababab"), ("ab", "abc")]
    got = sorted({f(a, b) for a, b in pairs for f in jaro_oracle.SCORERS.values()})
    assert len(got) >= 8 and all(0.0 < s < 1.0 for s in got)
    return got + [float(np.nextafter(s, 2.0)) for s in got]


def test_every_dismissal_is_safe_exhaustively(host):
    """all la, lb <= 24, all m <= min, all t-counts <= m / 2, every prefix the lengths allow, both scorers, the thresholds of
    THRESHOLDS and attained scores with their successors: where the length bound, m_need, the abandon rule at every split of
    flagged / remaining, or one of the two bounds behind the sweeps dismisses, jaro_score < t; the run the set-up launch finds is
    what the length bound admits; at t = 0 nothing is dismissed"""
    thr = np.array(list(THRESHOLDS) + _attained(), np.float64)
    dismissed = np.zeros(len(thr), np.int64)
    bad = host.k20_host_dismissals(24, len(thr), _p(thr), _p(dismissed))
    assert bad == 0
    assert dismissed[0] == 0                                                     # t = 0
    at = {t: int(d) for t, d in zip(thr.tolist(), dismissed.tolist())}
    assert 0 < at[0.5] < at[0.8] < at[0.9] < at[0.95] < at[1.0]                  # (the rules do dismiss, more the higher t)


def test_length_run_at_and_below_two_thirds(host):
    """Jaro at t <= 2/3: every non-empty to-length is inside (the bound is >= (0 + 1 + 1) / 3); above it, and under Winkler's
    step, the run is a proper window around la that holds la"""
    lo, hi = ctypes.c_int32(), ctypes.c_int32()
    for la in (1, 5, 40, 64, 200):
        for t in (0.5, TWO_THIRDS):
            host.k20_host_len_run(la, 1000, ctypes.c_double(t), 0, ctypes.byref(lo), ctypes.byref(hi))
            assert (lo.value, hi.value) == (1, 1000)
        for w in (0, 1):
            host.k20_host_len_run(la, 1000, ctypes.c_double(0.9), w, ctypes.byref(lo), ctypes.byref(hi))
            assert 1 <= lo.value <= la <= hi.value < 1000
            if la >= 40:
                # min / max >= 3t - 2 = 0.7 for Jaro; with four prefix characters (t - 0.4) / 0.6 stands for t: exactly 0.5
                assert (lo.value >= la // 2 and hi.value <= 2 * la) if w else (lo.value > 0.69 * la and hi.value < la / 0.69)
    for t, want in ((0.0, (0, 1000)), (0.5, (1, 0))):                           # an empty from-string: everything at 0, nothing above
        host.k20_host_len_run(0, 1000, ctypes.c_double(t), 1, ctypes.byref(lo), ctypes.byref(hi))
        assert (lo.value, hi.value) == want


def _symbols(strings, rank):
    off = np.zeros(len(strings) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in strings])
    return np.array([rank.get(c, 0) for s in strings for c in s] + [0], np.int32), off


def _dense_lists(word_bits):
    """dense random strings over 2 .. 4 letters: from-lengths 0 .. the word, to-lengths 0 .. 32 (32-bit class) or 0 .. 256"""
    rng = np.random.default_rng(200 + word_bits)
    mk = lambda alpha, lo, hi, n: ["".join(rng.choice(list(alpha), size=int(rng.integers(lo, hi + 1)))) for _ in range(n)]
    to_max = 32 if word_bits == 32 else 256
    fl = ["", "a"] + mk("ab", 1, word_bits, 40) + mk("abc", 1, word_bits, 30) + mk("abcd", word_bits - 2, word_bits, 20)
    tl = ["", "b"] + mk("ab", 1, to_max, 60) + mk("abc", 1, to_max, 40) + mk("abcd", 1, 64 if to_max > 64 else to_max, 30)
    tl += [s + "a" for s in fl[5:25] if len(s) < to_max] + [fl[30][:-1] + "b", fl[50], "ab" * (to_max // 2), "a" * to_max]
    assert max(map(len, fl)) == word_bits and max(map(len, tl)) == to_max
    return fl, tl


@pytest.mark.parametrize("word_bits", (32, 64))
def test_the_whole_decision_matches_the_definition_thresholded(host, oracle_mod, word_bits):
    """sweep 1 with the abandon rule once per packed dword (4 or 2 symbols), the bounds and the score, in both word widths: `hit`
    is the from-major definition >= t, a scored pair's score is the definition's, bit for bit -- and the rules do work: at 0.9
    fewer pairs pass each stage than the one before"""
    fl, tl = _dense_lists(word_bits)
    rank = {c: k + 1 for k, c in enumerate(sorted({c for s in tl for c in s}))}
    (a, a_off), (b, b_off) = _symbols(fl, rank), _symbols(tl, rank)
    for name, winkler in SCORERS:
        want = oracle_mod.jaro_matrix(fl, tl, name)
        np.testing.assert_array_equal(want[:6, :8], jaro_oracle.matrix(fl[:6], tl[:8], name))
        attained = float(np.sort(want[(want > 0.8) & (want < 1.0)])[3])
        for thr in THRESHOLDS + (attained, float(np.nextafter(attained, 2.0))):
            for per in (4, 2):
                hit, score = np.empty(want.shape, np.uint8), np.empty(want.shape, np.float64)
                stage = np.zeros(4, np.int64)
                rc = host.k20_host_pairs(word_bits, per, ctypes.c_int64(len(fl)), _p(a), _p(a_off), ctypes.c_int64(len(tl)), _p(b), _p(b_off),
                                         len(rank) + 1, winkler, ctypes.c_double(thr), _p(hit), _p(score), _p(stage))
                assert rc == 0
                np.testing.assert_array_equal(hit.astype(bool), want >= thr, err_msg=f"{name} t={thr!r} per={per}")
                scored = score >= 0.0
                np.testing.assert_array_equal(score[scored], want[scored])
                assert (scored | ~hit.astype(bool)).all() and int(scored.sum()) == stage[3]
                if thr == 0.0:
                    assert stage.tolist() == [want.size] * 4
                if thr == 0.9:
                    assert int(hit.sum()) <= stage[3] <= stage[2] < stage[1] < stage[0] < want.size and hit.sum() > 10
        assert ((want >= attained) != (want >= np.nextafter(attained, 2.0))).any()


def test_score_is_symmetric_bit_for_bit(oracle_mod):
    """score(a, b) and score(b, a) are the same float64: the self-join walks each unordered pair once, from either side"""
    rng = np.random.default_rng(220)
    mk = lambda alpha, lo, hi, n: ["".join(rng.choice(list(alpha), size=int(rng.integers(lo, hi + 1)))) for _ in range(n)]
    small = ["", "a", "ab", "ba"] + mk("ab", 1, 24, 40) + mk("abc", 1, 24, 30) + mk("abcd", 1, 40, 20)
    big = small + mk("ab", 1, 300, 150) + mk("abc", 30, 70, 150) + mk("abcd", 1, 64, 100)
    for name in jaro_oracle.SCORERS:
        m = jaro_oracle.matrix(small, small, name)
        np.testing.assert_array_equal(m, m.T)
        assert ((m > 0.7) & (m < 1.0)).sum() > 50
        m = oracle_mod.jaro_matrix(big, big, name)
        np.testing.assert_array_equal(m, m.T)


def _no_device(*a, **k):
    raise AssertionError("the device was reached")


def test_matcher_gates(monkeypatch):
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import EditDistance, JaroWinkler
    import polyfuzz_amd.models._jaro as mod
    monkeypatch.setattr(_lib.Context, "default", classmethod(_no_device))
    names = ["a", "b", "c"]
    for m in (JaroWinkler(), JaroWinkler(winkler=False)):
        for bad in (float("nan"), float("inf"), -float("inf"), -1e-300, np.nextafter(1.0, 2.0), 1.5, -0.1, "0.8", None, True, [0.8]):
            with pytest.raises(ValueError, match="min_similarity"):
                m.join(names, names, bad)
            with pytest.raises(ValueError, match="min_similarity"):
                m.join(names, min_similarity=bad)
            with pytest.raises(ValueError, match="min_similarity"):
                m.components(names, bad)
        for good in (0, 1, 0.0, 1.0, 0.8, np.float64(0.5), np.float32(0.25), np.int64(1)):      # accepted: the device is what stops these
            with pytest.raises(AssertionError, match="the device was reached"):
                m.join(names, names, good)
            with pytest.raises(AssertionError, match="the device was reached"):
                m.join(names)
            with pytest.raises(AssertionError, match="the device was reached"):
                m.components(names, good)
        assert not hasattr(m, "top_n") and "top_n" not in inspect.signature(JaroWinkler.__init__).parameters
    assert list(inspect.signature(JaroWinkler.__init__).parameters) == ["self", "winkler", "model_id", "normalize"]
    assert inspect.signature(JaroWinkler.join).parameters["min_similarity"].default == 0.9
    assert inspect.signature(JaroWinkler.components).parameters["min_similarity"].default == 0.9
    assert JaroWinkler()._scorer_name == "jaro_winkler" and JaroWinkler(False)._scorer_name == "jaro"
    assert JaroWinkler().components([], 0.9).tolist() == []

    # match delegates to EditDistance's, with the matcher's scorer and normalize
    seen = []

    def fake_match(self, from_list, to_list=None, **kwargs):
        seen.append((self._scorer_name, self.normalize, from_list, to_list, kwargs))
        return "the frame"
    monkeypatch.setattr(mod.EditDistance, "match", fake_match)
    assert mod.EditDistance is EditDistance
    assert JaroWinkler().match(names, ["x"], re_train=False) == "the frame"
    assert JaroWinkler(winkler=False, normalize=False).match(names) == "the frame"
    assert seen == [("jaro_winkler", True, names, ["x"], {"re_train": False}), ("jaro", False, names, None, {})]

    # the door of EditDistance stays shut
    for what in (lambda e: e.join(names, names, 0.9), lambda e: e.components(names, 0.9)):
        with pytest.raises(NotImplementedError):
            what(EditDistance(scorer="jaro_winkler"))


def test_entry_points_in_header_library_and_table():
    from polyfuzz_amd import _build, _lib
    if _build.is_stale():
        _build.build()
    header = open(os.path.join(REPO, "include", "polyfuzz_hip.h")).read()
    so = ctypes.CDLL(_lib.lib_path())
    for sym in ("pfz_jaro_join", "pfz_jaro_components"):
        assert f"int {sym}(" in header and hasattr(so, sym) and sym in _lib.SIGNATURES
    assert _lib.SIGNATURES["pfz_jaro_join"] == _lib.SIGNATURES["pfz_fuzz_join"]
    assert _lib.SIGNATURES["pfz_jaro_components"] == _lib.SIGNATURES["pfz_fuzz_components"]
    assert _lib.JARO_JOIN_COUNTERS == ("pairs_in_window", "pairs_alive_after_sweep1", "pairs_scored", "steps")
