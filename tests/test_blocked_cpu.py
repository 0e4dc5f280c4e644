"""BlockedEditDistance and K10 without a GPU: the constructor's scorer gate and argument checks, the refusals that must come before
any device call, pickling, the no-device error, the entry point in header / library / table, and k10_core.h's LCS (the one-word
and the multi-word form, compiled for the host) against oracle/indel.c."""
import ctypes
import os
import pickle
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

FIVE = ("ratio", "levenshtein", "osa", "jaro", "jaro_winkler")


def test_scorer_resolution():
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import BlockedEditDistance
    assert tuple(_lib.PAIR_SCORERS) == FIVE and [_lib.PAIR_SCORERS[s] for s in FIVE] == [0, 1, 2, 3, 4]
    for name in FIVE:
        assert BlockedEditDistance(scorer=name)._scorer_name == name
    for alias, name in (("jaro_similarity", "jaro"), ("jaro_winkler_similarity", "jaro_winkler"),
                        ("levenshtein_normalized_similarity", "levenshtein"), ("osa_normalized_similarity", "osa"), (None, "ratio")):
        assert BlockedEditDistance(scorer=alias)._scorer_name == name
    assert BlockedEditDistance()._scorer_name == "ratio"
    for bad in ("WRatio", "QRatio", "token_sort_ratio", "partial_ratio", "token_set_ratio", "nonsense", lambda a, b: 1.0, len):
        with pytest.raises(NotImplementedError):
            BlockedEditDistance(scorer=bad)


def test_argument_validation():
    from polyfuzz_amd.models import BlockedEditDistance
    m = BlockedEditDistance(scorer="osa", candidates=16, top_n=3, min_similarity=0.1, n_gram_range=(2, 3), clean_string=False,
                            remove_space_ngrams=False, normalize=False, model_id="b")
    assert (m.candidates, m.top_n, m.min_similarity, m.n_gram_range, m.clean_string, m.normalize) == (16, 3, 0.1, (2, 3), False, False)
    assert m.model_id == "b" and m.type == "BlockedEditDistance"
    t = m._tfidf
    assert (t.top_n, t.min_similarity, t.n_gram_range, t.clean_string, t.remove_space_ngrams) == (16, 0.1, (2, 3), False, False)
    assert BlockedEditDistance(candidates=np.int64(8), top_n=np.int32(8)).candidates == 8
    for kw in ({"candidates": 0}, {"candidates": 2.0}, {"candidates": True}, {"candidates": "8"}, {"top_n": 0}, {"top_n": -1}, {"top_n": 1.5},
               {"top_n": None}, {"top_n": 33}, {"candidates": 4, "top_n": 5}, {"min_similarity": "0.5"}, {"min_similarity": None},
               {"n_gram_range": 3}, {"n_gram_range": (3,)}, {"n_gram_range": (3, 2)}, {"n_gram_range": (0, 2)}, {"n_gram_range": (1.0, 2)}):
        with pytest.raises(ValueError):
            BlockedEditDistance(**kw)


@pytest.mark.parametrize("kw,limit", [({"candidates": 100, "top_n": 65}, "64"), ({"candidates": 1025, "top_n": 1}, "1024")])
def test_limits_are_refused_before_any_device_call(monkeypatch, kw, limit):
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import BlockedEditDistance

    def no_device(*a, **k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(_lib.Context, "default", classmethod(no_device))
    m = BlockedEditDistance(scorer="jaro", **kw)          # (the constructor alone does not raise)
    names = [f"name {k:04d}" for k in range(1100)]
    with pytest.raises(_lib.PfzUnsupported, match=limit):
        m.match(names[:3], names)
    with pytest.raises(_lib.PfzUnsupported, match=limit):
        m.match(names)
    # clipped to the distinct to-strings first (reference _utils.py:54-56): 40 of them are within both limits, the device is next
    with pytest.raises(AssertionError, match="the device was reached"):
        m.match(names[:3], names[:40])


def test_pickling_round_trip():
    from polyfuzz_amd.models import BlockedEditDistance
    m = BlockedEditDistance(scorer="jaro_winkler_similarity", candidates=12, top_n=4, normalize=False, model_id="x")
    m._to_dev, m._to_names = object(), ("a",)             # what a match leaves: stays behind
    c = pickle.loads(pickle.dumps(m))
    assert c._to_dev is None and c._to_names is None
    assert (c._scorer_name, c.scorer, c.candidates, c.top_n, c.normalize, c.model_id) == ("jaro_winkler", "jaro_winkler_similarity", 12, 4, False, "x")
    assert c._tfidf.top_n == 12 and c._tfidf._dev_vec is None


def test_no_device_no_fallback():
    import polyfuzz_amd
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import BlockedEditDistance
    if polyfuzz_amd.device_count() > 0:
        pytest.skip("a GPU is visible: the no-device failure path cannot be exercised")
    for name in FIVE:
        with pytest.raises(_lib.PfzNoDevice):
            BlockedEditDistance(scorer=name).match(["apple"], ["apples"])


def test_entry_point_in_header_library_and_table():
    from polyfuzz_amd import _lib
    with open(os.path.join(REPO, "include", "polyfuzz_hip.h")) as f:
        header = f.read()
    assert "int pfz_pairs_rescore_topn(" in header
    for k, name in enumerate(("RATIO", "LEVENSHTEIN", "OSA", "JARO", "JARO_WINKLER")):
        assert f"#define PFZ_PAIR_{name} {k}\n" in header
    assert "pfz_pairs_rescore_topn" in _lib.SIGNATURES and hasattr(_lib.load(), "pfz_pairs_rescore_topn")


# ---- k10_core.h on the host ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host():
    so = os.path.join(REPO, "oracle", "_build", "k10_core_host.so")
    src = [os.path.join(HERE, "k10_core_host.cpp"), os.path.join(REPO, "polyfuzz_amd", "csrc", "k10_core.h")]
    os.makedirs(os.path.dirname(so), exist_ok=True)
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", src[0], "-o", so])
    lib = ctypes.CDLL(so)
    lib.k10_host_lcs.restype = ctypes.c_int
    lib.k10_host_lcs.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.k10_host_ratio.restype = ctypes.c_double
    lib.k10_host_ratio.argtypes = [ctypes.c_int, ctypes.c_longlong]
    return lib


def _codes(s):
    return np.frombuffer(s.encode("utf-32-le", "surrogatepass"), np.uint32).astype(np.int32)


def test_lcs_and_ratio_match_the_oracle(host, oracle_mod):
    """random pairs over 2 and 9 letters, from-lengths on both sides of every word border (one 32-bit word, one 64-bit word, up to
    five 64-bit words), to-lengths 0 .. 300: ratio_of(LCS, |a| + |b|) of every mode that takes the from-string == oracle/indel.c's
    float64 ratio, and the modes agree on the LCS"""
    rng = np.random.default_rng(1010)
    mk = lambda alpha, n: "".join(alpha[i] for i in rng.integers(0, len(alpha), n))
    fl, tl = [], []
    for alpha in ("ab", "abcdefgh "):
        fl += [mk(alpha, n) for n in (0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 300)] + [mk(alpha, int(n)) for n in rng.integers(1, 70, 20)]
        tl += [mk(alpha, n) for n in (0, 1, 32, 33, 64, 65, 128, 129, 300)] + [mk(alpha, int(n)) for n in rng.integers(1, 140, 30)]
    fl.append("naïve café Ωmega \U0001f600 smile")
    tl.append("naive cafe Ωmega \U0001f601 smile \U0001f600")
    want = oracle_mod.indel_argmax(fl, tl, want_matrix=True)[2]
    fc, tc = [_codes(s) for s in fl], [_codes(s) for s in tl]
    seen = {0: 0, 1: 0, 2: 0}
    for i, a in enumerate(fc):
        for j, b in enumerate(tc):
            got = {}
            for mode in (0, 1, 2):
                lcs = host.k10_host_lcs(a.ctypes.data, len(a), b.ctypes.data, len(b), mode)
                if lcs < 0:
                    assert len(a) > (32, 64)[mode]
                    continue
                got[mode] = lcs
                seen[mode] += 1
                assert host.k10_host_ratio(lcs, len(a) + len(b)) == want[i, j], (fl[i], tl[j], mode, lcs)
            assert len(set(got.values())) == 1 and 2 in got
    assert min(seen.values()) > 1000
    assert host.k10_host_ratio(0, 0) == 100.0 and want[fl.index(""), tl.index("")] == 100.0      # two empty strings
