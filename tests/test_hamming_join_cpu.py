"""K23 without a GPU: the distance a similarity stands for (the rule evaluated, against numpy), the score of a distance, the cases
file's constants against its generator, Hamming's gates before any device call, the pinned refusal of Embeddings.join, the
kernels' register / LDS budgets and the three new symbols."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

from tests import hamming_join_cases as HJ

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WIDTHS = (1, 8, 40, 64, 96, 100, 768, 1000, 4104, 2 ** 24 - 1)


def _no_device(*a, **k):
    raise AssertionError("the device was reached")


def _rule_many(d, ts):
    """rule_max_distance for many thresholds at once: the scores fall with h, so the passing h are a prefix"""
    h = np.arange(d + 1, dtype=np.float32)            # (exact: d < 2**24)
    s = -((np.float32(d) - np.float32(2) * h) / np.float32(d)).astype(np.float64)
    assert s.dtype == np.float64 and (s[1:] >= s[:-1]).all()
    return np.searchsorted(s, -np.asarray(ts, np.float64), side="right") - 1


def _thresholds(d, rng):
    h = np.arange(min(d, 300) + 1, dtype=np.int64)
    own = ((np.float32(d) - np.float32(2) * h.astype(np.float32)) / np.float32(d)).astype(np.float64)      # every score value (of small d)
    ts = np.concatenate([rng.random(2000), own, np.nextafter(own, 2.0), np.nextafter(own, -2.0), [0.0, 1.0, 0.6, 0.7, 0.8, 0.9, 0.95]])
    return ts[(ts >= 0.0) & (ts <= 1.0)]


@pytest.mark.parametrize("d", WIDTHS)
def test_max_distance_is_the_rule_evaluated(d):
    from polyfuzz_amd import _lib
    ts = _thresholds(d, np.random.default_rng(23 + d % 1000))
    want = _rule_many(d, ts)
    assert len(ts) > 2000 and want.min() >= 0
    for t, w in zip(ts.tolist(), want.tolist()):
        got = _lib.hamming_max_distance(d, t)
        assert got == w, (d, t, got, w)
    if d <= 4104:                                    # the prefix search against the plain evaluation of the cases file
        for t in ts[::97].tolist() + [0.0, 1.0]:
            assert HJ.rule_max_distance(d, t) == _lib.hamming_max_distance(d, t), (d, t)
    assert _lib.hamming_max_distance(d, 0.0) >= d // 2 and _lib.hamming_max_distance(d, 1.0) == 0
    assert _lib.hamming_max_distance(np.int64(d), np.float32(0.5)) == _lib.hamming_max_distance(d, 0.5)


def test_max_distance_where_the_closed_form_is_wrong():
    from polyfuzz_amd import _lib
    for d, t, rule, closed in ((40, 0.8, 4, 3), (40, 0.7, 5, 6), (100, 0.8, 10, 9), (1000, 0.95, 24, 25)):
        assert int(np.floor((1 - t) / 2 * d)) == closed != rule
        assert _lib.hamming_max_distance(d, t) == rule == HJ.rule_max_distance(d, t), (d, t)
    for name in HJ.CASES:
        for t in HJ.THRESHOLDS:
            assert _lib.hamming_max_distance(HJ.bits(name), t) == HJ.HMAX[name][t], (name, t)


def test_max_distance_refusals():
    from polyfuzz_amd import _lib
    for bad in (float("nan"), -1e-300, np.nextafter(1.0, 2.0), 1.5, -0.1, float("inf"), "0.8", None, True):
        with pytest.raises(ValueError, match="min_similarity"):
            _lib.hamming_max_distance(64, bad)
    for bad in (0, -1, 2 ** 24, 2 ** 40, 64.0, True, None):
        with pytest.raises(ValueError, match="dim_bits"):
            _lib.hamming_max_distance(bad, 0.8)
    # the library's own gate, behind the binding's
    lib, out = _lib.load(), ctypes.c_int64(7)
    for d, t in ((0, 0.8), (2 ** 24, 0.8), (64, float("nan")), (64, 1.5), (64, -0.5)):
        assert lib.pfz_hamming_max_distance(d, t, ctypes.byref(out)) == -1 and out.value == 7, (d, t)      # PFZ_ERR_INVALID
    assert lib.pfz_hamming_max_distance(64, 0.8, None) == -1
    assert lib.pfz_hamming_max_distance(2 ** 24 - 1, 0.8, ctypes.byref(out)) == 0 and out.value == _rule_many(2 ** 24 - 1, [0.8])[0]


def test_similarity_bits_are_the_panel_oracles():
    from polyfuzz_amd import _lib
    from tests.test_hamming_cpu import scores
    rng = np.random.default_rng(5)
    for d in (8, 40, 64, 96, 768, 4104):
        a = rng.integers(0, 256, (9, d // 8), dtype=np.uint8)
        b = rng.integers(0, 256, (11, d // 8), dtype=np.uint8)
        b[0], b[1] = a[0], ~a[1]                      # h = 0 and h = d
        want = scores(a, b, d)
        got = _lib.hamming_similarity(HJ.distances_of(a, b), d)
        assert got.dtype == np.float32 == want.dtype and got.tobytes() == want.tobytes(), d
        assert got[0, 0] == 1.0 and got[1, 1] == -1.0
    every = _lib.hamming_similarity(np.arange(1001, dtype=np.int32), 1000)
    assert every.tobytes() == ((1000 - 2 * np.arange(1001)).astype(np.float32) / np.float32(1000)).tobytes()
    assert _lib.hamming_similarity(np.empty(0, np.int32), 64).shape == (0,)


def test_case_constants_are_the_oracle_on_the_generator():
    x = HJ.gen(5, 16, 2, 1)
    rng = np.random.default_rng(1)                    # the generator draws base, lab, noise in that order
    base = rng.integers(0, 2, (2, 16), dtype=np.uint8)
    lab = rng.integers(0, 2, 5)
    assert x.tobytes() == np.packbits(base[lab] ^ (rng.random((5, 16)) < 0.05), axis=1).tobytes() and x.dtype == np.uint8
    for name in HJ.CASES:
        f, to = HJ.lists(name)
        assert f.shape[1] * 8 >= HJ.bits(name) > f.shape[1] * 8 - 8 and (to is None) == (name in HJ.SELF_CASES)
        for t in HJ.THRESHOLDS:
            assert HJ.oracle_counts(name, t) == (HJ.HMAX[name][t],) + HJ.ORACLE_HITS[name][t], (name, t)
            if name in HJ.SELF_CASES:
                assert HJ.oracle_components(name, t) == HJ.ORACLE_COMPONENTS[name][t], (name, t)
    assert HJ.lists("130x4104")[0].shape == (130, 513) and HJ.lists(HJ.TWO_LIST_CASE)[1].shape == (1000, 96)
    assert sum(HJ.ORACLE_HITS[n][t][1] for n in HJ.CASES for t in HJ.THRESHOLDS) > 1000      # pairs exactly on a cutoff
    assert [n for n in HJ.CASES for t in HJ.THRESHOLDS if HJ.ORACLE_HITS[n][t][0] == 0] == ["130x4104", "200x1000"]


def _codes():
    return ["a", "b", "c"], np.eye(3, 8, dtype=np.uint8)


def test_exactly_one_threshold(monkeypatch):
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import Hamming
    monkeypatch.setattr(_lib.Context, "default", classmethod(_no_device))
    names, x = _codes()
    m = Hamming()
    assert m.type == "Embeddings"
    for kw in ({}, {"min_similarity": 0.8, "max_distance": 3}):
        with pytest.raises(ValueError, match="exactly one of min_similarity and max_distance"):
            m.join(names, embeddings_from=x, **kw)
        with pytest.raises(ValueError, match="exactly one of min_similarity and max_distance"):
            m.join(names, names, embeddings_from=x, embeddings_to=x, **kw)
        with pytest.raises(ValueError, match="exactly one of min_similarity and max_distance"):
            m.components(names, embeddings=x, **kw)
    for bad in (True, False, -1, 65, 3.0, "3", np.float32(2), [3]):
        with pytest.raises(ValueError, match="max_distance"):
            m.join(names, embeddings_from=x, max_distance=bad)
        with pytest.raises(ValueError, match="max_distance"):
            m.components(names, embeddings=x, max_distance=bad)
    for bad in (float("nan"), 1.5, -0.1, "0.8", True):
        with pytest.raises(ValueError, match="min_similarity"):
            m.join(names, min_similarity=bad, embeddings_from=x)
        with pytest.raises(ValueError, match="min_similarity"):
            m.components(names, bad, embeddings=x)
    for good in ({"max_distance": 0}, {"max_distance": 64}, {"max_distance": np.int64(3)}, {"min_similarity": 0.9},
                 {"min_similarity": 0}, {"min_similarity": np.float32(1.0)}):      # accepted: the device is what stops these
        with pytest.raises(AssertionError, match="the device was reached"):
            m.join(names, embeddings_from=x, **good)
        with pytest.raises(AssertionError, match="the device was reached"):
            m.join(names, names, embeddings_from=x, embeddings_to=x.view(np.int8), **good)
        with pytest.raises(AssertionError, match="the device was reached"):
            m.components(names, embeddings=x, **good)
    with pytest.raises(AssertionError, match="the device was reached"):
        m.components(names, 0.9, x)                  # (the positional order linkage.connected_components uses)


def test_codes_are_required_and_checked(monkeypatch):
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import Hamming
    monkeypatch.setattr(_lib.Context, "default", classmethod(_no_device))
    names, x = _codes()
    m = Hamming(model_id="h")
    assert m.model_id == "h"
    with pytest.raises(ValueError, match="embeddings_from is required"):
        m.join(names, max_distance=3)
    with pytest.raises(ValueError, match="embeddings_to is required"):
        m.join(names, names, max_distance=3, embeddings_from=x)
    with pytest.raises(ValueError, match="embeddings is required"):
        m.components(names, 0.9)
    with pytest.raises(ValueError, match="embeddings_to is given without a to_list"):
        m.join(names, max_distance=3, embeddings_from=x, embeddings_to=x)
    with pytest.raises(ValueError, match="shape"):
        m.join(names, max_distance=3, embeddings_from=x[:2])
    with pytest.raises(ValueError, match="shape"):
        m.join(names, names[:2], max_distance=3, embeddings_from=x, embeddings_to=x)
    with pytest.raises(ValueError, match="shape"):
        m.components(names, max_distance=3, embeddings=x[0])
    with pytest.raises(ValueError, match="equal width"):
        m.join(names, names, max_distance=3, embeddings_from=x, embeddings_to=x[:, :4])
    with pytest.raises(ValueError, match="equal width"):      # 8 packed bytes are 64 bits, 8 floats are 8
        m.join(names, names, max_distance=3, embeddings_from=x, embeddings_to=x.astype(np.float32))
    with pytest.raises(ValueError, match="packed uint8 / int8 rows or a float array"):
        m.join(names, max_distance=3, embeddings_from=x.astype(np.int32))
    assert list(inspect.signature(Hamming.__init__).parameters) == ["self", "model_id"]
    p = inspect.signature(Hamming.join).parameters
    assert list(p) == ["self", "from_list", "to_list", "min_similarity", "embeddings_from", "embeddings_to", "max_distance"]
    assert p["max_distance"].kind is inspect.Parameter.KEYWORD_ONLY and p["min_similarity"].default is None is p["max_distance"].default
    p = inspect.signature(Hamming.components).parameters
    assert list(p) == ["self", "strings", "min_similarity", "embeddings", "max_distance"]
    assert p["max_distance"].kind is inspect.Parameter.KEYWORD_ONLY and p["min_similarity"].default is None
    p = inspect.signature(Hamming.match).parameters
    assert list(p) == ["self", "from_list", "to_list", "embeddings_from", "embeddings_to", "top_n"] and p["top_n"].default == 1
    import polyfuzz_amd.models as models
    assert "Hamming" in models.__all__ and models.Hamming is Hamming


def test_match_delegates_to_embeddings(monkeypatch):
    from polyfuzz_amd.models import Embeddings, Hamming
    calls = []

    def fake(self, from_list, to_list=None, embeddings_from=None, embeddings_to=None, re_train=True):
        calls.append((self, from_list, to_list, embeddings_from, embeddings_to))
        return "frame"
    monkeypatch.setattr(Embeddings, "match", fake)
    names, x = _codes()
    assert Hamming().match(names, names[:2], x, x[:2], top_n=3) == "frame"
    assert Hamming().match(names, embeddings_from=x) == "frame"
    (e, fl, tl, ef, et), second = calls[0], calls[1]
    assert isinstance(e, Embeddings) and e.binary == "ubinary" and e.top_n == 3 and e.cosine_method == "hip"
    assert e.precision is None and e.compute_dtype is None and e.rescore_multiplier is None
    assert fl is names and tl == names[:2] and ef is x and et.tobytes() == x[:2].tobytes()
    assert second[0].top_n == 1 and second[2] is None and second[4] is None


def test_connected_components_hands_on_the_codes(monkeypatch):
    from polyfuzz_amd import _lib, linkage
    from polyfuzz_amd.models import Hamming
    names, x = _codes()
    seen = []

    def fake(ctx, dev, max_distance, counters=False):
        seen.append((dev, max_distance))
        return np.array([0, 0, 2], np.int32), 1, 2
    monkeypatch.setattr(_lib.Context, "default", classmethod(lambda cls: "ctx"))
    monkeypatch.setattr(_lib.DeviceDense, "upload_bits", classmethod(lambda cls, ctx, vec, normalize=True: ("handle", vec)))
    monkeypatch.setattr(_lib, "hamming_components", fake)
    m = Hamming()
    assert linkage.connected_components(names, m, 0.9, embeddings=x) == linkage.dicts_from_labels(names, [0, 0, 2])
    assert seen[0][0][1] is x and seen[0][1] == _lib.hamming_max_distance(64, 0.9) == 3 and m.last_counts == {"pairs": 1, "components": 2}
    assert "Hamming" in linkage.connected_components.__doc__


def test_binding_refuses_other_operands_without_a_library_call():
    from polyfuzz_amd import _lib

    class Dev:
        n, h, dim = 3, None, 64
    ok = Dev()
    ok.dtype = _lib.BINARY
    for dtype in ("float32", "int8", "float16", "bfloat16"):
        d = Dev()
        d.dtype = dtype
        with pytest.raises(ValueError, match="binary operands only") as e:
            _lib.hamming_join(None, d, None, 3)
        assert dtype in str(e.value) and not isinstance(e.value, _lib.PfzError)
        with pytest.raises(ValueError, match="binary operands only"):
            _lib.hamming_join(None, ok, d, 3)
        with pytest.raises(ValueError, match="binary operands only"):
            _lib.hamming_components(None, d, 3)
    assert _lib.HAMMING_JOIN_COUNTERS == ("tiles", "hit_waves")
    for f, names in ((_lib.hamming_join, ["ctx", "from_dev", "to_dev", "max_distance", "capacity", "counters"]),
                     (_lib.hamming_components, ["ctx", "dev", "max_distance", "counters"]),
                     (_lib.hamming_max_distance, ["dim_bits", "min_similarity"]), (_lib.hamming_similarity, ["dist", "dim_bits"])):
        assert list(inspect.signature(f).parameters) == names


def test_embeddings_join_still_refuses_binary(monkeypatch):
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import Embeddings
    monkeypatch.setattr(_lib.Context, "default", classmethod(_no_device))
    names, x = _codes()
    m = Embeddings()
    m.binary = "ubinary"
    with pytest.raises(ValueError, match="binary"):
        m.join(names, min_similarity=0.8, embeddings_from=x)
    with pytest.raises(ValueError, match="binary"):
        m.components(names, 0.8, embeddings=x)


def test_kernel_budget():
    """k23_join_kernel and k23_comp_kernel exist once each and fit TWO workgroups per CU, as their __launch_bounds__(256, 2) says:
    no scratch, the main loop's 36 864 B of LDS and nothing else, at most 128 registers per lane.  k5_hamming_panel is still
    there under its name, with the LDS and the scratch it had before its main loop became k5_hamming_loop."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_budget
    from polyfuzz_amd import _build
    for exe in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(kernel_budget.LLVM, exe)):
            pytest.skip(f"{exe} not in {kernel_budget.LLVM}")
    md = kernel_budget.kernel_metadata(_build.build())
    pretty = dict(zip(md, kernel_budget.demangled(list(md))))
    for name in ("k23_join_kernel", "k23_comp_kernel"):
        hits = [v for k, v in md.items() if pretty[k].startswith(f"pfz::{name}(")]
        assert len(hits) == 1, (name, [p for p in pretty.values() if "k23_" in p])
        k = hits[0]
        assert k["scratch"] == 0, (name, k)
        assert k["lds"] == 2 * 128 * 36 * 4 == 36864, (name, k)
        assert k["vgpr"] + k.get("agpr", 0) <= 128, (name, k)
    panel = [v for k, v in md.items() if pretty[k].startswith("pfz::k5_hamming_panel(")]
    assert len(panel) == 1 and (panel[0]["lds"], panel[0]["scratch"]) == (36864, 0), panel
    assert panel[0]["vgpr"] + panel[0].get("agpr", 0) <= 128, panel      # (122 before and after: cleared inside the loop function, h cost it 185)


def test_symbols_declared_exported_and_in_the_table():
    from polyfuzz_amd import _build, _lib
    if _build.is_stale():
        _build.build()
    header = open(os.path.join(REPO, "include", "polyfuzz_hip.h")).read()
    so = ctypes.CDLL(_lib.lib_path())
    for name, n_args in (("pfz_hamming_join", 10), ("pfz_hamming_components", 7), ("pfz_hamming_max_distance", 3)):
        assert f"int {name}(" in header and hasattr(so, name) and name in _lib.SIGNATURES
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == n_args
        decl = header[header.index(f"int {name}("):]
        assert len(decl[:decl.index(";")].split(",")) == n_args
    assert _lib.SIGNATURES["pfz_hamming_join"][1][3] is ctypes.c_int64 and _lib.SIGNATURES["pfz_hamming_max_distance"][1][1] is ctypes.c_double
    doc = " ".join(header[header.index("---- K23"):header.index("int pfz_hamming_max_distance(")].replace(" * ", " ").split())
    for phrase in ("k23_join", "k23_sort_unpack", "k23_components", "never (i, i)", "PFZ_ERR_UNSUPPORTED", "PFZ_ERR_INVALID",
                   "max_distance outside [0, dim_bits]", "do not read the handles' `normalize`", "not by a closed form"):
        assert phrase in doc, phrase
    blob = open(_build.LIB_PATH, "rb").read()
    assert b"k23_join_kernel" in blob and b"k23_comp_kernel" in blob and b"k5_hamming_panel" in blob
