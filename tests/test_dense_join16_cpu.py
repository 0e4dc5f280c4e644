"""K22 without a GPU: the four entry points in header, library and ctypes table, the header's contract, the margin function and the
search threshold, the rounding term of the margin held on numpy-emulated 16-bit rows, the gates of Embeddings.search_dtype with
the device stubbed, and the kernels' register / LDS budgets."""
import ctypes
import inspect
import math
import os
import pickle
import sys

import numpy as np
import pytest

from tests import dense_join16_cases as C
from tests import dense_join_cases as DJ

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pfz_dense_derive16", "pfz_dense_search_margin", "pfz_dense_join16", "pfz_dense_components16")


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
    for name in ENTRIES:
        assert f"int {name}(" in header and hasattr(so, name) and name in _lib.SIGNATURES, name
    assert _arg_names(header, "pfz_dense_join16") == ["ctx", "from16", "to16", "from32", "to32", "min_similarity", "capacity",
                                                      "cand_capacity", "out_row_ptr", "out_idx", "out_sim", "out_total", "out_counters"]
    assert _arg_names(header, "pfz_dense_components16") == ["ctx", "v16", "v32", "min_similarity", "cand_capacity", "out_label",
                                                            "out_pairs", "out_components", "out_counters"]
    assert _arg_names(header, "pfz_dense_derive16") == ["ctx", "exact", "dtype", "out"]
    assert _arg_names(header, "pfz_dense_search_margin") == ["dtype", "ld", "out_eps"]
    for name in ENTRIES:
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(_arg_names(header, name)), name
    assert _lib.SIGNATURES["pfz_dense_join16"][1][5] is ctypes.c_double and _lib.SIGNATURES["pfz_dense_components16"][1][3] is ctypes.c_double
    assert _lib.DENSE_JOIN16_COUNTERS == ("tiles", "hit_corners", "candidates")
    assert list(inspect.signature(_lib.dense_join16).parameters) == ["ctx", "from16", "to16", "from_exact", "to_exact", "min_similarity",
                                                                      "capacity", "counters", "cand_capacity"]
    assert list(inspect.signature(_lib.dense_components16).parameters)[:4] == ["ctx", "dev16", "dev_exact", "min_similarity"]
    assert callable(_lib.DeviceDense.derive16) and callable(_lib.dense_search_margin)


def test_header_carries_the_contract_the_formula_and_the_assumption():
    header = _header()
    doc = header[header.index("---- K22"):header.index("int pfz_dense_components16(")]
    doc = " ".join(doc.replace(" * ", " ").split())
    for phrase in ("*out_total is always the exact number of hits", "returns PFZ_OK, has written NONE of the three output arrays",
                   "repeated with capacity >= *out_total", "ascending within a row", "same call gives the same bytes", "never (i, i)",
                   "2^31 tiles", "fewer than 2^31 rows", "PFZ_ERR_UNSUPPORTED", "PFZ_ERR_INVALID", "int64[3]",
                   "eps = 2 asin(u + 2^-24 + sqrt(ld) 2^-25) + (ld + 8) 2^-23", "u = 2^-8 for bfloat16", "u = 2^-11 for float16",
                   "largest float32 <= min_similarity - eps", "assumption", "two runs at most", "O(candidates)",
                   "from32 == NULL", "bit for bit", "symmetric", "k22_search", "k22_rescore", "k22_sort_unpack"):
        assert phrase in doc, phrase


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_margin_equals_the_formula(dtype):
    from polyfuzz_amd import _lib
    u = {"bfloat16": 2.0 ** -8, "float16": 2.0 ** -11}[dtype]
    for ld in (64, 768, 4096, 131072):
        want = 2.0 * math.asin(u + 2.0 ** -24 + math.sqrt(ld) * 2.0 ** -25) + (ld + 8) * 2.0 ** -23
        got = _lib.dense_search_margin(dtype, ld)
        assert isinstance(got, float) and got == want == C.margin(dtype, ld), (dtype, ld, got, want)
    assert 0.0078 < _lib.dense_search_margin("bfloat16", 768) < 0.0080 and 0.0010 < _lib.dense_search_margin("float16", 768) < 0.0011
    for bad in ("float32", "int8", None):
        with pytest.raises(ValueError, match="search types"):
            _lib.dense_search_margin(bad, 64)
    eps = ctypes.c_double(-1.0)
    so = ctypes.CDLL(_lib.lib_path())
    so.pfz_dense_search_margin.argtypes = _lib.SIGNATURES["pfz_dense_search_margin"][1]
    assert so.pfz_dense_search_margin(0, 64, ctypes.byref(eps)) == -1 and eps.value == -1.0          # PFZ_ERR_INVALID: fp32 is no search type
    assert so.pfz_dense_search_margin(2, 0, ctypes.byref(eps)) == -1


def test_search_threshold32_is_the_largest_float32_at_or_below_t_minus_eps():
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(22)
    f32 = rng.random(2000).astype(np.float32)
    for dtype, ld in (("bfloat16", 768), ("float16", 64), ("bfloat16", 131072)):
        eps = _lib.dense_search_margin(dtype, ld)
        ts = np.concatenate([rng.random(5000), f32.astype(np.float64) + eps, np.nextafter(f32.astype(np.float64) + eps, 2.0),
                             np.nextafter(f32.astype(np.float64) + eps, -1.0), [0.0, 1.0, 0.6, 0.8, 0.9, eps]])
        ts = ts[(ts >= 0.0) & (ts <= 1.0)]
        for t in ts.tolist():
            r = _lib.dense_search_threshold32(t, eps)
            assert isinstance(r, np.float32)
            assert np.float64(r) <= t - eps < np.float64(np.nextafter(r, np.float32(np.inf))), (t, eps, r)
    assert _lib.dense_search_threshold32(0.0, 0.25) == np.float32(-0.25)                      # t < eps: every score is a candidate
    assert _lib.dense_search_threshold32(0.8, 0.0) <= _lib.dense_threshold32(0.8)


ROWS = 96


def _row_sets(dtype, d):
    """name -> float32 rows of width d: Gaussian, clustered (the K14 tests' generator), half-ulp adversarial; the float16 sets have
    values below 2^-14 in the unit vector"""
    tiny = d // 4 if dtype == "float16" else 0
    sets = {"gaussian": C.gaussian_rows(ROWS, d, 1000 + d, tiny), "clustered": DJ.gen(ROWS, d, 6, 2000 + d),
            "half_ulp": C.half_ulp_rows(ROWS, d, dtype, 3000 + d, tiny)}
    if tiny:
        for name in ("gaussian", "half_ulp"):
            unit = sets[name] * C.inv_norm32(sets[name])[:, None]
            assert 0 < np.abs(unit[unit != 0]).min() < 2.0 ** -14 and (np.abs(unit) < 2.0 ** -14).mean() > 0.2, name
    return sets


@pytest.mark.parametrize("d", [32, 64, 768])
@pytest.mark.parametrize("dtype", C.DTYPES)
def test_rounding_moves_a_cosine_by_less_than_the_first_term(dtype, d):
    """max |cos(rounded a, rounded b) - cos(a, b)| in float64 over all pairs of each row set stays below 2 asin(u + 2^-24 +
    sqrt(ld) 2^-25): the bound is derived (a relative rounding u turns a vector by at most asin(u)), this holds it on the rows
    that come nearest"""
    bound = C.rounding_term(dtype, C.padded(d))
    for name, x in _row_sets(dtype, d).items():
        r = C.search_copy(x, dtype)
        assert np.isfinite(r).all() and np.abs(r).max() <= 1.0
        if name == "half_ulp":                             # the rows are what they claim: rounding moves nearly every value by ~ half an ulp
            pre = (x * C.inv_norm32(x)[:, None]).astype(np.float64)
            rel = np.abs(r - pre) / np.maximum(np.abs(pre), 2.0 ** -14 if dtype == "float16" else 0.0)
            assert np.median(rel) > 0.25 * C.U[dtype], (dtype, d, np.median(rel))
        worst = np.abs(C.cosines64(r, r) - C.cosines64(x, x)).max()
        print(f"{dtype} d={d} {name}: worst |cos(rounded) - cos(exact)| {worst:.3e} = {worst / bound:.3f} of the first term {bound:.3e}")
        assert 0 < worst < bound, (dtype, d, name, worst, bound)


class _Dev:
    def __init__(self, log, what):
        self.log, self.what, self.n = log, what, 3

    def derive16(self, dtype):
        self.log.append(("derive16", self.what, dtype))
        return _Dev(self.log, self.what + "16")


def _stub_device(monkeypatch):
    """the device behind Embeddings.join / .components replaced by recorders: log of (call, ...)"""
    from polyfuzz_amd import _lib
    log = []
    monkeypatch.setattr(_lib.Context, "default", classmethod(lambda cls: "ctx"))
    monkeypatch.setattr(_lib.DeviceDense, "upload", classmethod(lambda cls, ctx, vec, normalize=True, compute_dtype=None:
                                                                (log.append(("upload", len(vec))), _Dev(log, "f32"))[1]))
    empty = (np.zeros(4, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
    monkeypatch.setattr(_lib, "dense_join", lambda ctx, f, t, ms, **k: (log.append(("k14_join", f.what, t and t.what)), empty + ({"pairs": 0},))[1])
    monkeypatch.setattr(_lib, "dense_components", lambda ctx, d, ms, **k: (log.append(("k14_components", d.what)),
                                                                          (np.arange(3, dtype=np.int32), 0, 3))[1])
    monkeypatch.setattr(_lib, "dense_join16", lambda ctx, f16, t16, f, t, ms, **k: (
        log.append(("k22_join", f16.what, t16 and t16.what, f.what, t and t.what)), empty + ({"pairs": 0, "candidates": 5},))[1])
    monkeypatch.setattr(_lib, "dense_components16", lambda ctx, d16, d, ms, **k: (
        log.append(("k22_components", d16.what, d.what)), (np.arange(3, dtype=np.int32), 0, 3, {"tiles": 1, "hit_corners": 0, "candidates": 7}))[1])
    return log


def _vectors():
    return ["a", "b", "c"], np.eye(3, 8, dtype=np.float32)


def test_search_dtype_is_validated_when_assigned():
    from polyfuzz_amd.models import Embeddings
    m = Embeddings()
    assert m.search_dtype is None
    for good in ("bfloat16", "float16", None):
        m.search_dtype = good
        assert m.search_dtype == good
    for bad in ("float32", "int8", "bf16", "binary", 16, True, ""):
        with pytest.raises(ValueError, match="search_dtype"):
            m.search_dtype = bad
    assert m.search_dtype is None
    assert "search_dtype" in Embeddings.__doc__ and "search_dtype" in Embeddings.join.__doc__ and "O(candidates)" in Embeddings.components.__doc__
    assert list(inspect.signature(Embeddings.join).parameters) == ["self", "from_list", "to_list", "min_similarity", "embeddings_from",
                                                                    "embeddings_to"]
    assert list(inspect.signature(Embeddings.components).parameters) == ["self", "strings", "min_similarity", "embeddings"]


def test_match_refuses_search_dtype_and_points_at_its_own_route(monkeypatch):
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import Embeddings
    monkeypatch.setattr(_lib.Context, "default", classmethod(_no_device))
    names, x = _vectors()
    m = Embeddings()
    m.search_dtype = "bfloat16"
    with pytest.raises(ValueError, match="search_dtype") as e:
        m.match(names, names, embeddings_from=x, embeddings_to=x)
    assert "compute_dtype" in str(e.value) and "rescore_multiplier" in str(e.value) and not isinstance(e.value, _lib.PfzError)
    m.search_dtype = None
    with pytest.raises(AssertionError, match="the device was reached"):
        m.match(names, names, embeddings_from=x, embeddings_to=x)


@pytest.mark.parametrize("field,value", [("precision", "int8"), ("binary", "ubinary"), ("compute_dtype", "float16"),
                                         ("rescore_multiplier", 4), ("rescore_to", "int8")])
@pytest.mark.parametrize("search", C.DTYPES)
def test_the_other_fields_are_still_refused_with_search_dtype_set(field, value, search, monkeypatch):
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import Embeddings
    monkeypatch.setattr(_lib.Context, "default", classmethod(_no_device))
    names, x = _vectors()
    m, plain = Embeddings(), Embeddings()
    m.search_dtype = search
    setattr(m, field, value)
    setattr(plain, field, value)
    for call in (lambda e: e.join(names, min_similarity=0.8, embeddings_from=x), lambda e: e.components(names, 0.8, embeddings=x)):
        with pytest.raises(ValueError, match=field) as got:
            call(m)
        with pytest.raises(ValueError, match=field) as want:
            call(plain)
        assert str(got.value) == str(want.value) and "fp32" in str(got.value)           # today's message, word for word


def test_search_dtype_none_reaches_k14_and_a_type_reaches_k22(monkeypatch):
    from polyfuzz_amd import linkage
    from polyfuzz_amd.models import Embeddings
    log = _stub_device(monkeypatch)
    names, x = _vectors()
    m = Embeddings()
    m.join(names, min_similarity=0.8, embeddings_from=x)
    m.join(names, names, 0.8, embeddings_from=x, embeddings_to=x)
    m.components(names, 0.8, embeddings=x)
    assert [c[0] for c in log if c[0] != "upload"] == ["k14_join", "k14_join", "k14_components"] and m.last_counts == {"pairs": 0, "components": 3}
    del log[:]
    m.search_dtype = "float16"
    frame = m.join(names, min_similarity=0.8, embeddings_from=x)
    assert list(frame.columns) == ["From", "To", "Similarity"] and m.last_counts == {"pairs": 0, "candidates": 5}
    assert log == [("upload", 3), ("derive16", "f32", "float16"), ("k22_join", "f3216", None, "f32", None)]      # uploaded once, derived on the device
    del log[:]
    m.join(names, names, 0.8, embeddings_from=x, embeddings_to=x)
    assert [c[0] for c in log] == ["upload", "upload", "derive16", "derive16", "k22_join"] and log[-1] == ("k22_join", "f3216", "f3216", "f32", "f32")
    del log[:]
    label = m.components(names, 0.8, embeddings=x)
    assert log == [("upload", 3), ("derive16", "f32", "float16"), ("k22_components", "f3216", "f32")]
    assert label.tolist() == [0, 1, 2] and m.last_counts == {"pairs": 0, "components": 3, "candidates": 7}
    assert set(m.last_timings) == {"device", "frame"}
    del log[:]
    assert linkage.connected_components(names, m, 0.8, embeddings=x) == linkage.dicts_from_labels(names, [0, 1, 2])
    assert log[-1][0] == "k22_components"


def test_search_dtype_survives_pickling_and_old_pickles_default_it():
    from polyfuzz_amd.models import Embeddings
    m = Embeddings()
    m.search_dtype = "bfloat16"
    assert pickle.loads(pickle.dumps(m)).search_dtype == "bfloat16"
    state = m.__getstate__()
    del state["_search_dtype"]                              # a matcher pickled before the attribute existed
    old = Embeddings.__new__(Embeddings)
    old.__setstate__(state)
    assert old.search_dtype is None


def test_binding_refuses_wrong_operands_without_a_library_call():
    from polyfuzz_amd import _lib

    class Dev:
        n, h = 3, None

    def dev(dtype, normalize=True):
        d = Dev()
        d.dtype, d.normalize = dtype, normalize
        return d
    for bad in (dev("float32"), dev("int8"), dev(_lib.BINARY), dev("float16", False)):
        with pytest.raises(ValueError, match="16-bit search"):
            _lib.dense_join16(None, bad, None, dev("float32"), None, 0.5)
        with pytest.raises(ValueError, match="16-bit search"):
            _lib.dense_components16(None, bad, dev("float32"), 0.5)
    for bad in (dev("float16"), dev("float32", False)):
        with pytest.raises(ValueError, match="fp32"):
            _lib.dense_join16(None, dev("bfloat16"), None, bad, None, 0.5)
        with pytest.raises(ValueError, match="fp32"):
            _lib.dense_components16(None, dev("bfloat16"), bad, 0.5)
    for d in (dev("float16"), dev("bfloat16")):             # K14's own entries keep refusing 16-bit handles
        with pytest.raises(ValueError, match="fp32"):
            _lib.dense_join(None, d, None, 0.5)
        with pytest.raises(ValueError, match="fp32"):
            _lib.dense_components(None, d, 0.5)


def test_kernel_budget():
    """Both k22_search_kernel instances keep the 16-bit tile program's budget -- no scratch, at most 256 registers per lane,
    accumulation registers included, LDS <= 160 KiB (the two double-buffered operand tiles: 147 456 B) -- and k22_rescore_kernel has
    no scratch."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_budget
    from polyfuzz_amd import _build
    for exe in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(kernel_budget.LLVM, exe)):
            pytest.skip(f"{exe} not in {kernel_budget.LLVM}")
    md = kernel_budget.kernel_metadata(_build.build())
    pretty = dict(zip(md, kernel_budget.demangled(list(md))))
    search = {pretty[k]: v for k, v in md.items() if "k22_search_kernel" in pretty[k]}
    assert len(search) == 2 and any("pfz::f16" in p for p in search) and any("pfz::bf16" in p for p in search), list(search)
    for name, k in search.items():
        assert k["scratch"] == 0 and k["vgpr"] + k.get("agpr", 0) <= 256, (name, k)
        assert k["lds"] <= 160 * 1024 and k["lds"] == 2 * 2 * 256 * 144, (name, k)
    rescore = {pretty[k]: v for k, v in md.items() if "k22_rescore_kernel" in pretty[k]}
    assert len(rescore) >= 1 and all(v["scratch"] == 0 for v in rescore.values()), rescore
    assert not any("k14_" in p or "gemm16_panel" in p for p in list(search) + list(rescore))
