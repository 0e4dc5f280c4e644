"""K14 without a GPU: the entry points in header, library and ctypes table, the header's contract, the float32 threshold, the
refusals of Embeddings.join / .components before any device call, and the kernels' register / LDS budgets."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    for name in ("pfz_dense_join", "pfz_dense_components"):
        assert f"int {name}(" in header and hasattr(so, name) and name in _lib.SIGNATURES
    assert _arg_names(header, "pfz_dense_join") == ["ctx", "from_vectors", "to_vectors", "min_similarity", "capacity", "out_row_ptr",
                                                    "out_idx", "out_sim", "out_total", "out_counters"]
    assert _arg_names(header, "pfz_dense_components") == ["ctx", "vectors", "min_similarity", "out_label", "out_pairs", "out_components",
                                                          "out_counters"]
    restype, argtypes = _lib.SIGNATURES["pfz_dense_join"]
    assert restype is ctypes.c_int and len(argtypes) == 10 and argtypes[3] is ctypes.c_double and argtypes[4] is ctypes.c_int64
    restype, argtypes = _lib.SIGNATURES["pfz_dense_components"]
    assert restype is ctypes.c_int and len(argtypes) == 7 and argtypes[2] is ctypes.c_double
    assert _lib.DENSE_JOIN_COUNTERS == ("tiles", "hit_corners")
    for f, names in ((_lib.dense_join, ["ctx", "from_dev", "to_dev", "min_similarity", "capacity", "counters"]),
                     (_lib.dense_components, ["ctx", "dev", "min_similarity", "counters"])):
        assert list(inspect.signature(f).parameters) == names


def test_header_states_the_capacity_rule_and_the_limits():
    header = _header()
    doc = header[header.index("---- K14"):header.index("int pfz_dense_components(")]
    doc = " ".join(doc.replace(" * ", " ").split())
    for phrase in ("*out_total is always the exact number of hits", "returns PFZ_OK, has written NONE of the three output arrays",
                   "repeated with capacity >= *out_total", "ascending within a row", "same call gives the same bytes",
                   "2^31 tiles", "fewer than 2^31 rows", "PFZ_ERR_UNSUPPORTED", "PFZ_ERR_INVALID", "fp32", "never (i, i)",
                   "k14_join", "k14_sort_unpack", "k14_components", "int64[2]"):
        assert phrase in doc, phrase


def test_dense_threshold32_is_the_smallest_float32_at_or_above_t():
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(14)
    f32 = rng.random(3000).astype(np.float32)
    ts = np.concatenate([rng.random(10000), f32.astype(np.float64), np.nextafter(f32.astype(np.float64), 2.0),
                         np.nextafter(f32.astype(np.float64), -1.0), [0.0, 1.0, 0.6, 0.8, 0.9, np.nextafter(1.0, 0.0), 5e-324]])
    ts = ts[(ts >= 0.0) & (ts <= 1.0)]
    for t in ts.tolist():
        r = _lib.dense_threshold32(t)
        assert isinstance(r, np.float32)
        assert np.float64(r) >= t > np.float64(np.nextafter(r, np.float32(-np.inf))), (t, r)
    assert _lib.dense_threshold32(0.0) == 0.0 and _lib.dense_threshold32(1.0) == 1.0
    assert _lib.dense_threshold32(np.float64(np.float32(0.8))) == np.float32(0.8) < _lib.dense_threshold32(0.8000001)


def _vectors():
    return ["a", "b", "c"], np.eye(3, 8, dtype=np.float32)


@pytest.mark.parametrize("field,value", [("precision", "int8"), ("binary", "ubinary"), ("compute_dtype", "float16"),
                                         ("compute_dtype", "bfloat16"), ("rescore_multiplier", 4), ("rescore_to", "int8")])
def test_other_operand_types_are_refused_before_any_device_call(field, value, monkeypatch):
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import Embeddings
    monkeypatch.setattr(_lib.Context, "default", classmethod(_no_device))
    names, x = _vectors()
    m = Embeddings()
    setattr(m, field, value)
    with pytest.raises(ValueError, match=field) as e:
        m.join(names, min_similarity=0.8, embeddings_from=x)
    assert "fp32" in str(e.value) and not isinstance(e.value, _lib.PfzError)
    with pytest.raises(ValueError, match=field):
        m.join(names, names, 0.8, embeddings_from=x, embeddings_to=x)
    with pytest.raises(ValueError, match=field):
        m.components(names, 0.8, embeddings=x)
    setattr(m, field, None)                               # unset again: the device is what stops the call
    with pytest.raises(AssertionError, match="the device was reached"):
        m.join(names, min_similarity=0.8, embeddings_from=x)
    m.compute_dtype = "float32"                           # (fp32 under its own name is no other type)
    with pytest.raises(AssertionError, match="the device was reached"):
        m.components(names, 0.8, embeddings=x)


def test_min_similarity_must_be_a_number_in_0_1(monkeypatch):
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import Embeddings
    monkeypatch.setattr(_lib.Context, "default", classmethod(_no_device))
    names, x = _vectors()
    m = Embeddings(cosine_method="sparse")
    for bad in (float("nan"), float("inf"), -float("inf"), -1e-300, np.nextafter(1.0, 2.0), 1.5, -0.1, "0.8", None, True, [0.8]):
        with pytest.raises(ValueError, match="min_similarity"):
            m.join(names, names, bad, embeddings_from=x, embeddings_to=x)
        with pytest.raises(ValueError, match="min_similarity"):
            m.join(names, min_similarity=bad, embeddings_from=x)
        with pytest.raises(ValueError, match="min_similarity"):
            m.components(names, bad, embeddings=x)
    for good in (0, 1, 0.0, 1.0, 0.8, np.float64(0.5), np.float32(0.25), np.int64(1)):      # accepted: the device is what stops these
        with pytest.raises(AssertionError, match="the device was reached"):
            m.join(names, names, good, embeddings_from=x, embeddings_to=x)
        with pytest.raises(AssertionError, match="the device was reached"):
            m.components(names, good, embeddings=x)
    with pytest.raises(ValueError, match="embeddings_to"):
        m.join(names, min_similarity=0.8, embeddings_from=x, embeddings_to=x)
    with pytest.raises(ValueError, match="shape"):
        m.join(names, min_similarity=0.8, embeddings_from=x[:2])
    with pytest.raises(ValueError, match="equal width"):
        m.join(names, names, 0.8, embeddings_from=x, embeddings_to=x[:, :4])
    assert "cosine_method" in Embeddings.join.__doc__ and list(inspect.signature(Embeddings.join).parameters) == [
        "self", "from_list", "to_list", "min_similarity", "embeddings_from", "embeddings_to"]
    assert list(inspect.signature(Embeddings.components).parameters) == ["self", "strings", "min_similarity", "embeddings"]


def test_binding_refuses_other_operands_without_a_library_call():
    from polyfuzz_amd import _lib

    class Dev:
        n, h = 3, None
    for dtype, normalize in (("float16", True), ("bfloat16", True), ("int8", True), (_lib.BINARY, True), ("float32", False)):
        d = Dev()
        d.dtype, d.normalize = dtype, normalize
        with pytest.raises(ValueError, match="fp32"):
            _lib.dense_join(None, d, None, 0.5)
        with pytest.raises(ValueError, match="fp32"):
            _lib.dense_components(None, d, 0.5)


def test_connected_components_passes_embeddings_only_when_given():
    from polyfuzz_amd import linkage
    calls = []

    class Model:
        def components(self, strings, min_similarity, **kw):
            calls.append((list(strings), min_similarity, kw))
            return np.array([0, 0, 2], np.int32)
    want = linkage.dicts_from_labels(["a", "b", "c"], [0, 0, 2])
    assert linkage.connected_components(["a", "b", "c"], Model(), 0.7) == want
    x = np.zeros((3, 4), np.float32)
    assert linkage.connected_components(["a", "b", "c"], Model(), 0.7, embeddings=x) == want
    assert calls[0] == (["a", "b", "c"], 0.7, {}) and calls[1][2].keys() == {"embeddings"} and calls[1][2]["embeddings"] is x
    p = inspect.signature(linkage.connected_components).parameters
    assert list(p)[-1] == "embeddings" and p["embeddings"].default is None


def test_kernel_budget():
    """k14_join_kernel and k14_comp_kernel exist once each and still fit TWO workgroups per CU, as their __launch_bounds__(256, 2)
    says: no scratch, static LDS <= 80 KiB (the two double-buffered operand tiles and nothing else: K5's 73 728 B), at most 256
    registers per lane, accumulation registers included.  k5_gemm_panel_pipe is still there under its name, with the LDS and
    the scratch it had before its main loop became k5_tile_loop (DESIGN.md section 4 records the registers)."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_budget
    from polyfuzz_amd import _build
    for exe in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(kernel_budget.LLVM, exe)):
            pytest.skip(f"{exe} not in {kernel_budget.LLVM}")
    md = kernel_budget.kernel_metadata(_build.build())
    pretty = dict(zip(md, kernel_budget.demangled(list(md))))
    for name in ("k14_join_kernel", "k14_comp_kernel"):
        hits = [v for k, v in md.items() if pretty[k].startswith(f"pfz::{name}(")]
        assert len(hits) == 1, (name, [p for p in pretty.values() if "k14_" in p])
        k = hits[0]
        assert k["scratch"] == 0, (name, k)
        assert k["lds"] <= 80 * 1024 and k["lds"] == 2 * 2 * 128 * 36 * 4, (name, k)
        # (on gfx950 the code object's vgpr_count is the lane's whole unified file, the accumulation registers included, so the
        # sum counts them twice: the bound is held the strict way)
        assert k["vgpr"] + k.get("agpr", 0) <= 256, (name, k)
    panel = [v for k, v in md.items() if pretty[k].startswith("pfz::k5_gemm_panel_pipe(")]
    assert len(panel) == 1 and (panel[0]["lds"], panel[0]["scratch"]) == (73728, 0) and panel[0]["vgpr"] <= 256, panel
    assert any(pretty[k].startswith("pfz::k14_unpack(") for k in md)
    for k, v in md.items():
        if "k14_" in pretty[k] or "k_bitonic_kv" in pretty[k] or "k_sort_pad_kv" in pretty[k]:
            assert v["scratch"] == 0, (pretty[k], v)
