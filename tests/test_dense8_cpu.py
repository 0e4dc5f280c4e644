"""The int8 dense path (scalar-quantised embeddings on the integer matrix cores) as far as it can be held without a GPU:
the C ABI declares and binds its entry point, the Python doors validate before any device call, `Embeddings.precision` is
kept through pickling, and the built library holds ONE instance of the int8 tile program within the budget of the 16-bit one
it shares its body with."""
import os
import pickle
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "tools"))


def test_header_and_ctypes_table_hold_the_int8_entry_point():
    from polyfuzz_amd import _lib
    src = open(os.path.join(REPO, "include", "polyfuzz_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+pfz_dense_upload8\s*\(([^)]*)\)", src)
    assert m and len(m.group(1).split(",")) == 7, m
    assert re.search(r"#define\s+PFZ_DENSE_I8\s+3\b", src)
    assert "pfz_dense_upload8" in _lib.SIGNATURES and len(_lib.SIGNATURES["pfz_dense_upload8"][1]) == 7
    assert _lib.DENSE_DTYPES == {"float32": 0, "float16": 1, "bfloat16": 2}      # int8 has a door of its own
    assert len(_lib.SIGNATURES["pfz_dense_upload16"][1]) == 8


def test_precision_validates_before_any_device_call():
    from polyfuzz_amd import _lib
    assert _lib.check_precision(None) is None and _lib.check_precision("int8") == "int8"
    for bad in ("uint8", "binary", "float32", "INT8", np.int8, 8, True):
        with pytest.raises(ValueError, match="precision"):
            _lib.check_precision(bad)
    # ctx=None: a device call would fail with AttributeError, not ValueError
    for bad in (np.zeros((2, 2), np.uint8), np.zeros((2, 2), np.int16), np.zeros((2, 2), np.int64), np.zeros((2, 2), bool)):
        with pytest.raises(ValueError, match="int8"):
            _lib.DeviceDense.upload_int8(None, bad)
        with pytest.raises(ValueError, match="int8"):
            _lib.dense_int8_topn_host(None, bad, bad, 1, 0.0)
    with pytest.raises(ValueError, match="unsigned"):
        _lib.DeviceDense.upload_int8(None, np.zeros((2, 2), np.uint8))
    with pytest.raises(ValueError, match="2-D"):
        _lib.DeviceDense.upload_int8(None, np.zeros(4, np.int8))
    with pytest.raises(ValueError, match="compute_dtype"):                        # the other door still refuses the name
        _lib.check_compute_dtype("int8")


def test_embeddings_precision_attribute():
    from polyfuzz_amd.models import Embeddings
    m = Embeddings(min_similarity=0.1, top_n=3, cosine_method="hip")
    assert m.precision is None and Embeddings().precision is None
    for bad in ("uint8", "binary", np.int8, 8):
        with pytest.raises(ValueError, match="precision"):
            m.precision = bad
    assert m.precision is None
    with pytest.raises(ValueError, match="compute_dtype"):
        m.compute_dtype = "int8"
    m.precision = "int8"
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.precision == "int8" and m2.compute_dtype is None and m2.top_n == 3 and m2._dev_to is None
    m.precision = None
    assert m.precision is None
    state = m.__getstate__()
    del state["_precision"]                                   # pickled before the attribute existed
    old = Embeddings.__new__(Embeddings)
    old.__setstate__(state)
    assert old.precision is None


def test_embeddings_refuses_int8_with_a_16bit_compute_dtype():
    """raised by match() before anything is uploaded: no device is needed to see it"""
    from polyfuzz_amd.models import Embeddings
    m = Embeddings(min_similarity=0.0, cosine_method="hip")
    m.precision = "int8"
    m.compute_dtype = "float16"
    e = np.ones((2, 4), np.float32)
    with pytest.raises(ValueError, match="precision.*compute_dtype"):
        m.match(["a", "b"], ["c", "d"], embeddings_from=e, embeddings_to=e)


def test_one_gemm8_instance_at_one_workgroup_per_cu():
    """k5_gemm8_panel shares the 16-bit tile program's body: ONE workgroup of 512 threads per CU, at most 256 registers per
    lane, 147 456 B of LDS within the CU's 160 KiB, no scratch; the 16-bit program stays two instances."""
    import kernel_budget
    from polyfuzz_amd import _build
    for exe in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(kernel_budget.LLVM, exe)):
            pytest.skip(f"{exe} not in {kernel_budget.LLVM}")
    md = kernel_budget.kernel_metadata(_build.build())
    pretty = dict(zip(md, kernel_budget.demangled(list(md))))
    hits = [v for k, v in md.items() if pretty[k].startswith("void pfz::k5_gemm8_panel")]
    assert len(hits) == 1, [p for p in pretty.values() if "gemm8" in p]
    k = hits[0]
    assert k["scratch"] == 0, k
    assert k["vgpr"] <= 256, k
    assert k["lds"] <= 160 * 1024, k
    assert len([p for p in pretty.values() if "k5_gemm16_panel" in p]) == 2


def test_one_operand_vocabulary_behind_both_keywords():
    """_lib.operand_type over the whole grid of the two public keywords, and DeviceDense.upload_as refusing what each door
    refuses, in the same words, before any device call (ctx=None: a device call would fail with AttributeError)."""
    from polyfuzz_amd import _lib
    assert _lib.OPERAND_TYPES == ("float32", "float16", "bfloat16", "int8")
    got = {}
    for cd in (None, "float32", "float16", "bfloat16"):
        for pr in (None, "int8"):
            try:
                got[cd, pr] = _lib.operand_type(cd, pr)
            except ValueError as e:
                got[cd, pr] = e
    assert [got[cd, None] for cd in (None, "float32", "float16", "bfloat16")] == ["float32", "float32", "float16", "bfloat16"]
    assert got[None, "int8"] == got["float32", "int8"] == "int8"
    for cd in ("float16", "bfloat16"):
        assert str(got[cd, "int8"]) == f'precision="int8" and compute_dtype={cd!r} name two operand types: leave compute_dtype at None'
    assert _lib.operand_type() == "float32"
    with pytest.raises(ValueError, match="compute_dtype must be None or one of"):
        _lib.operand_type("int8", None)
    with pytest.raises(ValueError, match='precision must be None or "int8"'):
        _lib.operand_type(None, "uint8")

    def refusal(f, *args):
        with pytest.raises(ValueError) as e:
            f(None, *args)
        return str(e.value)
    D = _lib.DeviceDense
    for bad in (np.zeros((2, 2), np.uint8), np.zeros((2, 2), np.int16), np.zeros(4, np.float32)):
        assert refusal(D.upload_as, bad, "int8") == refusal(D.upload_int8, bad)
        for name in ("float16", "bfloat16"):
            assert refusal(D.upload_as, bad, name) == refusal(D.upload, bad, True, name)
    assert "unsigned" in refusal(D.upload_as, np.zeros((2, 2), np.uint8), "int8")
    assert "raw bfloat16 bits as uint16, got int16" in refusal(D.upload_as, np.zeros((2, 2), np.int16), "bfloat16")
    assert refusal(D.upload_as, np.zeros(4, np.float32), "float32") == refusal(D.upload, np.zeros(4, np.float32)) \
        == "dense vectors must be a 2-D array, got shape (4,)"
    for unknown in ("fp8", "half", None, np.int8, 8):
        with pytest.raises(ValueError, match="operand must be one of"):
            D.upload_as(None, np.zeros((2, 2), np.float32), unknown)
