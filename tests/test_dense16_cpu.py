"""The 16-bit dense path (float16 / bfloat16 embeddings on the 16-bit matrix cores) as far as it can be held without a
GPU: the C ABI declares and binds its entry points, the Python keyword validates before any device call and is kept through
pickling, and
the built library holds one instance of the tile program per type within the budget it was designed for."""
import os
import pickle
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "tools"))


def test_header_and_ctypes_table_hold_the_new_entry_points():
    from polyfuzz_amd import _lib
    src = open(os.path.join(REPO, "include", "polyfuzz_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("pfz_dense_upload16", "pfz_dense_dtype"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["pfz_dense_upload16"][1]) == 8 and len(_lib.SIGNATURES["pfz_dense_dtype"][1]) == 2
    for const, value in (("PFZ_DENSE_F32", 0), ("PFZ_DENSE_F16", 1), ("PFZ_DENSE_BF16", 2)):
        assert re.search(r"#define\s+" + const + r"\s+" + str(value) + r"\b", src), const
    assert _lib.DENSE_DTYPES == {"float32": 0, "float16": 1, "bfloat16": 2}


def test_embeddings_refuses_an_unknown_compute_dtype():
    """Embeddings.__init__ and cosine_similarity are held EQUAL to the reference's signatures by
    tests/test_reference_interface_cpu.py, so the opt-in is an attribute of the matcher, validated when it is set."""
    from polyfuzz_amd.models import Embeddings
    m = Embeddings()
    with pytest.raises(ValueError, match="compute_dtype"):
        m.compute_dtype = "int8"
    with pytest.raises(ValueError, match="compute_dtype"):
        m.compute_dtype = np.float16                  # the names are strings: a numpy type is not silently accepted
    assert m.compute_dtype is None
    m.compute_dtype = "float32"


def test_embeddings_keeps_compute_dtype_through_pickling():
    from polyfuzz_amd.models import Embeddings
    m = Embeddings(min_similarity=0.1, top_n=3, cosine_method="hip")
    m.compute_dtype = "bfloat16"
    assert m.compute_dtype == "bfloat16"
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.compute_dtype == "bfloat16" and m2.top_n == 3 and m2._dev_to is None
    assert Embeddings().compute_dtype is None                       # opt-in: the default stays fp32


def test_the_keyword_validates_before_any_device_call():
    from polyfuzz_amd import _lib
    for bad in ("int8", "half", 16, np.float16):
        with pytest.raises(ValueError, match="compute_dtype"):
            _lib.check_compute_dtype(bad)
        with pytest.raises(ValueError, match="compute_dtype"):
            _lib.DeviceDense.upload(None, np.zeros((2, 2), np.float32), True, bad)
        with pytest.raises(ValueError, match="compute_dtype"):
            _lib.dense_cossim_topn_host(None, np.zeros((2, 2)), np.zeros((2, 2)), 1, 0.0, compute_dtype=bad)
    assert [_lib.check_compute_dtype(x) for x in (None, "float32", "float16", "bfloat16")] == \
        ["float32", "float32", "float16", "bfloat16"]
    import inspect
    from polyfuzz_amd import pipeline
    for f in (_lib.DeviceDense.upload, _lib.dense_cossim_topn_host, pipeline.DenseMatchJob.__init__):
        p = inspect.signature(f).parameters["compute_dtype"]
        assert p.default is None and list(inspect.signature(f).parameters)[-1] == "compute_dtype"      # trailing, opt-in


def test_one_gemm16_instance_per_type_at_one_workgroup_per_cu():
    """k5_gemm16_panel is built for ONE workgroup of 512 threads per CU (256 x 256 tiles): 8 waves = 2 waves per SIMD, so at
    most 256 registers per lane (512 per SIMD lane, vector + accumulation registers together), and its LDS (2 buffers x
    2 operands x 256 rows x 144 B = 147 456 B) within the CU's 160 KiB.  No scratch."""
    import kernel_budget
    from polyfuzz_amd import _build
    for exe in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(kernel_budget.LLVM, exe)):
            pytest.skip(f"{exe} not in {kernel_budget.LLVM}")
    md = kernel_budget.kernel_metadata(_build.build())
    pretty = dict(zip(md, kernel_budget.demangled(list(md))))
    for t in ("f16", "bf16"):
        hits = [v for k, v in md.items() if pretty[k].startswith(f"void pfz::k5_gemm16_panel<pfz::{t}>(")]
        assert len(hits) == 1, (t, [p for p in pretty.values() if "gemm16" in p])
        k = hits[0]
        assert k["scratch"] == 0, k
        assert k["vgpr"] <= 256, k
        assert k["lds"] <= 160 * 1024, k
    assert len([p for p in pretty.values() if "k5_gemm16_panel" in p]) == 2
