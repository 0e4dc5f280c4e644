"""Exact rescoring of a 16-bit / int8 top-n as far as it can be held without a GPU: the C ABI declares and binds the entry
point, the Python doors validate before any device call, `Embeddings.rescore_multiplier` is kept through pickling, and the
built library holds the two instances of k5_rescore_topn within their LDS plan."""
import inspect
import os
import pickle
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "tools"))


def test_header_and_ctypes_table_hold_the_rescoring_entry_point():
    """int pfz_dense_rescore_topn(ctx, from_exact, to_exact, candidates, ntop, lower_bound, out): seven parameters, the same
    seven in the ctypes table."""
    from polyfuzz_amd import _lib
    src = open(os.path.join(REPO, "include", "polyfuzz_hip.h")).read()
    assert "_embeddings.py:127-133" in src[src.index("Exact rescoring"):src.index("pfz_dense_rescore_topn(")]
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+pfz_dense_rescore_topn\s*\(([^)]*)\)", src)
    assert m, "include/polyfuzz_hip.h does not declare pfz_dense_rescore_topn"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["pfz_ctx *ctx", "const pfz_dense *from_exact", "const pfz_dense *to_exact", "const pfz_topn *candidates",
                      "int32_t ntop", "float lower_bound", "pfz_topn *out"]
    res, args = _lib.SIGNATURES["pfz_dense_rescore_topn"]
    assert res is _lib.ctypes.c_int and len(args) == len(params)
    assert args == [_lib.c_vp] * 4 + [_lib.c_i32, _lib.c_f32, _lib.c_vp]
    knobs = open(os.path.join(REPO, "polyfuzz_amd", "csrc", "pfz_knobs.h")).read()
    assert "RESCORE" not in knobs.upper()                                           # no new knob


def test_check_rescore_multiplier():
    from polyfuzz_amd import _lib
    assert _lib.check_rescore_multiplier(None) is None
    for ok in (1, 2, 4, 8, 1000, np.int64(3)):
        out = _lib.check_rescore_multiplier(ok)
        assert out == ok and type(out) is int
    for bad in (True, False, 0, -1, -4, 2.0, 0.5, "4", [4], np.float32(2)):
        with pytest.raises(ValueError, match="rescore_multiplier"):
            _lib.check_rescore_multiplier(bad)


def test_candidates_per_row_and_the_limit():
    from polyfuzz_amd import _lib
    assert _lib.RESCORE_MAX_CANDIDATES == 1024
    assert _lib.rescore_candidates(5, 4, 500_000) == 20
    assert _lib.rescore_candidates(10, 8, 50) == 50 and _lib.rescore_candidates(10, 8, 50, exclude_diag=True) == 49
    assert _lib.rescore_candidates(10, 8, 4) == 10                                  # at least top_n
    assert _lib.rescore_candidates(256, 4, 10_000) == 1024
    with pytest.raises(ValueError, match=r"top_n=257.*rescore_multiplier=4.*1024"):
        _lib.rescore_candidates(257, 4, 10_000)
    with pytest.raises(ValueError, match="rescore_multiplier"):
        _lib.rescore_candidates(5, None, 100)

    class Operand:                                                                  # what the doors read before the first device call
        def __init__(self, n, dim):
            self.n, self.dim = n, dim
    # ctx=None: a device call would fail with AttributeError, not ValueError
    with pytest.raises(ValueError, match=r"top_n=300.*rescore_multiplier=4.*1024"):
        _lib.dense_topn_rescored(None, Operand(10, 8), Operand(5000, 8), Operand(10, 8), Operand(5000, 8), 300, 0.0, 4)
    with pytest.raises(ValueError, match="rescore_multiplier"):
        _lib.dense_topn_rescored(None, Operand(10, 8), Operand(5000, 8), Operand(10, 8), Operand(5000, 8), 3, 0.0, 2.5)
    with pytest.raises(ValueError, match="not the same vectors"):
        _lib.dense_topn_rescored(None, Operand(10, 8), Operand(5000, 8), Operand(10, 8), Operand(4000, 8), 3, 0.0, 2)
    f = np.zeros((4, 8), np.float32)
    with pytest.raises(ValueError, match="coarse"):
        _lib.dense_rescored_topn_host(None, f, f, 1, 0.0, coarse="float32", multiplier=2)
    with pytest.raises(ValueError, match="rescore_multiplier"):
        _lib.dense_rescored_topn_host(None, f, f, 1, 0.0, coarse="int8", multiplier=0)
    for given in (f.astype(np.int8), f.astype(np.float16), f.astype(np.uint16)):
        with pytest.raises(ValueError, match="float32 / float64"):
            _lib.dense_rescored_topn_host(None, given, f, 1, 0.0, coarse="int8", multiplier=2)
    with pytest.raises(ValueError, match="1024"):
        _lib.dense_rescored_topn_host(None, f, np.zeros((3000, 8), np.float32), 600, 0.0, coarse="bfloat16", multiplier=2)
    sig = inspect.signature(_lib.dense_topn_rescored)
    assert list(sig.parameters)[:11] == ["ctx", "from_coarse", "to_coarse", "from_exact", "to_exact", "ntop", "lower_bound",
                                         "multiplier", "exclude_diag", "diag_offset", "out"]
    assert list(inspect.signature(_lib.dense_rescore).parameters) == ["ctx", "from_exact", "to_exact", "candidates", "ntop",
                                                                      "lower_bound", "out"]


def test_embeddings_rescore_multiplier_attribute():
    from polyfuzz_amd.models import Embeddings
    m = Embeddings(min_similarity=0.1, top_n=3, cosine_method="hip")
    assert m.rescore_multiplier is None and Embeddings().rescore_multiplier is None
    for bad in (True, 0, -2, 4.0, "4"):
        with pytest.raises(ValueError, match="rescore_multiplier"):
            m.rescore_multiplier = bad
    assert m.rescore_multiplier is None
    m.precision, m.rescore_multiplier = "int8", 4
    m2 = pickle.loads(pickle.dumps(m))                                              # never matched: no handles to leave behind
    assert m2.rescore_multiplier == 4 and m2.precision == "int8" and m2.top_n == 3
    assert m2._dev_to is None and m2._dev_to_exact is None
    state = m.__getstate__()
    assert "_dev_to" not in state and "_dev_to_exact" not in state
    del state["_rescore_multiplier"]                                                # pickled before the attribute existed
    old = Embeddings.__new__(Embeddings)
    old.__setstate__(state)
    assert old.rescore_multiplier is None and old.precision == "int8" and old._dev_to_exact is None
    m.rescore_multiplier = None
    assert m.rescore_multiplier is None
    assert "rescore_multiplier" not in inspect.signature(Embeddings.__init__).parameters      # the reference's constructor


def test_embeddings_refusals_need_no_device():
    """raised by match() before anything is uploaded"""
    from polyfuzz_amd.models import Embeddings
    e = np.ones((2, 4), np.float32)
    m = Embeddings(min_similarity=0.0, cosine_method="hip")
    m.rescore_multiplier = 2
    with pytest.raises(ValueError, match="nothing to rescore"):
        m.match(["a", "b"], ["c", "d"], embeddings_from=e, embeddings_to=e)
    m.precision = "int8"
    with pytest.raises(ValueError, match="embeddings_to.*int8.*no full-precision vectors"):
        m.match(["a", "b"], ["c", "d"], embeddings_from=e, embeddings_to=e.astype(np.int8))
    m.precision, m.compute_dtype = None, "bfloat16"
    with pytest.raises(ValueError, match="embeddings_from.*uint16.*no full-precision vectors"):
        m.match(["a", "b"], ["c", "d"], embeddings_from=e.astype(np.uint16), embeddings_to=e)
    m.compute_dtype = "float16"
    with pytest.raises(ValueError, match="float16.*no full-precision vectors"):
        m.match(["a", "b"], ["c", "d"], embeddings_from=e.astype(np.float16), embeddings_to=e)


def test_dense_match_job_keywords():
    from polyfuzz_amd import pipeline
    p = inspect.signature(pipeline.DenseMatchJob.__init__).parameters
    for name in ("rescore_from", "rescore_to", "rescore_multiplier"):
        assert p[name].default is None


def test_rescore_kernel_budget():
    """two instances: the from-row in LDS (16 KiB + 8 KiB of keys) or re-read from L2 (the keys alone); no scratch, and few
    enough registers for four workgroups of 256 threads per CU."""
    import kernel_budget
    from polyfuzz_amd import _build
    for exe in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(kernel_budget.LLVM, exe)):
            pytest.skip(f"{exe} not in {kernel_budget.LLVM}")
    md = kernel_budget.kernel_metadata(_build.build())
    pretty = dict(zip(md, kernel_budget.demangled(list(md))))
    hits = {pretty[k].split("(")[0]: v for k, v in md.items() if "k5_rescore_topn" in pretty[k]}
    assert sorted(hits) == ["void pfz::k5_rescore_topn<false>", "void pfz::k5_rescore_topn<true>"], sorted(hits)
    assert hits["void pfz::k5_rescore_topn<true>"]["lds"] == 8192 + 16384
    assert hits["void pfz::k5_rescore_topn<false>"]["lds"] <= 8192 + 16
    for k in hits.values():
        assert k["scratch"] == 0 and k["vgpr"] <= 128, k
