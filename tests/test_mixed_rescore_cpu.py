"""The mixed rescoring (float32 from-vectors against the int8 / 1-bit to-side itself) as far as it can be held without a GPU:
the C ABI declares, exports and binds pfz_dense_rescore_topn_mixed, the Python doors validate before any device call,
`Embeddings.rescore_to` is validated when set and kept through pickling, and the built library holds the instances of
k5_mixed_rescore within the LDS plan of k5_rescore_topn, without scratch."""
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


def test_header_ctypes_table_and_library_hold_the_entry_point():
    from polyfuzz_amd import _build, _lib
    src = open(os.path.join(REPO, "include", "polyfuzz_hip.h")).read()
    assert "_embeddings.py:127-133" in src[src.index("Mixed rescoring"):src.index("pfz_dense_rescore_topn_mixed(")]
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+pfz_dense_rescore_topn_mixed\s*\(([^)]*)\)", src)
    assert m, "include/polyfuzz_hip.h does not declare pfz_dense_rescore_topn_mixed"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["pfz_ctx *ctx", "const pfz_dense *from_exact", "const pfz_dense *to_coarse", "const pfz_topn *candidates",
                      "int32_t ntop", "float lower_bound", "pfz_topn *out"]
    res, args = _lib.SIGNATURES["pfz_dense_rescore_topn_mixed"]
    assert res is _lib.ctypes.c_int and args == [_lib.c_vp] * 4 + [_lib.c_i32, _lib.c_f32, _lib.c_vp]
    assert _lib.SIGNATURES["pfz_dense_rescore_topn"] == (res, args)                 # the sibling's seven, in its order
    if _build.is_stale():
        _build.build()
    assert hasattr(_lib.ctypes.CDLL(_lib.lib_path()), "pfz_dense_rescore_topn_mixed")      # exported by the built library
    knobs = open(os.path.join(REPO, "polyfuzz_amd", "csrc", "pfz_knobs.h")).read()
    assert "MIXED" not in knobs.upper() and "RESCORE" not in knobs.upper()          # no new knob
    assert list(inspect.signature(_lib.dense_rescore_mixed).parameters) == ["ctx", "from_exact", "to_coarse", "candidates", "ntop",
                                                                            "lower_bound", "out"]


def test_check_rescore_to_and_the_pairs():
    from polyfuzz_amd import _lib
    assert _lib.check_rescore_to(None) is None and _lib.check_rescore_to("int8") == "int8"
    assert _lib.check_rescore_to("binary") == _lib.check_rescore_to("ubinary") == _lib.BINARY
    for bad in ("float32", "float16", "INT8", "", 8, True, ("int8",)):
        with pytest.raises(ValueError, match="rescore_to must be"):
            _lib.check_rescore_to(bad)
    assert _lib.MIXED_RESCORE_PAIRS == (("int8", "int8"), ("binary", "binary"), ("binary", "int8"))
    for coarse, to in (("int8", "binary"), ("float16", "int8"), ("bfloat16", "binary"), ("float32", "int8")):
        with pytest.raises(ValueError, match="cannot follow"):
            _lib.check_mixed_pair(coarse, to)


def test_one_shot_refusals_need_no_device():
    """ctx=None: a device call would fail with AttributeError, not ValueError"""
    from polyfuzz_amd import _lib
    assert inspect.signature(_lib.dense_rescored_topn_host).parameters["rescore_to"].default is None
    f = np.zeros((4, 8), np.float32)
    q, u = f.astype(np.int8), np.zeros((4, 1), np.uint8)
    for coarse, to in (("int8", "binary"), ("int8", "ubinary"), ("float16", "int8"), ("bfloat16", "binary")):
        with pytest.raises(ValueError, match="cannot follow"):
            _lib.dense_rescored_topn_host(None, f, f, 1, 0.0, coarse=coarse, multiplier=2, rescore_to=to)
    with pytest.raises(ValueError, match="rescore_to must be"):
        _lib.dense_rescored_topn_host(None, f, f, 1, 0.0, coarse="int8", multiplier=2, rescore_to="float32")
    with pytest.raises(ValueError, match="coarse"):
        _lib.dense_rescored_topn_host(None, f, f, 1, 0.0, coarse="float32", multiplier=2, rescore_to="int8")
    with pytest.raises(ValueError, match="rescore_multiplier"):
        _lib.dense_rescored_topn_host(None, f, q, 1, 0.0, coarse="int8", multiplier=0, rescore_to="int8")
    with pytest.raises(ValueError, match="needs coarse='int8'"):                     # an int8 to-side under a bit search
        _lib.dense_rescored_topn_host(None, f, q, 1, 0.0, coarse="binary", multiplier=2, rescore_to="int8")
    with pytest.raises(ValueError, match="float32 / float64"):                      # packed bits cannot become int8
        _lib.dense_rescored_topn_host(None, f, u, 1, 0.0, coarse="binary", multiplier=2, rescore_to="int8")
    for given, to in ((q, "int8"), (u, "binary")):                                  # the from-side stays float
        with pytest.raises(ValueError, match="float32 / float64"):
            _lib.dense_rescored_topn_host(None, given, given, 1, 0.0, coarse=to, multiplier=2, rescore_to=to)
    with pytest.raises(ValueError, match="float32 / float64"):                      # without rescore_to: as before
        _lib.dense_rescored_topn_host(None, f, q, 1, 0.0, coarse="int8", multiplier=2)
    with pytest.raises(ValueError, match=r"equal width.*\(4, 16\).*8 bits per byte"):
        _lib.dense_rescored_topn_host(None, f, np.zeros((4, 2), np.uint8), 1, 0.0, coarse="binary", multiplier=2, rescore_to="ubinary")
    with pytest.raises(ValueError, match="equal width"):
        _lib.dense_rescored_topn_host(None, f, np.zeros((4, 9), np.int8), 1, 0.0, coarse="int8", multiplier=2, rescore_to="int8")
    with pytest.raises(ValueError, match="1024"):
        _lib.dense_rescored_topn_host(None, f, np.zeros((3000, 8), np.int8), 600, 0.0, coarse="int8", multiplier=2, rescore_to="int8")

    class Operand:                                                                  # what dense_topn_rescored reads first
        def __init__(self, n, dim, dtype):
            self.n, self.dim, self.dtype = n, dim, dtype
    with pytest.raises(ValueError, match="not the same vectors"):
        _lib.dense_topn_rescored(None, Operand(10, 8, "int8"), Operand(50, 8, "int8"), Operand(10, 8, "float32"), Operand(40, 8, "int8"),
                                 3, 0.0, 2)
    with pytest.raises(ValueError, match=r"top_n=300.*1024"):
        _lib.dense_topn_rescored(None, Operand(10, 8, "binary"), Operand(5000, 8, "binary"), Operand(10, 8, "float32"),
                                 Operand(5000, 8, "int8"), 300, 0.0, 4)


def test_embeddings_rescore_to_attribute():
    from polyfuzz_amd.models import Embeddings
    m = Embeddings(min_similarity=0.1, top_n=3, cosine_method="hip")
    assert m.rescore_to is None and Embeddings().rescore_to is None
    for bad in ("float32", "float16", 8, True, "INT8"):
        with pytest.raises(ValueError, match="rescore_to must be"):
            m.rescore_to = bad
    assert m.rescore_to is None
    for ok in ("int8", "binary", "ubinary", None):
        m.rescore_to = ok
        assert m.rescore_to == ok
    m.binary, m.rescore_multiplier, m.rescore_to = "ubinary", 16, "int8"
    m2 = pickle.loads(pickle.dumps(m))                                              # never matched: no handles to leave behind
    assert m2.rescore_to == "int8" and m2.binary == "ubinary" and m2.rescore_multiplier == 16 and m2.top_n == 3
    assert m2._dev_to is None and m2._dev_to_exact is None
    state = m.__getstate__()
    assert "_dev_to" not in state and "_dev_to_exact" not in state
    del state["_rescore_to"], state["_dev_to_exact_form"]                           # pickled before the attribute existed
    old = Embeddings.__new__(Embeddings)
    old.__setstate__(state)
    assert old.rescore_to is None and old.binary == "ubinary" and old._dev_to_exact is None
    assert "rescore_to" not in inspect.signature(Embeddings.__init__).parameters    # the reference's constructor
    assert "rescore_to:" in Embeddings.__doc__


def test_embeddings_refusals_need_no_device():
    """raised by match() before anything is uploaded (the arrays are not even 2-D floats of a sane width for the device)"""
    from polyfuzz_amd.models import Embeddings
    e = np.ones((2, 8), np.float32)
    u = np.ones((2, 1), np.uint8)
    lists = (["a", "b"], ["c", "d"])
    m = Embeddings(min_similarity=0.0, cosine_method="hip")
    m.rescore_to = "int8"
    with pytest.raises(ValueError, match="without a rescore_multiplier"):
        m.match(*lists, embeddings_from=e, embeddings_to=e)
    m.rescore_multiplier = 2
    with pytest.raises(ValueError, match="nothing to rescore"):                     # float32 operands
        m.match(*lists, embeddings_from=e, embeddings_to=e)
    m.compute_dtype = "float16"
    with pytest.raises(ValueError, match="rescore_to='int8'.*compute_dtype='float16'"):
        m.match(*lists, embeddings_from=e, embeddings_to=e)
    m.compute_dtype, m.precision, m.rescore_to = None, "int8", "ubinary"
    with pytest.raises(ValueError, match="cannot follow"):
        m.match(*lists, embeddings_from=e, embeddings_to=e)
    m.rescore_to = "int8"
    with pytest.raises(ValueError, match="embeddings_from.*int8.*no full-precision vectors"):
        m.match(*lists, embeddings_from=e.astype(np.int8), embeddings_to=e.astype(np.int8))
    m.precision, m.binary = None, "ubinary"
    with pytest.raises(ValueError, match="same form"):                              # packed bits cannot become int8
        m.match(*lists, embeddings_from=e, embeddings_to=u)
    m.rescore_to = "binary"
    with pytest.raises(ValueError, match="embeddings_from.*uint8.*no full-precision vectors"):
        m.match(*lists, embeddings_from=u, embeddings_to=u)
    # rescore_to at None: today's refusals of quantised arrays
    m.rescore_to = None
    with pytest.raises(ValueError, match="embeddings_to.*uint8.*no full-precision vectors"):
        m.match(*lists, embeddings_from=e, embeddings_to=u)
    m.binary, m.precision = None, "int8"
    with pytest.raises(ValueError, match="embeddings_to.*int8.*no full-precision vectors"):
        m.match(*lists, embeddings_from=e, embeddings_to=e.astype(np.int8))


def test_dense_match_job_refusals_need_no_device():
    """handles as DenseMatchJob reads them; every refusal comes before the first allocation (ctx=None)"""
    from polyfuzz_amd import _lib, pipeline

    def handle(n, dim, dtype):
        h = _lib.DeviceDense.__new__(_lib.DeviceDense)
        h.ctx, h.h, h.n, h.dim, h.dtype, h.normalize = None, None, n, dim, dtype, True
        return h
    f_a, q_a, b_a = (handle(10, 64, t) for t in ("float32", "int8", "binary"))
    q_b, b_b, h_b = (handle(50, 64, t) for t in ("int8", "binary", "float16"))
    with pytest.raises(ValueError, match="float32 form"):                           # a non-float32 rescore_from: today's words
        pipeline.DenseMatchJob(None, b_a, b_b, top_n=4, rescore_multiplier=4, rescore_from=b_a, rescore_to=b_b)
    with pytest.raises(ValueError, match="float32 form"):
        pipeline.DenseMatchJob(None, q_a, q_b, top_n=4, rescore_multiplier=4, rescore_from=q_a, rescore_to=q_b)
    with pytest.raises(ValueError, match="float32 form"):                           # bits after an int8 search: no such pair
        pipeline.DenseMatchJob(None, q_a, q_b, top_n=4, rescore_multiplier=4, rescore_from=f_a, rescore_to=b_b)
    with pytest.raises(ValueError, match="float32 form"):                           # a 16-bit to-side
        pipeline.DenseMatchJob(None, handle(10, 64, "float16"), h_b, top_n=4, rescore_multiplier=4, rescore_from=f_a, rescore_to=h_b)
    with pytest.raises(ValueError, match="float32 form"):                           # another shape
        pipeline.DenseMatchJob(None, b_a, b_b, top_n=4, rescore_multiplier=4, rescore_from=f_a, rescore_to=handle(49, 64, "int8"))
    with pytest.raises(ValueError, match="rescore_from and rescore_to"):
        pipeline.DenseMatchJob(None, b_a, b_b, top_n=4, rescore_multiplier=4, rescore_from=f_a)
    with pytest.raises(ValueError, match="without a rescore_multiplier"):
        pipeline.DenseMatchJob(None, b_a, b_b, top_n=4, rescore_from=f_a, rescore_to=b_b)
    with pytest.raises(ValueError, match="1024"):
        pipeline.DenseMatchJob(None, b_a, handle(5000, 64, "binary"), top_n=300, rescore_multiplier=4, rescore_from=f_a,
                               rescore_to=handle(5000, 64, "int8"))
    assert "MIXED_RESCORE_PAIRS" in inspect.getsource(pipeline.DenseMatchJob.__init__)


def test_mixed_rescore_kernel_budget():
    """four instances (int8 / bits x the from-row in LDS or re-read from L2), each within k5_rescore_topn's LDS plan -- 8 KiB of keys
    + 16 KiB of the row, or the keys alone --, no scratch, and few enough registers for four workgroups of 256 threads per CU.
    k5_rescore_topn itself stays two instances."""
    import kernel_budget
    from polyfuzz_amd import _build
    for exe in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(kernel_budget.LLVM, exe)):
            pytest.skip(f"{exe} not in {kernel_budget.LLVM}")
    md = kernel_budget.kernel_metadata(_build.build())
    pretty = dict(zip(md, kernel_budget.demangled(list(md))))
    hits = {pretty[k].split("(")[0]: v for k, v in md.items() if "k5_mixed_rescore" in pretty[k]}
    assert sorted(hits) == [f"void pfz::k5_mixed_rescore<{b}, {lds}>" for b in ("false", "true") for lds in ("false", "true")], sorted(hits)
    for name, k in hits.items():
        if name.endswith("true>"):
            assert k["lds"] == 8192 + 16384, (name, k)
        else:
            assert k["lds"] <= 8192 + 16, (name, k)
        assert k["scratch"] == 0 and k["vgpr"] <= 128, (name, k)
    assert not any("k5_rescore_topn" in n for n in hits)
    assert sum("k5_rescore_topn" in p for p in pretty.values()) == 2
