"""The 1-bit dense path (packed binary embeddings, Hamming top-n) as far as it can be held without a GPU: the C ABI declares
and binds its entry point, the Python doors validate before any device call (ctx=None: a device call would fail with
AttributeError, not ValueError), `Embeddings.binary` is validated when set and kept through pickling, the older doors still
refuse the name, and the numpy oracle the GPU tests are held to (tests/test_hamming_gpu.py imports it from here) is checked
against hand-made cases."""
import os
import pickle
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the oracle ---------------------------------------------------------------------------------------------------------
def pack(x):
    """float rows -> np.packbits(x > 0): bit k of a row is bit 7 - k % 8 of byte k // 8, the last byte padded with zeros"""
    return np.packbits(np.asarray(x) > 0, axis=1)


def ubinary(packed):
    """sentence-transformers' "binary" (int8 = ubinary - 128) -> "ubinary" (uint8); uint8 rows as they are"""
    packed = np.asarray(packed)
    if packed.dtype == np.int8:
        return (packed.astype(np.int16) + 128).astype(np.uint8)
    assert packed.dtype == np.uint8
    return packed


def hamming(a, b):
    """h[i, j] = differing bits of the packed uint8 rows a[i], b[j] (popcount through np.unpackbits)"""
    sa, sb = (2.0 * np.unpackbits(m, axis=1).astype(np.float64) - 1.0 for m in (a, b))      # +-1: sa . sb = bits - 2 h, exact
    return ((sa.shape[1] - sa @ sb.T) / 2).astype(np.int64)


def scores(a, b, d, normalize=True):
    """float32 score matrix of packed rows of d bits: float32(d - 2 h) / float32(d), or without normalisation float32(d - 2 h)"""
    dot = (d - 2 * hamming(a, b)).astype(np.float32)
    return dot / np.float32(d) if normalize else dot


def topn(s, ntop, lower_bound=0.0, exclude_diag=False, diag_offset=0):
    """K5's matching rules on a float32 score matrix: strictly above max(lower_bound, 0), score descending, column ascending,
    the diagonal j == i + diag_offset left out on request; (index -1, value 0) where a row runs out."""
    n, m = s.shape
    idx = np.full((n, ntop), -1, np.int32)
    val = np.zeros((n, ntop), np.float32)
    lb = np.float32(max(lower_bound, 0.0))
    cols = np.arange(m)
    for i in range(n):
        keep = s[i] > lb
        if exclude_diag:
            keep &= cols != i + diag_offset
        c = cols[keep]
        order = c[np.lexsort((c, -s[i, c].astype(np.float64)))][:ntop]
        idx[i, :len(order)] = order
        val[i, :len(order)] = s[i, order]
    return idx, val


def hamming_topn(a, b, d, ntop, lower_bound=0.0, exclude_diag=False, normalize=True):
    return topn(scores(ubinary(a), ubinary(b), d, normalize), ntop, lower_bound, exclude_diag)


def test_oracle_on_hand_made_rows():
    x = np.array([[1.0, -1.0, 0.5, 0.0, -0.0, np.nan, 2.0, 3.0, 1.0, -2.0]], np.float32)
    p = pack(x)
    assert p.dtype == np.uint8 and p.tolist() == [[0b10100011, 0b10000000]]          # NaN, 0.0 and -0.0 give 0; MSB first
    a = np.array([[0b11110000, 0b00000001]], np.uint8)
    b = np.array([[0b11110000, 0b00000001], [0b00001111, 0b11111110], [0b11110001, 0b00000001], [0b11110000, 0b00000000]], np.uint8)
    assert hamming(a, b).tolist() == [[0, 16, 1, 1]]
    s = scores(a, b, 16)
    assert s.dtype == np.float32 and s.tolist() == [[1.0, -1.0, 0.875, 0.875]]
    assert scores(a, b, 16, normalize=False).tolist() == [[16.0, -16.0, 14.0, 14.0]]
    assert scores(a, b, 12)[0, 2] == np.float32(10) / np.float32(12)                 # one correctly rounded fp32 division
    idx, val = topn(s, 4)
    assert idx.tolist() == [[0, 2, 3, -1]] and val.tolist() == [[1.0, 0.875, 0.875, 0.0]]          # ties: column ascending
    idx, val = topn(s, 2, lower_bound=0.875)
    assert idx.tolist() == [[0, -1]]                                                  # the bound is strict
    idx, _ = topn(s, 2, exclude_diag=True)
    assert idx.tolist() == [[2, 3]]
    idx, _ = topn(np.array([[-0.5, 0.0]], np.float32), 1, lower_bound=-1.0)
    assert idx.tolist() == [[-1]]                                                     # non-positive scores are no match


def test_binary_and_ubinary_are_one_form_on_the_host():
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(1)
    u = rng.integers(0, 256, (7, 12), dtype=np.uint8)
    b = (u.astype(np.int16) - 128).astype(np.int8)                                    # sentence-transformers' "binary"
    np.testing.assert_array_equal(_lib.ubinary_rows(b), u)
    np.testing.assert_array_equal(_lib.ubinary_rows(u), u)
    np.testing.assert_array_equal(ubinary(b), u)
    assert _lib.ubinary_rows(b).dtype == np.uint8 and _lib.ubinary_rows(b[:, ::2]).flags.c_contiguous
    np.testing.assert_array_equal(_lib.ubinary_rows(b[:, ::2]), u[:, ::2])
    np.testing.assert_array_equal(hamming(ubinary(b), u), hamming(u, u))
    for bad in (u.astype(np.int16), u.astype(np.float32), u.astype(bool)):
        with pytest.raises(ValueError, match="uint8 or an int8"):
            _lib.ubinary_rows(bad)


# ---- the ABI and the doors ----------------------------------------------------------------------------------------------
def test_header_and_ctypes_table_hold_the_bit_entry_point():
    from polyfuzz_amd import _lib
    src = open(os.path.join(REPO, "include", "polyfuzz_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+pfz_dense_upload1\s*\(([^)]*)\)", src)
    assert m and len(m.group(1).split(",")) == 7, m
    assert re.search(r"#define\s+PFZ_DENSE_B1\s+4\b", src)
    assert "pfz_dense_upload1" in _lib.SIGNATURES and len(_lib.SIGNATURES["pfz_dense_upload1"][1]) == 7
    # a door of its own: the vocabulary of `compute_dtype` / `precision` has not grown
    assert _lib.OPERAND_TYPES == ("float32", "float16", "bfloat16", "int8")
    assert "binary" not in _lib._OPERANDS and _lib.DENSE_DTYPES == {"float32": 0, "float16": 1, "bfloat16": 2}
    assert _lib.BINARY == "binary" and _lib.BINARY_FORMS == ("binary", "ubinary")


def test_the_library_exports_the_entry_point_and_its_kernels():
    import ctypes
    from polyfuzz_amd import _build, _lib
    if _build.is_stale():
        _build.build()
    _lib.load()
    assert hasattr(ctypes.CDLL(_lib.lib_path()), "pfz_dense_upload1")
    blob = open(_build.LIB_PATH, "rb").read()
    assert b"k5_hamming_panel" in blob and b"k5_pack_signs" in blob


def test_the_doors_validate_before_any_device_call():
    from polyfuzz_amd import _lib
    D = _lib.DeviceDense
    for bad in (np.zeros((2, 2), np.int16), np.zeros((2, 2), np.int64), np.zeros((2, 2), bool), np.zeros((2, 2), np.uint16)):
        with pytest.raises(ValueError, match="binary vectors are packed uint8 / int8 rows or a float array"):
            D.upload_bits(None, bad)
        with pytest.raises(ValueError, match="binary vectors"):
            _lib.dense_hamming_topn_host(None, bad, bad, 1, 0.0)
    for flat in (np.zeros(4, np.uint8), np.zeros(4, np.float32), np.zeros((2, 2, 2), np.int8)):
        with pytest.raises(ValueError, match="2-D"):
            D.upload_bits(None, flat)
    # the older doors still refuse the name and the unsigned bytes
    for bad in ("binary", "ubinary"):
        with pytest.raises(ValueError, match="precision"):
            _lib.check_precision(bad)
        with pytest.raises(ValueError, match="compute_dtype"):
            _lib.check_compute_dtype(bad)
        with pytest.raises(ValueError, match="operand must be one of"):
            D.upload_as(None, np.zeros((2, 2), np.float32), bad)
    with pytest.raises(ValueError, match="unsigned"):
        D.upload_int8(None, np.zeros((2, 2), np.uint8))
    assert _lib.check_binary(None) is None and _lib.check_binary("binary") == "binary" and _lib.check_binary("ubinary") == "ubinary"
    for bad in ("int8", "BINARY", 1, True, "", np.uint8):
        with pytest.raises(ValueError, match="binary must be None or one of"):
            _lib.check_binary(bad)
    # the rescored one-shot names the new coarse type, and still refuses what has nothing to rescore
    assert _lib.RESCORE_COARSE == ("int8", "float16", "bfloat16", "binary")
    f = np.ones((3, 8), np.float32)
    with pytest.raises(ValueError, match="coarse"):
        _lib.dense_rescored_topn_host(None, f, f, 1, 0.0, coarse="ubinary", multiplier=2)
    with pytest.raises(ValueError, match="rescore_multiplier"):
        _lib.dense_rescored_topn_host(None, f, f, 1, 0.0, coarse="binary", multiplier=0)
    with pytest.raises(ValueError, match="float32 / float64"):                        # packed rows: no full-precision vectors
        _lib.dense_rescored_topn_host(None, np.zeros((3, 1), np.uint8), f, 1, 0.0, coarse="binary", multiplier=2)


def test_embeddings_binary_attribute():
    from polyfuzz_amd.models import Embeddings
    m = Embeddings(min_similarity=0.1, top_n=3, cosine_method="hip")
    assert m.binary is None and Embeddings().binary is None
    for bad in ("int8", "BINARY", 1, True):
        with pytest.raises(ValueError, match="binary"):
            m.binary = bad
    assert m.binary is None
    with pytest.raises(ValueError, match="precision"):                                # `precision` still refuses the name
        m.precision = "binary"
    with pytest.raises(ValueError, match="compute_dtype"):
        m.compute_dtype = "ubinary"
    for name in ("binary", "ubinary"):
        m.binary = name
        m2 = pickle.loads(pickle.dumps(m))
        assert m2.binary == name and m2.precision is None and m2.compute_dtype is None and m2.top_n == 3 and m2._dev_to is None
    m.binary = None
    assert m.binary is None
    state = m.__getstate__()
    del state["_binary"]                                      # pickled before the attribute existed
    old = Embeddings.__new__(Embeddings)
    old.__setstate__(state)
    assert old.binary is None and old.precision is None


def test_embeddings_refuses_binary_with_another_operand_type():
    """raised by match() before anything is uploaded: no device is needed to see it"""
    from polyfuzz_amd.models import Embeddings
    e = np.ones((2, 8), np.float32)
    for attr, value in (("precision", "int8"), ("compute_dtype", "float16"), ("compute_dtype", "bfloat16")):
        m = Embeddings(min_similarity=0.0, cosine_method="hip")
        m.binary = "ubinary"
        setattr(m, attr, value)
        with pytest.raises(ValueError, match="binary.*precision.*compute_dtype"):
            m.match(["a", "b"], ["c", "d"], embeddings_from=e, embeddings_to=e)
    # rescoring needs the float vectors: packed arrays of either spelling are refused, on either side, before any upload
    m = Embeddings(min_similarity=0.0, cosine_method="hip")
    m.binary = "binary"
    m.rescore_multiplier = 4
    for packed in (np.zeros((2, 1), np.uint8), np.zeros((2, 1), np.int8)):
        with pytest.raises(ValueError, match="embeddings_to.*no full-precision vectors"):
            m.match(["a", "b"], ["c", "d"], embeddings_from=e, embeddings_to=packed)
        with pytest.raises(ValueError, match="embeddings_from.*no full-precision vectors"):
            m.match(["a", "b"], ["c", "d"], embeddings_from=packed, embeddings_to=e)
