"""K25 on the device: pfz_simhash's bytes, window counts and rows `==` the Python oracle (tests/simhash_oracle.py) on the edge
strings, list sizes, parameters and real names of tests/simhash_cases.py; and SimHash.join / .components / .match end to end on
3 000 company names against Hamming on the oracle's codes."""
import functools

import numpy as np
import pytest

from tests import simhash_cases as C
from tests import simhash_oracle as O

pytestmark = pytest.mark.gpu


def _device(ctx, strings, bits=64, grams=(3, 3), clean=True, remove_space=True):
    """_lib.simhash on the list as it is packed (no host cleaning): (bytes, windows, row, rows of the handle)"""
    from polyfuzz_amd import _lib
    dev = _lib.DeviceStrings.upload_packed(ctx, *_lib.pack_strings(list(strings)))
    params = _lib.TfidfParams(grams[0], grams[1], int(clean), int(remove_space))
    handle, row, windows, code = _lib.simhash(ctx, dev, params, bits, want_bytes=True)
    assert handle.dim == bits and handle.dtype == _lib.BINARY and handle.normalize is True
    assert code.shape == (len(strings), bits // 8) and code.dtype == np.uint8 and row.dtype == windows.dtype == np.int32
    return code, windows, row, handle.n


def _holds(ctx, strings, **kw):
    code, windows, row, n_rows = _device(ctx, strings, **kw)
    want = O.fingerprints(strings, kw.get("bits", 64), kw.get("grams", (3, 3)), kw.get("clean", True), kw.get("remove_space", True))
    assert np.array_equal(windows, want[1]), np.flatnonzero(windows != want[1])[:5]
    assert np.array_equal(code, want[0]), np.flatnonzero((code != want[0]).any(axis=1))[:5]
    assert np.array_equal(row, want[2]) and n_rows == int((want[1] > 0).sum())
    return want


def test_edge_strings(ctx):
    strings = C.edge_strings()
    code, windows, row, ties = _holds(ctx, strings)
    assert windows[:5].tolist() == [0, 0, 0, 1, 0] and windows[-2] == 0 and windows[-1] == 1 and (row[[0, 1, 2, 4]] == -1).all()
    assert code[5].tobytes().hex() == "402e92422208c030" and code[6].tobytes().hex() == "0a08738948e098d1" and ties[5] == 31
    assert not code[windows == 0].any()


@pytest.mark.parametrize("kw", [{}, {"bits": 128, "grams": (2, 4)}, {"remove_space": False, "grams": (1, 3)}, {"clean": False}],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()) or "defaults")
def test_pending_space_in_front_of_a_full_step(ctx, kw):
    strings = C.boundary_strings()
    _, windows, _, _ = _holds(ctx, strings, **kw)
    if not kw:
        assert windows[0] == 60 and windows[10] == 62      # 'x' + 62 / 63 spaces + 62 / 64 a's: the windows of the a's alone


@pytest.mark.parametrize("name", sorted(C.SMALL_LISTS))
def test_small_lists_and_windowless_places(ctx, name):
    strings = C.SMALL_LISTS[name]
    _, windows, row, _ = _holds(ctx, strings)
    if name == "all_windowless":
        assert (row == -1).all()
    if name == "none_windowless":
        assert row.tolist() == [0, 1, 2, 3]
    if name in ("start", "middle", "end"):
        assert int((windows == 0).sum()) == 1


@pytest.mark.parametrize("bits", [64, 128, 256, 1024])
def test_list_of_257_at_every_width(ctx, bits):
    code, windows, row, _ = _holds(ctx, C.list257(), bits=bits)
    assert row[-1] == -1 and row[0] == -1 and windows[256] == 0
    if bits > 64:
        assert np.array_equal(code[:, :8], O.fingerprints(C.list257())[0])      # the first 64 bits are the 64-bit fingerprint


@pytest.mark.parametrize("kw", [{"grams": (2, 4)}, {"grams": (1, 1)}, {"remove_space": False}, {"clean": False},
                                {"grams": (2, 4), "clean": False, "remove_space": False, "bits": 128}, {"grams": (8, 8), "bits": 256}],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_parameters(ctx, kw):
    _holds(ctx, C.list257(), **kw)


@pytest.mark.parametrize("kw", [{}, {"grams": (2, 4), "remove_space": True, "bits": 128}, {"grams": (1, 1), "bits": 256}],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()) or "defaults")
def test_four_byte_code_units(ctx, kw):
    from polyfuzz_amd import _lib
    assert _lib.pack_strings(list(C.WIDE))[2] == 4
    kw = {"remove_space": False, **kw, "clean": False}
    code, windows, _, _ = _holds(ctx, C.WIDE, **kw)
    if kw.get("bits", 64) == 64 and kw.get("grams", (3, 3)) == (3, 3):
        assert code[0].tobytes().hex() == "01d00841dfa28e00" and windows[0] == 10
    with pytest.raises(_lib.PfzError):                            # the library refuses to clean 4-byte units
        dev = _lib.DeviceStrings.upload_packed(ctx, *_lib.pack_strings(list(C.WIDE)))
        h = _lib.ctypes.c_void_p()
        row = np.empty(len(C.WIDE), np.int32)
        _lib.check(ctx.lib.pfz_simhash(ctx.h, dev.h, _lib.ctypes.byref(_lib.TfidfParams(3, 3, 1, 1)), 64, _lib.ctypes.byref(h), _lib._ptr(row),
                                       None, None))


def test_wide_strings_are_cleaned_on_the_host(ctx):
    from polyfuzz_amd.models import SimHash
    m = SimHash()
    got = m.fingerprints(list(C.WIDE))
    assert np.array_equal(got, O.fingerprints(C.WIDE)[0]) and m.last_counts["windowless"] == int((O.fingerprints(C.WIDE)[1] == 0).sum())


def test_one_string_of_9000_characters(ctx):
    rng = np.random.default_rng(9)
    long = "".join(rng.choice(list("abcdefgh  ,.XYZ09"), 9000))
    for kw in ({}, {"bits": 256, "grams": (2, 4)}, {"clean": False, "remove_space": False}):
        _, windows, _, _ = _holds(ctx, ["abc", long, "ab"], **kw)
        assert windows[1] > 4000


def test_library_refusals_on_the_device(ctx):
    from polyfuzz_amd import _lib
    dev = _lib.DeviceStrings.upload_packed(ctx, *_lib.pack_strings(["abc", "abd"]))
    row = np.empty(2, np.int32)
    for bits, lo, hi in ((0, 3, 3), (32, 3, 3), (96, 3, 3), (1088, 3, 3), (64, 0, 3), (64, 4, 3), (64, 3, 9)):
        h = _lib.ctypes.c_void_p()
        rc = ctx.lib.pfz_simhash(ctx.h, dev.h, _lib.ctypes.byref(_lib.TfidfParams(lo, hi, 1, 1)), bits, _lib.ctypes.byref(h), _lib._ptr(row), None, None)
        assert rc == -1 and not h.value, (bits, lo, hi)


# ---- real names -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _names_oracle():
    """the oracle on the first 3 000 company names, computed once: (names, codes, windows, row, ties, positions with a window)"""
    names = list(C.names())
    code, windows, row, ties = O.fingerprints(names)
    for a in (code, windows, row, ties):
        a.setflags(write=False)
    return names, code, windows, row, ties, np.flatnonzero(windows > 0)


@functools.lru_cache(maxsize=None)
def _names_pairs(hmax=3):
    """the oracle's pairs i < j among the names with a window, as positions in the list: (rows, cols, distances)"""
    _, code, _, _, _, pos = _names_oracle()
    h = C.popcounts(code[pos], code[pos])
    r, c = np.nonzero(np.triu(h <= hmax, 1))
    return pos[r], pos[c], h[r, c]


def test_real_names_fingerprints(ctx):
    names, code, windows, row, ties, pos = _names_oracle()
    assert int((windows == 0).sum()) == 5 and int((ties > 0).sum()) == 1453      # the tie rule and the compaction meet real data
    got = _device(ctx, names)
    assert np.array_equal(got[0], code) and np.array_equal(got[1], windows) and np.array_equal(got[2], row) and got[3] == len(pos) == 2995


@pytest.mark.parametrize("index", [None, "blocks", "auto"])
def test_join_of_real_names(ctx, index):
    from polyfuzz_amd.models import Hamming, SimHash
    names, code, _, _, _, pos = _names_oracle()
    rows, cols, dist = _names_pairs()
    # 240 pairs, 201 of them equal fingerprints (the 5 all-zero codes of the windowless names would add 10 more: they are no pairs)
    assert (len(rows), int((dist == 0).sum())) == (240, 201)
    m = SimHash()
    assert m.index == "auto"
    m.index = index
    frame = m.join(names, max_distance=3)
    assert list(frame.columns) == ["From", "To", "Similarity", "Distance"] and len(frame) == len(rows) > 0
    assert frame["From"].tolist() == [names[i] for i in rows] and frame["To"].tolist() == [names[j] for j in cols]
    assert frame["Distance"].tolist() == dist.tolist()
    h = Hamming()
    h.index = index
    want = h.join([names[i] for i in pos], max_distance=3, embeddings_from=np.ascontiguousarray(code[pos]))
    for col in want.columns:
        assert frame[col].tolist() == want[col].tolist(), col
    assert frame["Similarity"].dtype == np.float64 and m.last_counts["pairs"] == len(rows) and m.last_counts["windowless"] == 5
    assert set(m.last_timings) == {"fingerprint", "device", "frame"}
    by_similarity = m.join(names, min_similarity=0.9)               # 0.9 at 64 bits stands for 3 bits
    assert by_similarity["Distance"].tolist() == dist.tolist()


def test_join_of_two_lists(ctx):
    from polyfuzz_amd.models import Hamming, SimHash
    names, code, windows, _, _, _ = _names_oracle()
    a, b = names[:1500], names[1500:]
    pa, pb = np.flatnonzero(windows[:1500] > 0), np.flatnonzero(windows[1500:] > 0)
    h = C.popcounts(code[:1500][pa], code[1500:][pb])
    r, c = np.nonzero(h <= 6)
    assert len(r) > 0 and len(pa) < 1500 and len(pb) < 1500      # windowless names on both sides
    for index in (None, "auto"):
        m = SimHash()
        m.index = index
        frame = m.join(a, b, max_distance=6)
        assert frame["From"].tolist() == [a[i] for i in pa[r]] and frame["To"].tolist() == [b[j] for j in pb[c]]
        assert frame["Distance"].tolist() == h[r, c].tolist()
        assert m.last_counts["windowless"] == 5
    want = Hamming().join([a[i] for i in pa], [b[j] for j in pb], max_distance=6, embeddings_from=np.ascontiguousarray(code[:1500][pa]),
                          embeddings_to=np.ascontiguousarray(code[1500:][pb]))
    for col in want.columns:
        assert frame[col].tolist() == want[col].tolist(), col


@pytest.mark.parametrize("index", [None, "blocks", "auto"])
def test_components_of_real_names(ctx, index):
    from polyfuzz_amd import linkage
    from polyfuzz_amd.models import SimHash
    names, _, windows, _, _, _ = _names_oracle()
    rows, cols, _ = _names_pairs()
    want = C.union_find_labels(len(names), rows, cols)
    assert (want[windows == 0] == np.flatnonzero(windows == 0)).all()      # a windowless name is its own component
    m = SimHash()
    m.index = index
    label = m.components(names, max_distance=3)
    assert label.dtype == np.int32 and np.array_equal(label, want)
    assert m.last_counts["pairs"] == len(rows) and m.last_counts["components"] == len(np.unique(want)) and m.last_counts["windowless"] == 5
    assert np.array_equal(m.components(names, 0.9), want)
    if index == "auto":
        assert linkage.connected_components(names, SimHash(), 0.9) == linkage.dicts_from_labels(names, want)


def test_match_of_real_names(ctx):
    from polyfuzz_amd.models import Hamming, SimHash
    names, code, windows, _, _, pos = _names_oracle()
    with_window = [names[i] for i in pos]
    codes = np.ascontiguousarray(code[pos])
    m = SimHash()
    # the self-match: the row itself is left out
    frame = m.match(names, top_n=3)
    want = Hamming().match(with_window, embeddings_from=codes, top_n=3)
    assert list(frame.columns) == list(want.columns) == ["From", "To", "Similarity", "To_2", "Similarity_2", "To_3", "Similarity_3"]
    assert frame["From"].tolist() == names and len(frame) == len(names)
    for col in want.columns:
        assert frame[col].to_numpy()[pos].tolist() == want[col].tolist(), col
    none = np.flatnonzero(windows == 0)
    for col in want.columns[1:]:
        assert all(v is None or v == 0.0 for v in frame[col].to_numpy()[none].tolist()), col
    assert frame["To"].to_numpy()[none].tolist() == [None] * 5 and frame["Similarity"].to_numpy()[none].tolist() == [0.0] * 5
    windowless_names = {names[i] for i in none}
    assert not windowless_names & set(frame["To"].tolist())       # never chosen
    assert m.last_counts == {"windowless": 5} and set(m.last_timings) == {"fingerprint", "device", "frame"}
    # two lists
    a, b = names[:1500], names[1500:]
    pa, pb = np.flatnonzero(windows[:1500] > 0), np.flatnonzero(windows[1500:] > 0)
    frame = m.match(a, b, top_n=3)
    want = Hamming().match([a[i] for i in pa], [b[j] for j in pb], np.ascontiguousarray(code[:1500][pa]), np.ascontiguousarray(code[1500:][pb]), top_n=3)
    for col in want.columns:
        assert frame[col].to_numpy()[pa].tolist() == want[col].tolist(), col
    assert frame["To"].to_numpy()[windows[:1500] == 0].tolist() == [None] * int((windows[:1500] == 0).sum())
