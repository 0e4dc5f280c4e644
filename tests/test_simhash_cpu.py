"""K25 (pfz_simhash, _lib.simhash, models.SimHash) without a GPU: the oracle (tests/simhash_oracle.py) held to the issue's known
answers; the rule of polyfuzz_amd/csrc/k25_core.h compiled for the host (tests/k25_core_host.cpp) and held to the oracle -- it
walks a string in the kernel's steps through the functions the kernel calls --, its cleaning to TFIDF's _clean_string; the matcher's refusals with the device patched away; the symbol; the kernels' budget."""
import ctypes
import inspect
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from tests import simhash_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


# ---- the oracle against the known answers -----------------------------------------------------------------------------------------

KNOWN = [  # string, keywords, fingerprint, windows, tied votes
    ("abc", {}, "0b1873a968eedcd3", 1, None),
    ("apple", {}, "502fbe72e608c174", 3, None),
    ("similarity", {}, "bc2880221043c343", 8, 17),
    ("Apple  Inc.", {}, "402e92422208c030", 4, 31),
    ("abcabc", {}, "0a08738948e098d1", 4, None),
    ("ab", {}, "00" * 8, 0, None),
    ("", {}, "00" * 8, 0, None),
    ("apple", {"bits": 128}, "502fbe72e608c174c70559cc497eb8b7", 3, None),
    ("abc", {"bits": 192}, "0b1873a968eedcd34d959ecb97209c0c6c421b9ff8d4051e", 1, None),
    ("Apple Inc", {"n_gram_range": (2, 4), "clean": False, "remove_space": False}, "3a3ea955fa1566b7", 21, None),
    ("Zażółć gęślą", {"clean": False, "remove_space": False}, "01d00841dfa28e00", 10, None),
]


def test_oracle_reproduces_the_known_answers():
    assert f"{O.mix(O.G):016x}" == "e220a8397b1dcdaf"
    assert f"{O.window_hash([ord(c) for c in 'abc']):016x}" == "cb3b771695ce18d0"
    assert int(O.mix_np(np.array([O.G, 0, O.M], np.uint64))[0]) == O.mix(O.G) and int(O.mix_np(np.array([O.M], np.uint64))[0]) == O.mix(O.M)
    for string, kw, want, windows, ties in KNOWN:
        code, n, votes = O.fingerprint(string, **kw)
        assert (code.tobytes().hex(), n) == (want, windows), string
        if ties is not None:
            assert int((votes == 0).sum()) == ties, string
    # the first 64 bits of a wider fingerprint are the 64-bit one; the layout is packbits of (V > 0)
    wide, _, votes = O.fingerprint("similarity", bits=1024)
    assert wide[:8].tobytes().hex() == "bc2880221043c343" and (np.packbits(votes > 0) == wide).all() and len(wide) == 128


# ---- k25_core.h on the host -------------------------------------------------------------------------------------------------------

def _host_program():
    exe = os.path.join(REPO, "oracle", "_build", "k25_core_host")
    src = [os.path.join(HERE, "k25_core_host.cpp"), os.path.join(REPO, "polyfuzz_amd", "csrc", "k25_core.h")]
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=undefined,address",
                               "-fno-sanitize-recover=all", src[0], "-o", exe])
    return exe


def _ask(text):
    out = subprocess.run([_host_program()], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return [ln for ln in out.stdout.split("\n") if ln]


def _command(string, lo, hi, clean, rs, bits):
    return f"S {lo} {hi} {int(clean)} {int(rs)} {bits} {len(string)} " + " ".join(f"{ord(c):x}" for c in string) + "\n"


def test_constants_and_known_answers_on_the_host():
    from polyfuzz_amd import _lib
    first = _ask("C\n")[0].split()
    assert first[:2] == ["e220a8397b1dcdaf", "cb3b771695ce18d0"]
    assert tuple(map(int, first[2:])) == (_lib.SIMHASH_MIN_BITS, _lib.SIMHASH_MAX_BITS, _lib.SIMHASH_MAX_GRAM) == (64, 1024, 8)
    text = ""
    for string, kw, _, _, _ in KNOWN:
        lo, hi = kw.get("n_gram_range", (3, 3))
        text += _command(string, lo, hi, kw.get("clean", True), kw.get("remove_space", True), kw.get("bits", 64))
    for (string, kw, want, windows, _), line in zip(KNOWN, _ask(text)):
        got = line.split()
        assert (got[0], int(got[1])) == (want, windows), string


RANGES = [(1, 1), (3, 3), (2, 4), (8, 8)]
WIDTHS = [64, 128, 1024]


def _random_strings():
    """500 strings over a small alphabet with spaces and punctuation; every length 0 .. 200 occurs"""
    rng = np.random.default_rng(25)
    alphabet = list("abcAB19 ") + [" ", " ", ".", ",", "-", "\t", "é", "Z"]
    lengths = list(range(201)) + rng.integers(0, 201, 299).tolist()
    return ["".join(rng.choice(alphabet, n)) for n in lengths]


def test_host_program_equals_the_oracle():
    from polyfuzz_amd.models._tfidf import _clean_string
    from tests import simhash_cases
    strings = _random_strings()
    assert len(strings) == 500 and sorted(set(map(len, strings))) == list(range(201))
    # ... and the strings that put a pending space in front of a full step (the program walks in the kernel's steps, through the
    # functions the kernel calls, on a line of the kernel's size: a symbol too many is an error of the sanitizer's)
    strings = strings + list(simhash_cases.boundary_strings())
    cases = [(s, lo, hi, clean, rs) for s in strings for lo, hi in RANGES for clean in (True, False) for rs in (True, False)]
    lines = _ask("".join(_command(s, lo, hi, clean, rs, bits) for s, lo, hi, clean, rs in cases for bits in WIDTHS))
    assert len(lines) == len(cases) * len(WIDTHS)
    windowless = with_ties = spaces_dropped = 0
    for k, (s, lo, hi, clean, rs) in enumerate(cases):
        g = O.hashes(s, (lo, hi), clean, rs)
        kept = _clean_string(s) if clean else s
        symbols = ",".join(f"{ord(c):x}" for c in kept) or "-"
        for j, bits in enumerate(WIDTHS):
            votes = O.votes(g, bits)
            code, n, sym = lines[k * len(WIDTHS) + j].split()
            assert code == np.packbits(votes > 0).tobytes().hex() and int(n) == len(g), (s, lo, hi, clean, rs, bits)
            assert sym == symbols, (s, clean)                      # the cleaning rule against _clean_string
            with_ties += int(len(g) > 0 and (votes == 0).any())
        windowless += int(len(g) == 0)
        spaces_dropped += int(rs and len(g) < len(O.hashes(s, (lo, hi), clean, False)))
    assert windowless > 100 and with_ties > 1000 and spaces_dropped > 1000      # the cases reach the rules they are there for


# ---- refusals before any device call ----------------------------------------------------------------------------------------------

def _no_device(monkeypatch):
    from polyfuzz_amd import _lib

    def reached(*a, **k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(_lib.Context, "default", classmethod(reached))
    monkeypatch.setattr(_lib.DeviceStrings, "upload_packed", classmethod(reached))
    monkeypatch.setattr(_lib.DeviceStrings, "upload_direct", classmethod(reached))


@pytest.mark.parametrize("bits", [0, 32, 96, 1088, -64, 64.0, True, None, "64"])
def test_bad_bits_are_refused(monkeypatch, bits):
    from polyfuzz_amd.models import SimHash
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match="bits"):
        SimHash(bits=bits)
    m = SimHash()
    m.bits = bits                                                  # set behind the constructor's back: refused at the call
    for call in (lambda: m.join(["abc", "abd"], max_distance=3), lambda: m.components(["abc"], 0.9), lambda: m.fingerprints(["abc"]),
                 lambda: m.match(["abc"], ["abd"])):
        with pytest.raises(ValueError, match="bits"):
            call()


@pytest.mark.parametrize("grams", [(0, 3), (4, 3), (3, 9), (3,), 3, (1.0, 2), (True, 2), None])
def test_bad_n_gram_ranges_are_refused(monkeypatch, grams):
    from polyfuzz_amd.models import SimHash
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match="n_gram_range"):
        SimHash(n_gram_range=grams)
    m = SimHash()
    m.n_gram_range = grams
    for call in (lambda: m.join(["abc", "abd"], max_distance=3), lambda: m.components(["abc"], 0.9), lambda: m.fingerprints(["abc"])):
        with pytest.raises(ValueError, match="n_gram_range"):
            call()


def test_thresholds_and_index_are_refused(monkeypatch):
    from polyfuzz_amd.models import Hamming, SimHash
    _no_device(monkeypatch)
    m = SimHash()
    names = ["abc", "abd"]
    for kw in ({}, {"min_similarity": 0.9, "max_distance": 3}):
        with pytest.raises(ValueError, match="exactly one"):
            m.join(names, **kw)
        with pytest.raises(ValueError, match="exactly one"):
            m.components(names, **kw)
    for bad in (-1, 65, 3.0, True):
        with pytest.raises(ValueError, match="max_distance"):
            m.join(names, max_distance=bad)
    for bad in (1.5, -0.1, float("nan")):
        with pytest.raises(ValueError):
            m.components(names, bad)
    assert m.index == "auto" and Hamming().index is None           # a new class with its own default; Hamming's stays
    for bad in ("Blocks", "tiles", "", 1, True, False, 0, b"auto", ["auto"]):
        with pytest.raises(ValueError, match="index"):
            m.index = bad
        assert m.index == "auto"
    m.index = "blocks"
    with pytest.raises(ValueError, match='index = "blocks"'):      # 65 blocks for 64 bits
        m.join(names, max_distance=64)
    for good in ("blocks", None, "auto"):
        m.index = good
        back = pickle.loads(pickle.dumps(m))
        assert back.index == good and type(back) is SimHash and back.bits == 64 and back.n_gram_range == (3, 3)
    with pytest.raises(AssertionError, match="the device was reached"):      # a good call goes on to the device
        m.join(names, max_distance=3)


def test_matcher_surface():
    from polyfuzz_amd import linkage, models
    from polyfuzz_amd.models import SimHash
    assert "SimHash" in models.__all__ and issubclass(SimHash, models.BaseMatcher)
    sig = inspect.signature(SimHash.__init__).parameters
    assert list(sig) == ["self", "bits", "n_gram_range", "clean_string", "remove_space_ngrams", "model_id"]
    assert [sig[k].default for k in list(sig)[1:]] == [64, (3, 3), True, True, None]
    assert SimHash().type == "Embeddings"
    join = inspect.signature(SimHash.join).parameters
    assert list(join) == ["self", "from_list", "to_list", "min_similarity", "max_distance"] and join["max_distance"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(SimHash.components).parameters) == ["self", "strings", "min_similarity", "max_distance"]
    assert list(inspect.signature(SimHash.match).parameters) == ["self", "from_list", "to_list", "top_n"]
    assert "SimHash" in linkage.connected_components.__doc__


def test_join_maps_compact_rows_to_positions(monkeypatch):
    """the device patched away: rows of the handle are positions among the strings WITH a window"""
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import SimHash

    class Dev:
        def __init__(self, n):
            self.n, self.dim, self.dtype = n, 64, _lib.BINARY
    names = ["ab", "abcd", "", "abce", "abcf", "a"]
    row = np.array([-1, 0, -1, 1, 2, -1], np.int32)
    seen = []
    monkeypatch.setattr(_lib.Context, "default", classmethod(lambda cls: "ctx"))
    monkeypatch.setattr(SimHash, "_codes", lambda self, strings, want_bytes=False: (Dev(3), row, np.maximum(row + 1, 0)))
    monkeypatch.setattr(_lib, "hamming_join_indexed", lambda *a, **k: seen.append((a, k)) or (
        np.array([0, 2, 3, 3], np.int64), np.array([1, 2, 2], np.int32), np.array([1, 3, 0], np.int32), {"pairs": 3, "route": 0}))
    monkeypatch.setattr(_lib, "hamming_components_indexed", lambda *a, **k: seen.append((a, k)) or (np.array([0, 0, 2], np.int32), 1, 2, {"route": 0}))
    m = SimHash()
    frame = m.join(names, max_distance=3)
    assert list(frame.columns) == ["From", "To", "Similarity", "Distance"]
    assert frame["From"].tolist() == ["abcd", "abcd", "abce"] and frame["To"].tolist() == ["abce", "abcf", "abcf"]
    assert frame["Distance"].tolist() == [1, 3, 0] and frame["Similarity"].tolist() == [float(np.float32(62) / np.float32(64)), float(np.float32(58) / np.float32(64)), 1.0]
    assert m.last_counts == {"pairs": 3, "route": 0, "windowless": 3} and set(m.last_timings) == {"fingerprint", "device", "frame"}
    assert seen[0][0][2] is None and seen[0][0][3] == 3 and seen[0][1] == {"auto": True, "counters": True}
    label = m.components(names, max_distance=3)
    assert label.tolist() == [0, 1, 2, 1, 4, 5] and label.dtype == np.int32
    assert m.last_counts == {"pairs": 1, "components": 5, "route": 0, "windowless": 3}


# ---- the symbol, the binding, the kernels ---------------------------------------------------------------------------------------------

def test_symbol_declared_exported_and_in_the_table():
    from polyfuzz_amd import _build, _lib
    if _build.is_stale():
        _build.build()
    header = open(os.path.join(REPO, "include", "polyfuzz_hip.h")).read()
    so = ctypes.CDLL(_lib.lib_path())
    assert "int pfz_simhash(" in header and hasattr(so, "pfz_simhash") and "pfz_simhash" in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES["pfz_simhash"]
    decl = header[header.index("int pfz_simhash("):]
    assert restype is ctypes.c_int and len(argtypes) == 8 == len(decl[:decl.index(";")].split(","))
    assert argtypes[3] is ctypes.c_int32 and header.index("---- K25") > header.index("int pfz_hamming_index_plan(")
    assert list(inspect.signature(_lib.simhash).parameters) == ["ctx", "dev_strings", "params", "bits", "want_bytes"]
    assert inspect.signature(_lib.simhash).parameters["want_bytes"].default is False


def test_binding_refuses_before_the_library(monkeypatch):
    from polyfuzz_amd import _lib

    class Strings:
        n, h, char_width = 2, None, 4
    for bits in (0, 32, 96, 1088):
        with pytest.raises(ValueError, match="bits"):
            _lib.simhash(None, Strings(), _lib.TfidfParams(3, 3, 0, 1), bits)
    for lo, hi in ((0, 3), (4, 3), (3, 9)):
        with pytest.raises(ValueError, match="n_gram_range"):
            _lib.simhash(None, Strings(), _lib.TfidfParams(lo, hi, 0, 1), 64)
    with pytest.raises(ValueError, match="4-byte"):
        _lib.simhash(None, Strings(), _lib.TfidfParams(3, 3, 1, 1), 64)


def test_library_refuses_bad_arguments_without_a_device():
    """pfz_simhash checks its arguments before it touches the device: a NULL context is enough to ask"""
    from polyfuzz_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.pfz_simhash(None, None, ctypes.byref(_lib.TfidfParams(3, 3, 1, 1)), 64, ctypes.byref(h), None, None, None) == -1
    assert b"NULL" in lib.pfz_last_error() and not h.value


BUDGET = {  # kernel -> (registers per lane, LDS bytes): what the build reports, pinned
    "k25_fingerprint<1, 1>": (36, 1152),
    "k25_fingerprint<1, 2>": (40, 1152),
    "k25_fingerprint<1, 4>": (50, 1152),
    "k25_fingerprint<4, 1>": (30, 1152),
    "k25_fingerprint<4, 2>": (32, 1152),
    "k25_fingerprint<4, 4>": (44, 1152),
    "k25_compact": (12, 0),
}


def test_kernel_budget():
    """the k25_* kernels exist once each, without scratch, with the registers and the LDS line (4 waves x (8 + 64) words) pinned"""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_budget
    from polyfuzz_amd import _build
    for exe in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(kernel_budget.LLVM, exe)):
            pytest.skip(f"{exe} not in {kernel_budget.LLVM}")
    md = kernel_budget.kernel_metadata(_build.build())
    pretty = dict(zip(md, kernel_budget.demangled(list(md))))
    ours = {p: md[k] for k, p in pretty.items() if "pfz::k25_" in p}
    assert len(ours) == len(BUDGET), sorted(ours)
    for name, (vgpr, lds) in BUDGET.items():
        hits = [v for p, v in ours.items() if f"pfz::{name}(" in p]
        assert len(hits) == 1, (name, sorted(ours))
        k = hits[0]
        assert k["scratch"] == 0, (name, k)
        assert (k["vgpr"] + k.get("agpr", 0), k["lds"]) == (vgpr, lds), (name, k)
