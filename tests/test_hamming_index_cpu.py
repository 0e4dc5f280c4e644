"""K24 (pfz_hamming_join_indexed, pfz_hamming_components_indexed, pfz_hamming_index_plan, Hamming.index) without a GPU: the rule of
polyfuzz_amd/csrc/k24_core.h compiled for the host (tests/k24_core_host.cpp) and held to a numpy restatement; that restatement held
to the XOR / popcount oracle -- the rule loses nothing and repeats nothing; pairs built by hand; the plan entry; the matcher's gates
with the device patched away; the symbols; the kernels' budget."""
import ctypes
import inspect
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from tests import hamming_index_cases as C
from tests import hamming_join_cases as HJ

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


# ---- k24_core.h on the host ------------------------------------------------------------------------------------------------------

def _host_program():
    exe = os.path.join(REPO, "oracle", "_build", "k24_core_host")
    csrc = os.path.join(REPO, "polyfuzz_amd", "csrc")
    src = [os.path.join(HERE, "k24_core_host.cpp")] + [os.path.join(csrc, h) for h in ("k24_core.h", "k17_core.h", "k16_core.h")]
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=undefined,address",
                               "-fno-sanitize-recover=all", src[0], "-o", exe])
    return exe


def _ask(text):
    out = subprocess.run([_host_program()], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return [ln for ln in out.stdout.split("\n") if ln]


def test_constants_on_the_host():
    from polyfuzz_amd import _lib
    max_blocks, max_rows, ratio, piece = map(int, _ask("C\n")[0].split())
    assert (max_blocks, max_rows, piece) == (C.MAX_BLOCKS, 1 << 24, _lib.PAIR_SLICE)
    assert 1 <= ratio and ratio & (ratio - 1) == 0                       # a power of two
    assert ratio == _lib.hamming_index_plan(64, 3)["ratio"]


def test_block_bounds_on_the_host():
    asked = [(d, hmax) for d in range(1, 131) for hmax in range(d)]
    for d in (256, 768, 4104, (1 << 24) - 1):
        asked += [(d, hmax) for hmax in (0, 1, 2, 3, 6, 7, 31, 100, 205, 254, 255, 256, 300, d - 1) if hmax < d]
    asked += [(64, 64), (8, 9), (0, 0), (1 << 24, 3), (64, -1)]
    lines = _ask("".join(f"B {d} {hmax}\n" for d, hmax in asked))
    assert len(lines) == len(asked)
    n_yes = 0
    for (d, hmax), line in zip(asked, lines):
        got = list(map(int, line.split()))
        if not C.indexable(d, hmax):
            assert got == [0], (d, hmax)
            continue
        n_yes += 1
        bd = C.bounds(d, hmax)
        widths = np.diff(bd)
        assert got == [1, hmax + 1, int(widths.min()), int(widths.max())] + bd, (d, hmax)
        assert bd[0] == 0 and bd[-1] == d and widths.min() >= 1 and widths.max() - widths.min() <= 1
    assert n_yes > 8000 and any(not C.indexable(d, h) for d, h in asked)
    assert not C.indexable(4104, 410) and C.indexable(4104, 205) and C.indexable(64, 63) and not C.indexable(64, 64)


def _keys_on_host(x, d, hmax):
    text = f"K {d} {hmax} {len(x)} {x.shape[1]}\n" + "\n".join(" ".join(f"{v:02x}" for v in row) for row in x.tolist()) + "\n"
    return np.array([list(map(int, ln.split())) for ln in _ask(text)], np.uint64).reshape(len(x), hmax + 1)


@pytest.mark.parametrize("d,hmax", [(96, 4), (64, 63), (768, 3), (64, 0), (100, 6), (4104, 205), (64, 3), (13, 12), (40, 2)])
def test_block_keys_on_the_host(d, hmax):
    """blocks that straddle byte and dword borders (96 / 5: 19, 38, 57, 76), width 1, blocks wider than a key, a width that is no
    multiple of 8 -- the rows handed over have exactly ceil(d / 8) bytes, under the address sanitizer"""
    if (d, hmax) == (96, 4):
        assert C.bounds(96, 4) == [0, 19, 38, 57, 76, 96]
    rng = np.random.default_rng(d * 1000 + hmax)
    bits = rng.integers(0, 2, (24, d), dtype=np.uint8)
    bits[0], bits[1] = 0, 1
    x = np.packbits(bits, axis=1)
    assert x.shape[1] == (d + 7) // 8
    want = C.block_keys(x, d, hmax)
    assert (_keys_on_host(x, d, hmax) == want).all()
    widths = np.diff(C.bounds(d, hmax))
    assert (want[1] == np.array([(1 << min(int(w), 32)) - 1 for w in widths], np.uint64)).all() and not want[0].any()


def test_first_block_rule_and_probe_runs_on_the_host():
    rng = np.random.default_rng(241)
    text, want = "", []
    for _ in range(300):
        m = int(rng.integers(1, 9))
        ka, kb = rng.integers(0, 3, m), rng.integers(0, 3, m)
        b = int(rng.integers(0, m))
        text += f"F {m} {b}\n{' '.join(map(str, ka))}\n{' '.join(map(str, kb))}\n"
        want.append(str(int(C.first_block(ka, kb, b))))
    assert _ask(text) == want and "0" in want and "1" in want
    # the run of a probe in sorted keys: n_to rows of few distinct keys, so that buckets are long; the top key and block too
    text, want = "", []
    for n_to, m, top in ((1, 1, 0), (37, 3, 0), (50, 256, 0xffffffff)):
        keys = rng.integers(0, 4, (n_to, m)).astype(np.uint64)
        keys[keys == 3] = top
        s = np.sort(np.array([(b << 56) | (int(keys[j, b]) << 24) | j for b in range(m) for j in range(n_to)], np.uint64))
        for _ in range(12):
            b, i, self_join = int(rng.integers(0, m)), int(rng.integers(0, n_to)), int(rng.integers(0, 2))
            key = int(keys[i, b]) if rng.random() < 0.8 else 2 ** 31
            text += f"R {n_to} {m} {b} {key} {i} {self_join}\n{' '.join(map(str, s.tolist()))}\n"
            run = [p for p in range(len(s)) if int(s[p]) >> 56 == b and (int(s[p]) >> 24) & 0xffffffff == key
                   and (not self_join or int(s[p]) & 0xffffff > i)]
            got_p = (run[0], run[-1] + 1) if run else None
            want.append(got_p)
    for line, w in zip(_ask(text), want):
        p0, p1 = map(int, line.split())
        assert (p0, p1) == w if w else p0 == p1, (line, w)


# ---- the rule loses nothing and repeats nothing (numpy alone) -------------------------------------------------------------------

def _holds(x, y, d, hmax):
    checks, hits = C.rule(x, y, d, hmax)
    rows, cols, _ = C.oracle(x, y, hmax)
    pairs = [(i, j) for i, j, _ in hits]
    assert len(set(pairs)) == len(pairs)                                  # each pair in exactly one block
    assert sorted(pairs) == list(zip(rows.tolist(), cols.tolist()))       # and every pair of the oracle, no other
    return checks, len(hits)


@pytest.mark.parametrize("name,t", C.INDEXABLE)
def test_rule_equals_the_oracle_on_the_join_cases(name, t):
    x, y = HJ.lists(name)
    hmax = HJ.HMAX[name][t]
    assert C.indexable(HJ.bits(name), hmax)
    checks, hits = _holds(x, y, HJ.bits(name), hmax)
    assert checks == C.CHECKS[name][t] and hits == HJ.ORACLE_HITS[name][t][0] and C.all_pairs(x, y) == C.ALL_PAIRS[name]


def test_cases_that_have_no_index():
    for name, t in C.NOT_INDEXABLE:
        assert not C.indexable(HJ.bits(name), HJ.HMAX[name][t]) and HJ.HMAX[name][t] + 1 in (411, 821)
    assert len(C.INDEXABLE) == 10


def test_rule_on_the_planted_list():
    x, p = C.planted(), C.PLANTED
    checks, hits = _holds(x, None, p["d"], p["hmax"])
    h = HJ.distances_of(x)
    assert (checks, hits, C.all_pairs(x, None)) == (p["checks"], p["hits"], p["all"]) == (3075, 750, 8386560)
    assert (int((h == 3).sum()), int((h == 4).sum())) == (p["at_cutoff"], p["one_beyond"]) == (186, 218)


@pytest.mark.parametrize("name", C.SHAPES)
def test_rule_on_the_block_shapes(name):
    codes, d, hmax = C.shape(name)
    x = C.packed(codes)
    checks, hits = _holds(x, None, d, hmax)
    assert hits > 0 and len(x) == 512
    _holds(x[:100], np.ascontiguousarray(x[::-1]), d, hmax)
    if name == "768":       # pairs within the distance whose every difference lies behind a block's first 32 bits
        rows, cols, dist = C.oracle(x, None, hmax)
        k = C.block_keys(x, d, hmax)
        assert ((dist > 0) & (k[rows] == k[cols]).all(axis=1)).any()


def test_heavy_bucket_in_numpy():
    x = C.heavy()
    checks, hits = C.rule(x, None, 64, 3)
    assert hits and sum(1 for i, j, b in hits if b == 0) >= 244650 == 700 * 699 // 2 and checks >= 4 * 244650


def test_adversarial_pairs():
    x, why = C.adversarial64()
    keys = C.block_keys(x, 64, 3)
    h = HJ.distances_of(x)
    checks, hits = C.rule(x, None, 64, 3)
    by_pair = {(i, j): b for i, j, b in hits}
    for k, (what, dist, block) in enumerate(why):
        i, j = 2 * k, 2 * k + 1
        agree = [b for b in range(4) if keys[i, b] == keys[j, b]]
        assert h[i, j] == dist, what
        if block is None:
            assert agree == [] and (i, j) not in by_pair, what            # one bit in every block: a candidate nowhere
        elif dist == 0:
            assert agree == [0, 1, 2, 3] and by_pair[i, j] == 0, what      # equal codes: ONE hit, in block 0
        else:
            assert agree == [block] and by_pair[i, j] == block, what
    assert sum(1 for i, j in by_pair if j == i + 1 and i % 2 == 0) == 5
    y = C.adversarial768()
    k = C.block_keys(y, 768, 3)
    assert HJ.distances_of(y)[0, 1] == 3 and (k[0] == k[1]).all()         # agrees on every KEY, differs in block 1's tail
    checks, hits = C.rule(y, None, 768, 3)
    assert checks == 4 and hits == [(0, 1, 0)]
    checks, hits = C.rule(y, None, 768, 2)                                 # one bit too far: still a candidate, never a hit
    assert checks == 3 and hits == []


# ---- pfz_hamming_index_plan --------------------------------------------------------------------------------------------------------

def test_index_plan_against_numpy():
    from polyfuzz_amd import _lib
    for d, hmax in [(64, 3), (64, 0), (64, 63), (96, 4), (100, 6), (768, 3), (768, 38), (768, 255), (4104, 205), (1, 0), ((1 << 24) - 1, 255)]:
        plan = _lib.hamming_index_plan(d, hmax)
        widths = np.diff(C.bounds(d, hmax))
        assert (plan["blocks"], plan["min_block_bits"], plan["max_block_bits"]) == (hmax + 1, widths.min(), widths.max()), (d, hmax)
        assert 1 <= plan["ratio"] and plan["ratio"] & (plan["ratio"] - 1) == 0
    for d, hmax, word in [(4104, 410, "256"), (768, 256, "256"), (64, 64, "blocks"), (8, 8, "blocks")]:      # m > 256; hmax >= d
        with pytest.raises(_lib.PfzUnsupported, match=word) as e:
            _lib.hamming_index_plan(d, hmax)
        assert e.value.code == -4
    for d, hmax in [(0, 0), (1 << 24, 3), (64, -1), (64, 65), (True, 0), (64.0, 3), (64, 3.0)]:               # out of range
        with pytest.raises(ValueError):
            _lib.hamming_index_plan(d, hmax)
    lib = _lib.load()
    out = np.zeros(4, np.int64)
    assert lib.pfz_hamming_index_plan(64, 3, None) != 0                    # NULL
    for d, hmax in [(0, 0), (1 << 24, 3), (64, -1), (64, 65)]:
        assert lib.pfz_hamming_index_plan(d, hmax, out.ctypes.data_as(ctypes.c_void_p)) not in (0, -4)
    assert lib.pfz_hamming_index_plan(64, 64, out.ctypes.data_as(ctypes.c_void_p)) == -4 and not out.any()


# ---- the matcher's gates, the device patched away ------------------------------------------------------------------------------

def _codes():
    return ["a", "b", "c"], np.array([[0] * 8, [0] * 7 + [1], [255] * 8], np.uint8)


def _patched(monkeypatch):
    from polyfuzz_amd import _lib
    seen = []
    monkeypatch.setattr(_lib.Context, "default", classmethod(lambda cls: "ctx"))
    monkeypatch.setattr(_lib.DeviceDense, "upload_bits", classmethod(lambda cls, ctx, vec, normalize=True: ("handle", vec)))
    join = (np.array([0, 1, 1, 1], np.int64), np.array([1], np.int32), np.array([1], np.int32))
    monkeypatch.setattr(_lib, "hamming_join", lambda *a, **k: seen.append(("join", a, k)) or join + ({"pairs": 1},))
    monkeypatch.setattr(_lib, "hamming_components", lambda *a, **k: seen.append(("comp", a, k)) or (np.array([0, 0, 2], np.int32), 1, 2))
    monkeypatch.setattr(_lib, "hamming_join_indexed",
                        lambda *a, **k: seen.append(("join_indexed", a, k)) or join + ({"pairs": 1, "checks": 5, "route": 1},))
    monkeypatch.setattr(_lib, "hamming_components_indexed", lambda *a, **k: seen.append(("comp_indexed", a, k))
                        or (np.array([0, 0, 2], np.int32), 1, 2, {"checks": 5, "route": 1}))
    return seen


def test_index_none_calls_what_it_called_before(monkeypatch):
    from polyfuzz_amd.models import Hamming
    seen = _patched(monkeypatch)
    names, x = _codes()
    m = Hamming()
    assert m.index is None
    frame = m.join(names, max_distance=3, embeddings_from=x)
    assert frame["From"].tolist() == ["a"] and frame["To"].tolist() == ["b"] and frame["Distance"].tolist() == [1]
    m.join(names, names, 0.9, x, x)
    m.components(names, 0.9, embeddings=x)
    kinds = [s[0] for s in seen]
    assert kinds == ["join", "join", "comp"]
    assert seen[0][1][0] == "ctx" and seen[0][1][1][1] is x and seen[0][1][2] is None and seen[0][1][3] == 3 and seen[0][2] == {}
    assert len(seen[0][1]) == 4 and seen[1][1][2][1] is x and seen[1][1][3] == 3 and seen[1][2] == {}
    assert len(seen[2][1]) == 3 and seen[2][1][2] == 3 and seen[2][2] == {} and m.last_counts == {"pairs": 1, "components": 2}


@pytest.mark.parametrize("index", ["blocks", "auto"])
def test_index_routes_through_the_new_entries(monkeypatch, index):
    from polyfuzz_amd import linkage
    from polyfuzz_amd.models import Hamming
    seen = _patched(monkeypatch)
    names, x = _codes()
    m = Hamming()
    m.index = index
    frame = m.join(names, max_distance=3, embeddings_from=x)
    assert frame["Distance"].tolist() == [1] and m.last_counts == {"pairs": 1, "checks": 5, "route": 1}
    m.join(names, names, 0.9, x, x)
    label = m.components(names, 0.9, embeddings=x)
    assert label.tolist() == [0, 0, 2] and m.last_counts == {"pairs": 1, "components": 2, "checks": 5, "route": 1}
    assert linkage.connected_components(names, m, 0.9, embeddings=x) == linkage.dicts_from_labels(names, [0, 0, 2])
    assert [s[0] for s in seen] == ["join_indexed", "join_indexed", "comp_indexed", "comp_indexed"]
    for s in seen:
        assert s[2] == {"auto": index == "auto", "counters": True} and s[1][-1] == 3
    assert seen[0][1][2] is None and seen[1][1][2][1] is x


def test_bad_index_values_raise_and_pickling_keeps_it():
    from polyfuzz_amd.models import Hamming
    m = Hamming()
    for bad in ("Blocks", "tiles", "", 1, True, False, 0, b"auto", ["auto"], 2.0):
        with pytest.raises(ValueError, match="index"):
            m.index = bad
        assert m.index is None
    for good in ("blocks", "auto", None):
        m.index = good
        back = pickle.loads(pickle.dumps(m))
        assert back.index == good and type(back) is Hamming
    old = Hamming()
    del old.__dict__["_index"]                      # what a matcher pickled before the attribute existed holds
    assert pickle.loads(pickle.dumps(old)).index is None
    assert "index" not in inspect.signature(Hamming.__init__).parameters and "index" not in inspect.signature(Hamming.join).parameters
    assert '"blocks"' in Hamming.__doc__ and '"auto"' in Hamming.__doc__


def test_blocks_without_a_plan_raises_before_the_device(monkeypatch):
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import Hamming

    def _no_device(*a, **k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(_lib.Context, "default", classmethod(_no_device))
    names = ["a", "b", "c"]
    x = np.zeros((3, 513), np.uint8)
    m = Hamming()
    m.index = "blocks"
    for call in (lambda: m.join(names, max_distance=410, embeddings_from=x), lambda: m.join(names, names, 0.6, x, x),
                 lambda: m.components(names, 0.8, embeddings=x), lambda: m.join(names, max_distance=4104, embeddings_from=x)):
        with pytest.raises(ValueError, match="256|blocks") as e:
            call()
        assert not isinstance(e.value, _lib.PfzError) and 'index = "blocks"' in str(e.value)
    with pytest.raises(AssertionError, match="the device was reached"):      # an indexable plan goes on to the device
        m.join(names, max_distance=205, embeddings_from=x)
    m.index = "auto"                                                         # auto never refuses: the tiles are its other route
    with pytest.raises(AssertionError, match="the device was reached"):
        m.join(names, max_distance=410, embeddings_from=x)


def test_bindings():
    from polyfuzz_amd import _lib

    class Dev:
        n, h, dim = 3, None, 64
    ok = Dev()
    ok.dtype = _lib.BINARY
    for dtype in ("float32", "int8"):
        d = Dev()
        d.dtype = dtype
        with pytest.raises(ValueError, match="binary operands only"):
            _lib.hamming_join_indexed(None, d, None, 3)
        with pytest.raises(ValueError, match="binary operands only"):
            _lib.hamming_join_indexed(None, ok, d, 3)
        with pytest.raises(ValueError, match="binary operands only"):
            _lib.hamming_components_indexed(None, d, 3)
    assert _lib.HAMMING_INDEX_COUNTERS == ("blocks", "min_block_bits", "checks", "items", "route")
    for f, names in ((_lib.hamming_join_indexed, ["ctx", "from_dev", "to_dev", "max_distance", "auto", "capacity", "counters"]),
                     (_lib.hamming_components_indexed, ["ctx", "dev", "max_distance", "auto", "counters"]),
                     (_lib.hamming_index_plan, ["dim_bits", "max_distance"])):
        assert list(inspect.signature(f).parameters) == names
    assert inspect.signature(_lib.hamming_join_indexed).parameters["auto"].default is False


def test_symbols_declared_exported_and_in_the_table():
    from polyfuzz_amd import _build, _lib
    if _build.is_stale():
        _build.build()
    header = open(os.path.join(REPO, "include", "polyfuzz_hip.h")).read()
    so = ctypes.CDLL(_lib.lib_path())
    for name, n_args in (("pfz_hamming_join_indexed", 11), ("pfz_hamming_components_indexed", 8), ("pfz_hamming_index_plan", 3)):
        assert f"int {name}(" in header and hasattr(so, name) and name in _lib.SIGNATURES
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == n_args
        decl = header[header.index(f"int {name}("):]
        assert len(decl[:decl.index(";")].split(",")) == n_args
    assert header.index("---- K24") > header.index("int pfz_hamming_max_distance(")
    assert _lib.SIGNATURES["pfz_hamming_join_indexed"][1][4] is ctypes.c_int32
    assert "#define PFZ_HAMMING_INDEX_BLOCKS 1" in header and "#define PFZ_HAMMING_INDEX_AUTO 2" in header
    assert (_lib.HAMMING_INDEX_BLOCKS, _lib.HAMMING_INDEX_AUTO) == (1, 2)


def test_kernel_budget():
    """the k24_* kernels exist once each, without scratch, with at most 128 registers per lane"""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_budget
    from polyfuzz_amd import _build
    for exe in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(kernel_budget.LLVM, exe)):
            pytest.skip(f"{exe} not in {kernel_budget.LLVM}")
    md = kernel_budget.kernel_metadata(_build.build())
    pretty = dict(zip(md, kernel_budget.demangled(list(md))))
    for name in ("k24_keys", "k24_ranges", "k24_items", "k24_probe_join", "k24_probe_comp"):
        hits = [v for k, v in md.items() if pretty[k].startswith(f"pfz::{name}(")]
        assert len(hits) == 1, (name, [p for p in pretty.values() if "k24_" in p])
        k = hits[0]
        assert k["scratch"] == 0, (name, k)
        assert k["vgpr"] + k.get("agpr", 0) <= 128, (name, k)
