"""K15 without a GPU: the entry points in header, library and ctypes table, the header's contract, the refusals of TFIDF.join /
.components before any device call, polyfuzz_amd/csrc/k15_core.h compiled for the host (tests/k15_core_host.cpp) -- the integer
cutoff against its definition, the block bound against K3's simulated sums on real rows -- and the kernels' LDS budget."""
import ctypes
import inspect
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from tests import document_cases as dc
from tests import sparse_join_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


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
    for name in ("pfz_cossim_join", "pfz_cossim_components"):
        assert f"int {name}(" in header and hasattr(so, name) and name in _lib.SIGNATURES
    assert _arg_names(header, "pfz_cossim_join") == ["ctx", "to_index", "from_matrix", "self_join", "min_similarity", "capacity",
                                                     "out_row_ptr", "out_idx", "out_sim", "out_total", "out_counters"]
    assert _arg_names(header, "pfz_cossim_components") == ["ctx", "index", "matrix", "min_similarity", "out_label", "out_pairs",
                                                           "out_components", "out_counters"]
    restype, argtypes = _lib.SIGNATURES["pfz_cossim_join"]
    assert restype is ctypes.c_int and len(argtypes) == 11 and argtypes[3] is ctypes.c_int32 and argtypes[4] is ctypes.c_double \
        and argtypes[5] is ctypes.c_int64
    restype, argtypes = _lib.SIGNATURES["pfz_cossim_components"]
    assert restype is ctypes.c_int and len(argtypes) == 8 and argtypes[3] is ctypes.c_double
    assert _lib.SPARSE_JOIN_COUNTERS == ("visits", "skipped", "hit_steps")
    for f, names in ((_lib.sparse_join, ["ctx", "index", "from_dev", "min_similarity", "self_join", "capacity", "counters"]),
                     (_lib.sparse_components, ["ctx", "index", "dev", "min_similarity", "counters"])):
        assert list(inspect.signature(f).parameters) == names
    assert inspect.signature(_lib.sparse_join).parameters["self_join"].default is False


def test_header_states_the_hit_rule_the_capacity_rule_and_the_limits():
    header = _header()
    doc = header[header.index("---- K15"):header.index("int pfz_cossim_components(")]
    doc = " ".join(doc.replace("\n * ", "\n").split())      # (the comment's line prefix only: the text has products of its own)
    for phrase in ("*out_total is always the exact number of hits", "returns PFZ_OK, has written NONE of the three output arrays",
                   "repeated with capacity >= *out_total", "ascending within a row", "same call gives the same bytes",
                   "fewer than 2^31 rows", "the index's own limits", "PFZ_ERR_UNSUPPORTED", "PFZ_ERR_INVALID", "never (i, i)",
                   "(double)score >= min_similarity", "bit for bit", "c * 2^-30 * (norm bound) + 3e-7", "still rounds to 1.0",
                   "shares no n-gram", "the matrix to_index was built from", "unequal n_cols", "capacity < 0",
                   "k15_join", "k15_sort_unpack", "k15_components", "int64[3]", "NULL out_pairs / out_components"):
        assert phrase in doc, phrase
    prof = header[header.index("int pfz_prof_enable("):header.index("int pfz_prof_get(")]
    assert all(scope in prof for scope in ("`k15_join`", "`k15_sort_unpack`", "`k15_components`"))


def test_min_similarity_must_be_a_number_in_0_1(monkeypatch):
    from polyfuzz_amd import _lib, linkage
    from polyfuzz_amd.models import TFIDF
    monkeypatch.setattr(_lib.Context, "default", classmethod(_no_device))
    names = ["apple inc", "apple incorporated", "pear ltd"]
    m = TFIDF()
    for bad in (float("nan"), float("inf"), -float("inf"), -1e-300, np.nextafter(1.0, 2.0), 1.5, -0.1, "0.8", None, True, [0.8]):
        with pytest.raises(ValueError, match="min_similarity"):
            m.join(names, names, bad)
        with pytest.raises(ValueError, match="min_similarity"):
            m.join(names, min_similarity=bad)
        with pytest.raises(ValueError, match="min_similarity"):
            m.join(names, None, bad, re_train=False)
        with pytest.raises(ValueError, match="min_similarity"):
            m.components(names, bad)
        with pytest.raises(ValueError, match="min_similarity"):
            linkage.connected_components(names, m, bad)
        with pytest.raises(ValueError, match="min_similarity"):      # the binding refuses too, without a library call
            _lib.sparse_join(None, None, None, bad)
        with pytest.raises(ValueError, match="min_similarity"):
            _lib.sparse_components(None, None, None, bad)
    for good in (0, 1, 0.0, 1.0, 0.8, np.float64(0.5), np.float32(0.25), np.int64(1)):      # accepted: the device is what stops these
        with pytest.raises(AssertionError, match="the device was reached"):
            m.join(names, names, good)
        with pytest.raises(AssertionError, match="the device was reached"):
            m.components(names, good)
    assert list(inspect.signature(TFIDF.join).parameters) == ["self", "from_list", "to_list", "min_similarity", "re_train"]
    p = inspect.signature(TFIDF.join).parameters
    assert p["to_list"].default is None and p["min_similarity"].default == 0.8 and p["re_train"].default is True
    assert list(inspect.signature(TFIDF.components).parameters) == ["self", "from_list", "min_similarity"]
    assert inspect.signature(TFIDF.components).parameters["min_similarity"].default == 0.8
    for word in ("top_n", "min_similarity", "cosine_method"):
        assert word in TFIDF.join.__doc__ and word in TFIDF.components.__doc__


def test_the_cases_are_what_they_are_there_for():
    names, _ = C.lists("names2600")
    a = C.oracle_csr("names2600")
    per_row = np.diff(a.indptr)
    short = [s for s in names if len(s.strip()) < 3]
    assert len(names) == 2600 and len(short) == 2 and (per_row == 0).sum() >= 2 and per_row.max() <= 64
    spliced, _ = C.lists("spliced")
    assert len(spliced) == 3060 and spliced[2600:2900] == names[:300] and len(set(spliced[2900:3050])) == 1
    assert all(len(s) == 300 for s in spliced[3050:]) and all(spliced[i] != spliced[i + 1] for i in range(3050, 3060, 2))
    frm, to = C.lists(C.TWO_LIST_CASE)
    assert len(frm) == 750 and to == names and frm[:700] == C.lists("names10k")[0][2600:3300]


def _host_program():
    exe = os.path.join(REPO, "oracle", "_build", "k15_core_host")
    src = [os.path.join(HERE, "k15_core_host.cpp"), os.path.join(REPO, "polyfuzz_amd", "csrc", "k15_core.h")]
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", src[0], "-o", exe])
    return exe


def _run(mode, payload, tmp_path):
    fin, fout = str(tmp_path / f"{mode}.in"), str(tmp_path / f"{mode}.out")
    with open(fin, "wb") as f:
        f.write(payload)
    r = subprocess.run([_host_program(), mode, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    return open(fout, "rb").read()


def test_cutoff_is_the_smallest_sum_that_passes(tmp_path):
    """smin satisfies (double)((float)sum * 2^-k) >= t and smin - 1 does not, for t over a grid plus the float32 neighbours of
    each t, at scale exponents 28 .. 30 -- checked by the program on k15_passes itself and here again in numpy"""
    grid = np.concatenate([np.linspace(0.0, 1.0, 201), [0.6, 0.8, 0.9, 1e-9, 2.0 ** -30, 1.0 - 2.0 ** -25, np.nextafter(1.0, 0.0), 5e-324],
                           np.random.default_rng(15).random(300)])
    f32 = grid.astype(np.float32)
    ts = np.concatenate([grid, f32.astype(np.float64), np.nextafter(f32, np.float32(2.0)).astype(np.float64),
                         np.nextafter(f32, np.float32(-1.0)).astype(np.float64)])
    ts = np.unique(ts[(ts >= 0.0) & (ts <= 1.0)])
    cases = [(k, float(t)) for k in (28, 29, 30) for t in ts] + [(40, 0.5), (40, 1e-6), (32, 0.5), (32, np.nextafter(0.5, 0.0))]
    payload = struct.pack("<i", len(cases)) + b"".join(struct.pack("<id", k, t) for k, t in cases)
    smin = np.frombuffer(_run("cutoff", payload, tmp_path), np.int32)
    assert len(smin) == len(cases)

    def score(s, k):
        return np.float64(np.float32(np.float32(s) * np.float32(2.0 ** -k)))
    n_none = 0
    for (k, t), s in zip(cases, smin.tolist()):
        if s == 0:                                     # no sum below 2^31 passes: only where even the largest sum scores below t
            assert score(2 ** 31 - 1, k) < t, (k, t)
            n_none += 1
            continue
        assert s >= 1 and score(s, k) >= t, (k, t, s)
        assert s == 1 or score(s - 1, k) < t, (k, t, s)
    by = dict(zip(cases, smin.tolist()))
    # at 2^-28 .. 2^-30 a sum below 2^31 scores up to 8 .. 2: every t in [0, 1] has a cutoff.  At 2^-40 the largest score is 2^-9,
    # at 2^-32 it is float32(2^31 - 1) * 2^-32 = 0.5 exactly
    assert n_none == 1 and by[(40, 0.5)] == 0 and by[(40, 1e-6)] >= 1 and by[(32, 0.5)] >= 1 and by[(32, np.nextafter(0.5, 0.0))] >= 1
    assert n_none == sum(s == 0 for s in smin.tolist())
    assert by[(30, 0.0)] == 1 and by[(30, 1.0)] <= 2 ** 30 and by[(30, 0.5)] <= 2 ** 29 < by[(30, 0.6)]
    # ceil(t * S) is NOT the cutoff: the float32 rounding of the sum lets smaller sums pass
    assert any(s < int(np.ceil(t * 2.0 ** k)) for (k, t), s in by.items() if s)


def test_block_bound_is_never_below_a_sum_of_the_block(tmp_path):
    """200 random from-rows of names2600 against every block of 1024 rows: k15_block_bound over the row's n-grams that occur in
    the block is at least the largest sum K3's arithmetic (document_cases.k3_simulated_score) gives the row against a row of
    the block.  The simulated sum is taken for every row of the block whose float64 dot product is within 1e-6 of the block's
    best: K3's error on these rows is below that (k3_bound), so the largest simulated sum is among them."""
    a = C.oracle_csr("names2600")
    n, block, k = a.shape[0], 1024, dc.k3_scale_exponent(1.0, 1.0)
    assert k == 30
    rows = dc.csr_to_rows((a.indptr, a.indices, a.data))
    rng = np.random.default_rng(151)
    picked = np.sort(rng.choice(np.nonzero(np.diff(a.indptr) > 0)[0], size=200, replace=False))
    dots = (a[picked] @ a.T).toarray()
    scale = np.float32(2.0 ** k)
    records, best = [], []
    for p, i in enumerate(picked.tolist()):
        ci, vi = rows[i]
        as_k = (vi.astype(np.float32) * scale).astype(np.float32)
        for b0 in range(0, n, block):
            d = dots[p, b0:b0 + block]
            if d.max() <= 0.0:
                continue
            in_block = np.isin(ci, a.indices[a.indptr[b0]:a.indptr[min(n, b0 + block)]])      # P: the lists (k, b) that are not empty
            near = b0 + np.nonzero(d >= d.max() - 1e-6)[0]
            top = max(dc.k3_simulated_score(rows[i], rows[j], k)[0] for j in near.tolist())
            records.append(as_k[in_block])
            best.append(np.float32(top) * scale)       # float32(sum): the score times 2^k, exact
    assert len(records) > 300
    payload = struct.pack("<fi", 1.0, len(records)) + b"".join(struct.pack("<i", len(r)) + r.tobytes() for r in records)
    bound = np.frombuffer(_run("bound", payload, tmp_path), np.float32)
    best = np.array(best, np.float32)
    assert len(bound) == len(best) and (bound >= best).all(), int((bound < best).sum())
    assert (bound < np.float32(0.9 * 2.0 ** k)).mean() > 0.2                              # and worth something: blocks it would skip at 0.9


def test_kernel_budget():
    """each K15 kernel exists once per block size and form, has no scratch, and its LDS is no larger than that of the
    k3_cossim_topn_kernel<C, 96> of the same C (4 C + 768 bytes), so the workgroups per CU are K3's"""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_budget
    from polyfuzz_amd import _build
    for exe in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(kernel_budget.LLVM, exe)):
            pytest.skip(f"{exe} not in {kernel_budget.LLVM}")
    md = kernel_budget.kernel_metadata(_build.build())
    pretty = dict(zip(md, kernel_budget.demangled(list(md))))
    for c in (1024, 1536, 2048, 4096):
        k3 = [v for k, v in md.items() if f"pfz::k3_cossim_topn_kernel<{c}, 96, false>(" in pretty[k]]
        assert len(k3) == 1 and k3[0]["lds"] == 4 * c + 768, (c, k3)
        for comp in ("false", "true"):
            hits = [v for k, v in md.items() if f"pfz::k15_sparse_join_kernel<{c}, {comp}>(" in pretty[k]]
            assert len(hits) == 1, (c, comp, [p for p in pretty.values() if "k15_" in p])
            assert hits[0]["scratch"] == 0 and hits[0]["lds"] <= k3[0]["lds"], (c, comp, hits[0])
            assert hits[0]["vgpr"] <= 96, (c, comp, hits[0])      # (18 one-wave workgroups per CU are five waves on a SIMD of 512 registers)
    assert sum("k15_sparse_join_kernel<" in p for p in pretty.values()) == 8
    assert any(pretty[k].startswith("pfz::k14_unpack(") for k in md)                     # the one unpack, shared with K14
    assert not any("unpack" in p and "k15" in p for p in pretty.values())
