"""K12 (EditDistance.components: the connected components of "Levenshtein / OSA similarity >= t", united on the device) without a
GPU: the lock-free union-find of polyfuzz_amd/csrc/k12_core.h compiled for the host (tests/k12_core_host.cpp) -- every graph on
up to 5 nodes in several edge orders, and random graphs of 2 000 nodes hooked by 8 racing host threads: the root of a node is the
smallest node of its component and parent[x] <= x throughout --, linkage.dicts_from_labels on hand-made labels, the scorer gate
and the argument checks of EditDistance.components, the entry point in header / library / ctypes table, and the kernels'
register and scratch budget."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import lev_oracle

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def host():
    so = os.path.join(REPO, "oracle", "_build", "k12_core_host.so")
    src = [os.path.join(HERE, "k12_core_host.cpp"), os.path.join(REPO, "polyfuzz_amd", "csrc", "k12_core.h")]
    os.makedirs(os.path.dirname(so), exist_ok=True)
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", src[0], "-o", so])
    lib = ctypes.CDLL(so)
    lib.k12_host_exhaustive.restype = lib.k12_host_race.restype = ctypes.c_int
    lib.k12_host_exhaustive.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.k12_host_race.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def _p(x):
    return x.ctypes.data_as(ctypes.c_void_p)


def union_find_labels(n, pairs):
    """the oracle's union-find: the larger root hooked under the smaller; label[i] = the smallest position of i's component"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in pairs:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(i) for i in range(n)], np.int32)


def test_every_small_graph_in_several_edge_orders(host):
    """all 1 + 2 + 8 + 64 + 1024 graphs on 1 .. 5 nodes, their edges united ascending, descending, with swapped ends and in four
    seeded shuffles: uf_find and uf_root of every node == the smallest node of its component; parent[x] <= x after every unite"""
    report = np.zeros(5, np.int64)
    assert host.k12_host_exhaustive(5, 4, _p(report)) == 0
    assert report[0] == (1 + 2 + 8 + 64 + 1024) * 7 and report[1] == 0 and report[2] == 0, report.tolist()
    assert report[3] == 0                                      # (one thread: no compare-and-swap can fail)


@pytest.mark.parametrize("n_edges,hot", [(500, 0), (2000, 0), (20_000, 0), (200_000, 4)],
                         ids=("sparse", "critical", "one_component", "hot_roots"))
def test_racing_host_threads(host, n_edges, hot):
    """2 000 nodes, seeded random edges united by 8 threads at once through the host trait (relaxed __atomic_*): the roots are
    the smallest node of each component of the same edge list -- computed here by the oracle's sequential union-find --, and no
    thread ever saw parent[x] > x.  From many small components (500 edges) over the critical density to one component, and one
    run whose hooks all meet on four roots."""
    n = 2000
    report, label = np.zeros(5, np.int64), np.full(n + 8, -7, np.int32)
    for seed in (1, 2, 3):
        assert host.k12_host_race(n, n_edges, 8, hot, seed, _p(report), _p(label)) == 0
        assert report[0] == n_edges and report[1] == 0 and report[2] == 0, (seed, report.tolist())
        assert (label[n:] == -7).all() and (label[:n] <= np.arange(n)).all()
        assert report[4] == (label[:n] == np.arange(n)).sum() == len(np.unique(label[:n]))
        np.testing.assert_array_equal(label[label[:n]], label[:n])            # a label is its own label
        print(f"K12 host race {n_edges} edges seed {seed}: {report[4]} components, {report[3]} failed compare-and-swaps")
    if n_edges == 500:
        assert report[4] > 1000
    if n_edges >= 20_000:
        assert report[4] == 1


def test_oracle_union_find_on_known_graphs():
    """the ten-line union-find the GPU tests compare with, on graphs whose components are plain to see"""
    assert union_find_labels(6, [(4, 5), (2, 4), (0, 3)]).tolist() == [0, 1, 2, 0, 2, 2]
    assert union_find_labels(5, [(k, k + 1) for k in (3, 1, 2, 0)]).tolist() == [0] * 5
    assert union_find_labels(3, []).tolist() == [0, 1, 2] and union_find_labels(0, []).dtype == np.int32


def test_dicts_from_labels():
    """duplicates share a key, singletons are left out, ids count from 1 by the component's smallest position, the first string
    of a component names it"""
    from polyfuzz_amd.linkage import connected_components, dicts_from_labels
    strings = ["b", "solo", "a", "b", "c", "a2", "dup", "lone", "dup", "c2"]
    labels = np.array([0, 1, 2, 0, 4, 2, 6, 7, 6, 4], np.int32)              # {b, b} {a, a2} {c, c2} {dup, dup}; solo and lone alone
    clusters, mapping, names = dicts_from_labels(strings, labels)
    assert clusters == {1: ["b"], 2: ["a", "a2"], 3: ["c", "c2"], 4: ["dup"]}
    assert list(clusters) == [1, 2, 3, 4]
    assert mapping == {"b": 1, "a": 2, "a2": 2, "c": 3, "c2": 3, "dup": 4}
    assert names == {"b": "b", "a": "a", "a2": "a", "c": "c", "c2": "c", "dup": "dup"}
    assert "solo" not in mapping and "lone" not in names
    # one component of everything, members in order of first position, each distinct string once
    clusters, mapping, names = dicts_from_labels(["z", "y", "z", "x"], np.zeros(4, np.int32))
    assert clusters == {1: ["z", "y", "x"]} and set(mapping.values()) == {1} and set(names.values()) == {"z"}
    assert dicts_from_labels([], np.zeros(0, np.int32)) == ({}, {}, {})
    assert dicts_from_labels(["a", "b"], np.array([0, 1], np.int32)) == ({}, {}, {})

    class Model:                                               # connected_components: the labels of model.components, nothing else
        def components(self, strings, min_similarity):
            assert strings == ["p", "q", "p"] and min_similarity == 0.7
            return np.array([0, 1, 0], np.int32)
    assert connected_components(("p", "q", "p"), Model(), 0.7) == ({1: ["p"]}, {"p": 1}, {"p": "p"})


def _no_device(*a, **k):
    raise AssertionError("the device was reached")


@pytest.mark.parametrize("scorer", ["ratio", "jaro", "jaro_winkler", "WRatio", "token_set_ratio"])
def test_scorers_without_components_raise_before_any_device_call(scorer, monkeypatch):
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import EditDistance
    monkeypatch.setattr(_lib.Context, "default", classmethod(_no_device))
    with pytest.raises(NotImplementedError) as e:
        EditDistance(scorer=scorer).components(["a", "b"], 0.5)
    assert not isinstance(e.value, _lib.PfzError)
    for name in ("levenshtein", "osa"):
        assert name in str(e.value)


@pytest.mark.parametrize("scorer", lev_oracle.SCORERS)
def test_min_similarity_must_be_a_number_in_0_1(scorer, monkeypatch):
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import EditDistance
    monkeypatch.setattr(_lib.Context, "default", classmethod(_no_device))
    m = EditDistance(scorer=scorer)
    for bad in (float("nan"), float("inf"), -float("inf"), -1e-300, np.nextafter(1.0, 2.0), 1.5, -0.1, "0.8", None, True, [0.8]):
        with pytest.raises(ValueError):
            m.components(["a", "b"], bad)
        with pytest.raises(ValueError):
            m.components(["a", "b"], min_similarity=bad)
    for good in (0, 1, 0.0, 1.0, 0.8, np.float64(0.5), np.float32(0.25), np.int64(1)):      # accepted: the device is what stops these
        with pytest.raises(AssertionError, match="the device was reached"):
            m.components(["a", "b"], good)
    assert "normalize" in EditDistance.components.__doc__ and "NOT applied" in EditDistance.components.__doc__
    assert "components" in EditDistance.__doc__ and "components" in EditDistance.join.__doc__


def test_entry_point_in_header_library_and_table():
    from polyfuzz_amd import _build, _lib
    if _build.is_stale():
        _build.build()
    header = open(os.path.join(REPO, "include", "polyfuzz_hip.h")).read()
    so = ctypes.CDLL(_lib.lib_path())
    assert "int pfz_lev_components(" in header and hasattr(so, "pfz_lev_components") and "pfz_lev_components" in _lib.SIGNATURES
    decl = header[header.index("int pfz_lev_components("):]
    decl = decl[:decl.index(";")]
    assert [a.strip().split()[-1].lstrip("*") for a in decl[decl.index("(") + 1:decl.rindex(")")].split(",")] == [
        "ctx", "strings", "scorer", "min_similarity", "out_label", "out_pairs", "out_components", "out_counters"]
    restype, argtypes = _lib.SIGNATURES["pfz_lev_components"]
    assert restype is ctypes.c_int and len(argtypes) == 8 and argtypes[2] is ctypes.c_int32 and argtypes[3] is ctypes.c_double
    assert callable(_lib.lev_components)
    k12 = header[header.index("K12: connected components"):header.index("int pfz_lev_components(")]
    assert "Limits" in k12 and "PFZ_ERR_UNSUPPORTED" in k12 and "smallest position" in k12.lower()


def test_no_device_no_fallback():
    import polyfuzz_amd
    from polyfuzz_amd import _lib
    from polyfuzz_amd.linkage import connected_components
    from polyfuzz_amd.models import EditDistance
    if polyfuzz_amd.device_count() > 0:
        pytest.skip("a GPU is visible: the no-device failure path cannot be exercised")
    for name in lev_oracle.SCORERS:
        with pytest.raises(_lib.PfzNoDevice):
            EditDistance(scorer=name).components(["a", "b"], 0.5)
        with pytest.raises(_lib.PfzNoDevice):
            connected_components(["a", "b"], EditDistance(scorer=name), 0.5)


def test_kernel_budget():
    """the eight register walk kernels (32- / 64-bit words x 8- / 16-bit symbols x Levenshtein / OSA): no scratch, no static LDS
    beyond K8's (the match table is dynamic), at most 64 registers -- eight waves per SIMD, K11's bound: the hook is a handful of
    registers on a rare path.  The general kernel, the set-up (edit_walk.h's, shared with K11) and the flattening: no scratch.
    All 14 are counted; none carries a name K11's or K9's kernels are counted by."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_budget
    from polyfuzz_amd import _build
    for exe in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(kernel_budget.LLVM, exe)):
            pytest.skip(f"{exe} not in {kernel_budget.LLVM}")
    md = kernel_budget.kernel_metadata(_build.build())
    pretty = dict(zip(md, kernel_budget.demangled(list(md))))
    k8_lds = max(v["lds"] for k, v in md.items() if "k8_jaro_kernel" in pretty[k])
    walk = {pretty[k].split("(")[0]: v for k, v in md.items() if "k12_walk_kernel" in pretty[k]}
    assert sorted(walk) == sorted(f"void pfz::k12_walk_kernel<unsigned {w}, {idb}, {osa}>" for w in ("int", "long") for idb in (8, 16)
                                  for osa in ("false", "true")), sorted(walk)
    for name, k in walk.items():
        assert k["scratch"] == 0 and k["lds"] <= k8_lds and k["lds"] % 16 == 0 and k["vgpr"] <= 64, (name, k)
    k12 = {pretty[k]: v for k, v in md.items() if "k12_" in pretty[k] or "walk_begin_kernel<pfz::KmaxByM>" in pretty[k]}
    assert len(k12) == 8 + 4 + 2 and sum("k12_walk_general_kernel" in n for n in k12) == 4, sorted(k12)
    assert any("walk_begin_kernel<pfz::KmaxByM>" in n for n in k12) and any("k12_flatten" in n for n in k12)
    for name, k in k12.items():
        assert k["scratch"] == 0, (name, k)
        assert "k11_" not in name and "k9_lev_kernel" not in name and "k9_lev_general_kernel" not in name
