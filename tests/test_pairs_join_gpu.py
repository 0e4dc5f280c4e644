"""GPU parity of K16's join (pfz_pairs_join) and of BlockedEditDistance.join: the candidate pairs of a device-resident table whose
Levenshtein / OSA / Jaro / Jaro-Winkler score is >= t, as CSR, == the definition restated on the host (tests/pairs_join_cases.py)
over the CPU oracles' scores (tests/lev_oracle.py; oracle/jaro.c).  Every comparison is == on int64 row pointers, int32 indices and
float64 scores; there is no tolerance."""
import contextlib
import ctypes

import numpy as np
import pytest

from tests import pairs_join_cases as C

pytestmark = pytest.mark.gpu


def _assert_join(got, want, what):
    row_ptr, idx, sim = got[:3]
    assert row_ptr.dtype == np.int64 and idx.dtype == np.int32 and sim.dtype == np.float64, what
    np.testing.assert_array_equal(row_ptr, want[0], err_msg=str(what))
    np.testing.assert_array_equal(idx, want[1], err_msg=str(what))
    np.testing.assert_array_equal(sim, want[2], err_msg=str(what))
    if len(got) > 3:
        assert got[3] == want[3], (what, got[3], want[3])


@contextlib.contextmanager
def _k16_counters(ctx):
    """box["launches"] = timed K16 scoring scopes (one per call that reaches the device), box["general"] = launches of the general
    kernel"""
    box = {}
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        yield box
        ctx.sync()
        box["launches"] = ctx.prof_get("k16_pairs_join")[1]
        box["general"] = ctx.prof_get("k16_pairs_join_general")[1]
    finally:
        ctx.prof_enable(False)


def _attained(sim, cand, self_join):
    """a score strictly inside (0, 1) that a candidate pair attains exactly: the median of the distinct ones"""
    i, j, _ = C.candidate_pairs(cand[:sim.shape[0]], sim.shape[1], self_join)
    s = np.unique(sim[i, j])
    s = s[(s > 0.0) & (s < 1.0)]
    return float(s[len(s) // 2])


# ---- 1. mixed shapes, two lists -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", C.FOUR)
def test_mixed_shapes_two_lists(ctx, name):
    """both word widths, Jaro's 256-character border, the general kernel, a second and a third chunk of partners, junk cells, a
    duplicated index, rows without any pair; every threshold of the issue and one that a pair attains exactly"""
    from polyfuzz_amd import _lib
    fl, tl, sims, tables = C.mixed()
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for m, tab in tables.items():
        c = C.device_table(ctx, tab)
        eq = _attained(sims[name], tab, False)
        for thr in C.THRESHOLDS + (eq,):
            want = C.expected_join(sims[name], tab, thr, False)
            with _k16_counters(ctx) as box:
                got = _lib.pairs_join(ctx, f, t, c, name, thr, capacity=tab.size, counters=True)
            _assert_join(got, want, (name, m, thr))
            assert box["launches"] == 1 and box["general"] == 1          # (from-strings beyond 64 characters are in every call)
        assert (want[2] == eq).any() and (sims[name] < eq).any()          # equal is kept, and the threshold is one
    # the PFZ_PAIR_* id names the scorer as well
    _assert_join(_lib.pairs_join(ctx, f, t, c, _lib.PAIR_SCORERS[name], 0.5), C.expected_join(sims[name], tab, 0.5, False), name)


# ---- 2. the self-join -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", C.FOUR)
def test_self_join(ctx, name):
    """pairs listed in both rows, only in the higher row, own indices, duplicates; long lower positions with short higher ones and
    the reverse; a Jaro pair with a partner beyond 256 characters.  No to-list and the from-list's own handle are the same call."""
    from polyfuzz_amd import _lib
    strings, sims, tab = C.self_list()
    f, c = _lib.DeviceStrings.upload(ctx, strings), C.device_table(ctx, tab)
    for thr in C.THRESHOLDS + (_attained(sims[name], tab, True),):
        want = C.expected_join(sims[name], tab, thr, True)
        _assert_join(_lib.pairs_join(ctx, f, None, c, name, thr, counters=True), want, (name, thr, "no to-list"))
        _assert_join(_lib.pairs_join(ctx, f, f, c, name, thr, counters=True), want, (name, thr, "own handle"))
        row = np.repeat(np.arange(len(strings)), np.diff(want[0]))
        assert (row < want[1]).all()                                       # reported as (min, max)
    # another handle of the same list is a to-list: the table is then read as it stands, own indices included
    g = _lib.DeviceStrings.upload(ctx, strings)
    _assert_join(_lib.pairs_join(ctx, f, g, c, name, 0.8, counters=True), C.expected_join(sims[name], tab, 0.8, False), (name, "two handles"))


# ---- 3. a hub -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("position,length", [("first", 20), ("first", 50), ("first", 80), ("last", 20)])
def test_hub(ctx, position, length):
    """m = 5, but the hub's row has 72 partners after the symmetrisation: a second chunk of lanes, in 32-bit words, in 64-bit words
    and in the general kernel; with the hub last, its 72 pairs belong to 72 other rows"""
    from polyfuzz_amd import _lib
    strings, sims, tab = C.hub(position, length)
    f, c = _lib.DeviceStrings.upload(ctx, strings), C.device_table(ctx, tab)
    for name in C.FOUR:
        for thr in C.THRESHOLDS:
            want = C.expected_join(sims[name], tab, thr, True)
            _assert_join(_lib.pairs_join(ctx, f, None, c, name, thr, counters=True), want, (position, length, name, thr))
        if position == "first":
            assert np.diff(C.expected_join(sims[name], tab, 0.0, True)[0])[0] == 72


# ---- 4. capacity ----------------------------------------------------------------------------------------------------------------

def _raw_join(ctx, f, t, c, scorer, thr, cap, n_from):
    """pfz_pairs_join itself, with 8 guard words behind every buffer: (rc, total, row_ptr, idx, sim) -- whole buffers"""
    from polyfuzz_amd import _lib
    row_ptr = np.full(n_from + 1 + 8, -7, np.int64)
    idx, sim = np.full(cap + 8, -7, np.int32), np.full(cap + 8, -7.0, np.float64)
    total = ctypes.c_int64(-7)
    rc = ctx.lib.pfz_pairs_join(ctx.h, f.h, None if t is None else t.h, c.h, scorer, ctypes.c_double(thr), cap, _lib._ptr(row_ptr),
                                _lib._ptr(idx), _lib._ptr(sim), ctypes.byref(total), None)
    return rc, total.value, row_ptr, idx, sim


def test_capacity_total_and_guard_words(ctx, monkeypatch):
    """capacity = 0, total - 1, total and more through pfz_pairs_join: the total is exact every time; with room, exactly `total`
    entries and n + 1 row pointers are written and not a word behind them; without, none of the three arrays is touched; the
    binding then repeats the call once, never more often"""
    from polyfuzz_amd import _lib
    strings, sims, tab = C.self_list()
    n = len(strings)
    f, c = _lib.DeviceStrings.upload(ctx, strings), C.device_table(ctx, tab)
    for name in ("osa", "jaro_winkler"):
        want = C.expected_join(sims[name], tab, 0.5, True)
        total = len(want[1])
        assert total > 3
        for cap in (0, total - 1, total, total + 5, 1):
            rc, got_total, row_ptr, idx, sim = _raw_join(ctx, f, None, c, _lib.PAIR_JOIN_SCORERS[name], 0.5, cap, n)
            assert rc == 0 and got_total == total, (name, cap, rc, got_total)
            if cap >= total:
                _assert_join((row_ptr[:n + 1], idx[:total], sim[:total]), want, f"{name} capacity {cap}")
                assert (row_ptr[n + 1:] == -7).all() and (idx[total:] == -7).all() and (sim[total:] == -7.0).all()
            else:
                assert (row_ptr == -7).all() and (idx == -7).all() and (sim == -7.0).all(), (name, cap)
        real, calls = ctx.lib.pfz_pairs_join, []

        def counted(*a):
            calls.append(a[6])
            return real(*a)
        monkeypatch.setattr(ctx.lib, "pfz_pairs_join", counted)
        for cap, n_calls in ((0, 2), (1, 2), (total - 1, 2), (total, 1), (None, 1)):
            del calls[:]
            _assert_join(_lib.pairs_join(ctx, f, None, c, name, 0.5, capacity=cap), want, f"{name} binding, capacity {cap}")
            assert len(calls) == n_calls and (n_calls == 1 or calls[1] == total), (cap, calls)
        monkeypatch.undo()


# ---- 5. order independence ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", C.FOUR)
def test_order_independence(ctx, name):
    """the columns of every row shuffled: identical bytes, two lists and self-join"""
    from polyfuzz_amd import _lib
    fl, tl, _, tables = C.mixed()
    strings, _, stab = C.self_list()
    f, t, s = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl), _lib.DeviceStrings.upload(ctx, strings)
    rng = np.random.default_rng(1605)
    for frm, to, tab in ((f, t, tables[5]), (f, t, tables[65]), (f, t, tables[130]), (s, None, stab)):
        first = _lib.pairs_join(ctx, frm, to, C.device_table(ctx, tab), name, 0.5, counters=True)
        assert len(first[1]) > 0
        for _ in range(2):
            perm = np.stack([row[rng.permutation(tab.shape[1])] for row in tab])
            assert (perm != tab).any()
            got = _lib.pairs_join(ctx, frm, to, C.device_table(ctx, perm), name, 0.5, counters=True)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], first[:3])) and got[3] == first[3], (name, tab.shape)


# ---- 6. agreement with the all-pairs kernels ------------------------------------------------------------------------------------

def test_agreement_with_the_all_pairs_kernels(ctx):
    """every row lists all n_to indices (shuffled): Levenshtein / OSA are K11's join, CSR and scores, two lists and self-join; Jaro
    / Jaro-Winkler are K8's matrix thresholded on the host"""
    from polyfuzz_amd import _lib
    fl, tl, _, _ = C.mixed()
    strings, _, _ = C.self_list()
    f, t, s = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl), _lib.DeviceStrings.upload(ctx, strings)
    rng = np.random.default_rng(1606)
    full = lambda n, n_to: C.device_table(ctx, np.stack([rng.permutation(n_to).astype(np.int32) for _ in range(n)]))
    c2, c1 = full(len(fl), len(tl)), full(len(strings), len(strings))
    assert len(tl) <= 270 and len(strings) <= 210
    for thr in (0.3, 0.5, 0.8, 1.0):
        for name in ("levenshtein", "osa"):
            for frm, to, c in ((f, t, c2), (s, None, c1)):
                row_ptr, idx, _, sim = _lib.lev_join(ctx, frm, to, name, thr)
                _assert_join(_lib.pairs_join(ctx, frm, to, c, name, thr), (row_ptr, idx, sim), (name, thr, to is None))
        for name in ("jaro", "jaro_winkler"):
            m2 = _lib.jaro_matrix(ctx, f, t, name)
            _assert_join(_lib.pairs_join(ctx, f, t, c2, name, thr), _csr_of(m2 >= thr, m2), (name, thr))
            m1 = _lib.jaro_matrix(ctx, s, s, name)
            _assert_join(_lib.pairs_join(ctx, s, None, c1, name, thr), _csr_of(np.triu(m1 >= thr, 1), m1), (name, thr, "self"))


def _csr_of(keep, m):
    row_ptr = np.zeros(len(m) + 1, np.int64)
    np.cumsum(keep.sum(axis=1), out=row_ptr[1:])
    i, j = np.nonzero(keep)
    return row_ptr, j.astype(np.int32), m[i, j]


# ---- 7. an alphabet whose match table does not fit LDS ---------------------------------------------------------------------------

def test_wide_alphabet_takes_the_general_kernel(ctx, oracle_mod):
    """8 000 distinct code points in the to-list: 64 KB of 64-bit table entries, beyond the 60 KiB budget -- every row is the general
    kernel's, short ones included"""
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(1604)
    wide = [chr(c) for c in range(0x4E00, 0x4E00 + 8000)]
    mk = lambda n, a: "".join(a[i] for i in rng.integers(0, len(a), n))
    uniq = ["".join(wide[k:k + 100]) for k in range(0, 8000, 100)] + [mk(int(n), wide[:12]) for n in rng.integers(0, 40, 20)]
    tl = uniq + uniq[::-1]
    fl = [mk(int(n), wide[:12]) for n in (0, 1, 20, 32, 33, 64, 65, 130)] + [s[::2] for s in uniq[:6]] + [uniq[3], uniq[85]]
    assert len(set("".join(tl))) == 8000 and (8000 + 1) * 8 > 60 * 1024
    sims = C.all_scores(oracle_mod, fl, tl)
    tab = C.random_table(rng, len(fl), len(tl), 70)
    f, t, c = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl), C.device_table(ctx, tab)
    for name in C.FOUR:
        for thr in (0.0, 0.2, 1.0):
            with _k16_counters(ctx) as box:
                got = _lib.pairs_join(ctx, f, t, c, name, thr, capacity=tab.size, counters=True)
            _assert_join(got, C.expected_join(sims[name], tab, thr, False), (name, thr))
            assert box["launches"] == 1 and box["general"] == 1
        assert 0 < C.expected_join(sims[name], tab, 0.2, False)[3]["pairs"] < C.expected_join(sims[name], tab, 0.0, False)[3]["pairs"]


# ---- 8. the entry point ---------------------------------------------------------------------------------------------------------

def test_entry_point_refuses_what_it_cannot_do(ctx):
    from polyfuzz_amd import _lib
    f = _lib.DeviceStrings.upload(ctx, ["ab", "b", "abc"])
    t = _lib.DeviceStrings.upload(ctx, ["a", "b"])
    c = C.device_table(ctx, np.array([[0, 1], [1, -1], [5, 0]], np.int32))
    row_ptr, idx, sim = _lib.pairs_join(ctx, f, t, c, "levenshtein", 0.5)
    assert row_ptr.tolist() == [0, 2, 3, 3] and idx.tolist() == [0, 1, 1] and sim.tolist() == [0.5, 0.5, 1.0]
    n = 3

    def raw(scorer, thr, cap, table=c, outputs=True):
        row_ptr, idx, sim = np.zeros(n + 1, np.int64), np.zeros(4, np.int32), np.zeros(4)
        total = ctypes.c_int64(0)
        return ctx.lib.pfz_pairs_join(ctx.h, f.h, t.h, table.h, scorer, ctypes.c_double(thr), cap, _lib._ptr(row_ptr),
                                      _lib._ptr(idx) if outputs else None, _lib._ptr(sim) if outputs else None, ctypes.byref(total), None)
    for scorer, thr, cap in ((0, 0.5, 4), (5, 0.5, 4), (-1, 0.5, 4), (1, float("nan"), 4), (2, 1.5, 4), (3, -0.25, 4), (4, float("inf"), 4),
                             (1, 0.5, -1)):
        assert raw(scorer, thr, cap) == -1, (scorer, thr, cap)           # PFZ_ERR_INVALID
    assert raw(1, 0.5, 4, outputs=False) == -1 and raw(1, 0.5, 0, outputs=False) == 0       # NULL outputs need capacity 0
    assert raw(1, 0.5, 4, table=C.device_table(ctx, np.zeros((2, 2), np.int32))) == -1      # fewer rows than from-strings
    with pytest.raises(_lib.PfzError, match="0 .. 100") as e:
        _lib.pairs_join(ctx, f, t, c, 0, 0.5)
    assert e.value.code == -1 and "ratio" in str(e.value)
    with pytest.raises(_lib.PfzError, match="0 .. 100"):
        _lib.pairs_components(ctx, f, c, 0, 0.5)
    with pytest.raises(KeyError):
        _lib.pairs_join(ctx, f, t, c, "ratio", 0.5)
    with pytest.raises(_lib.PfzUnsupported, match="1024"):
        _lib.pairs_join(ctx, f, t, C.device_table(ctx, np.full((3, 1025), -1, np.int32)), "jaro", 0.5)
    with pytest.raises(_lib.PfzUnsupported, match="1024"):
        _lib.pairs_components(ctx, f, C.device_table(ctx, np.full((3, 1025), -1, np.int32)), "jaro", 0.5)
    row_ptr, idx, sim, counts = _lib.pairs_join(ctx, f, t, C.device_table(ctx, np.full((3, 1024), -1, np.int32)), "osa", 0.0, counters=True)
    assert row_ptr.tolist() == [0, 0, 0, 0] and len(idx) == len(sim) == 0 and counts == {"candidates": 0, "scored": 0, "pairs": 0}
    # the zero-size cases: empty results (a table without columns cannot be allocated: pfz_topn_alloc wants ntop >= 1)
    e0 = _lib.DeviceStrings.upload(ctx, [])
    for frm, to, table, rows in ((e0, t, c, 0), (f, e0, c, n), (e0, None, c, 0)):
        row_ptr, idx, sim, counts = _lib.pairs_join(ctx, frm, to, table, "jaro", 0.0, counters=True)
        assert row_ptr.tolist() == [0] * (rows + 1) and len(idx) == len(sim) == 0 and counts == {"candidates": 0, "scored": 0, "pairs": 0}


# ---- 9. the matcher -------------------------------------------------------------------------------------------------------------

def _assert_frame(df, want):
    assert list(df.columns) == ["From", "To", "Similarity"] == list(want.columns) and len(df) == len(want)
    assert df["Similarity"].dtype == np.float64
    np.testing.assert_array_equal(df["Similarity"].to_numpy(), want["Similarity"].to_numpy())
    assert df["From"].tolist() == want["From"].tolist() and df["To"].tolist() == want["To"].tolist()


@pytest.fixture(scope="module")
def titles(ctx, golden, oracle_mod):
    """303 from-strings x 500 to-titles, a second from-list, a self-join list of 400 with repeats (the shapes of
    tests/test_pairs_rescore_gpu.py's `titles`) -- with the oracles' scores and the candidate indices of an identically configured
    TFIDF"""
    from polyfuzz_amd.models import TFIDF
    t, s = golden["titles_lists"], golden["titles_self_list"]["from_list"]
    fl = t["from_list"][:300] + ["", "ab", "zzzqqqxxx"]
    tl = (t["to_list"] + s + t["from_list"][::-1])[:500]
    fl2 = t["from_list"][40:100] + s[:30] + ["q", "the"]
    dup, sims_self = C.titles_self()
    assert len(fl) == 303 and len(tl) == 500 and len(dup) == 400 and len(set(dup)) < 400
    tf = TFIDF(min_similarity=0.0, top_n=16)
    cand = tf.match_device(fl, tl).download()[0]
    cand2 = tf.match_device(fl2, tl, re_train=False).download()[0]
    cand_self = TFIDF(min_similarity=0.0, top_n=16).match_device(dup).download()[0]
    assert cand.shape == (303, 16) and cand_self.shape == (400, 16) and (cand[300:302] == -1).all()
    return {"fl": fl, "tl": tl, "fl2": fl2, "dup": dup, "cand": cand, "cand2": cand2, "cand_self": cand_self,
            "sims": C.all_scores(oracle_mod, fl, tl), "sims2": C.all_scores(oracle_mod, fl2, tl), "sims_self": sims_self}


@pytest.mark.parametrize("name", C.FOUR)
def test_matcher(ctx, titles, name):
    from polyfuzz_amd.models import BlockedEditDistance
    d = titles
    fl, tl, fl2, dup = d["fl"], d["tl"], d["fl2"], d["dup"]
    for thr in (0.5, 0.8):
        m = BlockedEditDistance(scorer=name, candidates=16, normalize=True)
        want = C.expected_join(d["sims"][name], d["cand"], thr, False)
        _assert_frame(m.join(fl, tl, thr), C.frame_of(fl, tl, *want[:3]))
        assert m.last_counts == want[3] and 0 < want[3]["pairs"] < want[3]["scored"]
        assert set(m.last_timings) == {"tfidf", "k16", "frame"}
        # re_train=False on a second from-list: the fitted TF-IDF side and the resident raw to-list serve again
        held = m._to_dev
        want = C.expected_join(d["sims2"][name], d["cand2"], thr, False)
        _assert_frame(m.join(fl2, list(tl), thr, re_train=False), C.frame_of(fl2, tl, *want[:3]))
        assert m._to_dev is held and m.last_counts == want[3]
        # the self-join
        want = C.expected_join(d["sims_self"][name], d["cand_self"], thr, True)
        m = BlockedEditDistance(scorer=name, candidates=16)
        _assert_frame(m.join(dup, min_similarity=thr), C.frame_of(dup, dup, *want[:3]))
        assert m.last_counts == want[3] and want[3]["scored"] < want[3]["candidates"]      # (pairs listed from both sides)
    assert len(BlockedEditDistance(scorer=name, candidates=16).join(dup)) == len(C.expected_join(d["sims_self"][name], d["cand_self"], 0.8, True)[1])
