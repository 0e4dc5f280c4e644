"""GPU parity of K21 -- JaroWinkler.match(top_n=, min_similarity=) / _lib.jaro_topn, the n best choices of every from-string under
Jaro / Jaro-Winkler -- against the stable sort of the oracles' scores (tests/jaro_oracle.py; oracle/jaro.c for the large shapes)
after the left-out choices are masked and the cutoff applied.  Every comparison is == on int32 indices and on float64 scores; there
is no tolerance."""
import contextlib

import numpy as np
import pytest

from tests import helpers, jaro_oracle
from tests.test_edit_topn_gpu import _assert_frame, _want_frame, expected_topn
from tests.test_jaro_gpu import (LDS_LIMIT_SYMBOLS, N_TO_LONG_LANES, _first_occurrence, _left_out, _rand, lds_limit_lists, long_lane_lists,
                                 wide_alphabet_lists)
from tests.test_levenshtein_gpu import _skip_forms, pruning_lists

pytestmark = pytest.mark.gpu

SCORERS = ("jaro", "jaro_winkler")


def _with_cutoff(want, cutoff):
    """expected_topn's pair with the entries below `cutoff` gone (they are a suffix of every row: -1 / 0.0)"""
    idx, val = want
    keep = (idx >= 0) & (val >= cutoff)
    return np.where(keep, idx, -1).astype(np.int32), np.where(keep, val, 0.0)


def _assert_topn(got, want, what):
    idx, score = got[0], got[1]
    assert idx.dtype == np.int32 and score.dtype == np.float64 and idx.shape == want[0].shape == score.shape, what
    np.testing.assert_array_equal(idx, want[0], err_msg=str(what))
    np.testing.assert_array_equal(score, want[1], err_msg=str(what))


@contextlib.contextmanager
def _k21_scopes(ctx):
    """with _k21_scopes(ctx) as box: ...K21 calls...  ->  box["launches"] = timed K21 scopes (one per call), box["general"] = launches
    of the general kernel"""
    box = {}
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        yield box
        ctx.sync()
        box["launches"] = ctx.prof_get("k21_jaro_topn")[1]
        box["general"] = ctx.prof_get("k21_jaro_topn_general")[1]
    finally:
        ctx.prof_enable(False)


# ---- 1. mixed ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed(golden):
    """~120 x 250 on the recipe of test_jaro_gpu.py's `mixed`, every to-string present twice (the index decides)"""
    rng = np.random.default_rng(211)
    t = golden["titles_lists"]
    edge = [31, 32, 33, 63, 64, 65]
    base = "the quick brown fox jumps over the lazy dog and runs far away from home again"
    prefixes = ["abcdef"[:k] + "uvwxyz"[k:] + tail for k in range(7) for tail in ("", "mnopq", "qponm")]
    fl = (t["from_list"][:35] + ["", "a", "ab", "the matrix", "Z"] + [base[:n] for n in edge] + [base[::-1][:n] for n in edge] +
          ["ab" * 100, "naïve café Ωmega \U0001f600 smile", "qqq中文", "####", "\U0001f600\U0001f601"] + _rand(rng, "ab", 1, 70, 30) +
          prefixes[:14] + _rand(rng, "abcdefgh ", 60, 66, 10))
    uniq = (t["to_list"][:40] + ["", "a", "ba", "the matrix", "The Matrix"] + [base[:n] for n in edge] + [base[3:3 + n] for n in edge] +
            ["ba" * 75, "naïve cafe Ωmega \U0001f601 smile \U0001f600", "中文qqq"] + [(base * 4)[:n] for n in (255, 256, 257)] + [(base * 14)[:1000]] +
            _rand(rng, "ab", 1, 70, 16) + prefixes + _rand(rng, "abcdefgh ", 60, 66, 6) + _rand(rng, "abc", 1, 9, 14))
    tl = uniq + uniq[::-1]
    return fl, tl, {name: jaro_oracle.matrix(fl, tl, name) for name in SCORERS}


def test_mixed_skips_cutoffs_and_shard(ctx, mixed):
    from polyfuzz_amd import _lib
    fl, tl, sims = mixed
    n, n_to = len(fl), len(tl)
    assert 110 <= n <= 130 and 230 <= n_to <= 270
    assert {0, 1, 31, 32, 33, 63, 64, 65, 200} <= set(map(len, fl)) and {0, 1, 32, 33, 64, 65, 255, 256, 257, 1000} <= set(map(len, tl))
    assert max(map(ord, "".join(tl))) > 0xFFFF and any(255 < ord(c) <= 0xFFFF for c in "".join(tl))
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    rng = np.random.default_rng(212)
    for name in SCORERS:
        sim = sims[name]
        plain = jaro_oracle.argmax(sim)
        assert (plain[0] < n_to // 2).all()                           # (every best has a later twin: ties did occur)
        one, up_to = _skip_forms(rng, plain[0], n, n_to, n_to - 1)
        assert (expected_topn(sim, 5, up_to)[0][-3:] == -1).all()     # the last rows keep no choice at all
        for what, skip in (("no skip", None), ("one choice", one), ("up to", up_to)):
            a_idx, a_score = _lib.jaro_argmax(ctx, f, t, name, skip)
            for ntop in (1, 2, 5, 64):
                got = _lib.jaro_topn(ctx, f, t, name, ntop, skip)
                _assert_topn(got, expected_topn(sim, ntop, skip), (name, what, ntop))
                np.testing.assert_array_equal(got[0][:, 0], a_idx)
                np.testing.assert_array_equal(got[1][:, 0], a_score)
        _assert_topn(_lib.jaro_topn(ctx, f, t, name, 5, None, begin=30, end=61), [a[30:61] for a in expected_topn(sim, 5)], (name, "row shard"))
        # an empty from-string scores 0.0 against everything: its top-n is its first choices not left out
        e = fl.index("")
        assert expected_topn(sim, 5)[0][e].tolist() == [0, 1, 2, 3, 4] and (sim[e] == 0.0).all()
        # the cutoff: equal is kept, the next float64 above it drops the pair
        top5 = expected_topn(sim, 5)[1]
        inner = np.sort(top5[(top5 > 0.75) & (top5 < 1.0)])
        attained = float(inner[len(inner) // 2])
        above = float(np.nextafter(attained, 2.0))
        for cutoff in (0.7, 1.0, attained, above):
            for what, skip in (("no skip", None), ("up to", up_to)):
                for ntop in (5, 64):
                    want = _with_cutoff(expected_topn(sim, ntop, skip), cutoff)
                    _assert_topn(_lib.jaro_topn(ctx, f, t, name, ntop, skip, score_cutoff=cutoff), want, (name, what, ntop, cutoff))
        at, ab = (_with_cutoff(expected_topn(sim, 5), c) for c in (attained, above))
        assert (at[1] == attained).any() and not (ab[1] == attained).any() and (ab[0] >= 0).sum() < (at[0] >= 0).sum()
        assert (_with_cutoff(expected_topn(sim, 5), 1.0)[0] >= 0).sum() >= 4


# ---- 2. fewer choices than ntop; the refusals ----------------------------------------------------------------------------------

def test_fewer_choices_than_ntop(ctx):
    from polyfuzz_amd import _lib
    rng = np.random.default_rng(213)
    fl = _rand(rng, "abc", 0, 12, 9) + ["", "abc" * 30]
    for tl, ntop, skip in ((["abc", "", "abcb"], 5, None),
                           (_rand(rng, "abc", 0, 12, 70), 64, np.full(len(fl), -2 - 59, np.int32))):      # up to 59: ten choices left
        f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
        left = len(tl) if skip is None else 10
        for name in SCORERS:
            want = expected_topn(jaro_oracle.matrix(fl, tl, name), ntop, skip)
            assert (want[0][:, :left] >= 0).all() and (want[0][:, left:] == -1).all() and (want[1][:, left:] == 0.0).all()
            _assert_topn(_lib.jaro_topn(ctx, f, t, name, ntop, skip), want, (name, len(tl), ntop))


def test_entry_point_refuses_what_it_cannot_do(ctx):
    from polyfuzz_amd import _lib
    f = _lib.DeviceStrings.upload(ctx, ["a", "b"])
    for bad in (0, -3):
        with pytest.raises(_lib.PfzError) as e:
            _lib.jaro_topn(ctx, f, f, "jaro", bad)
        assert e.value.code == -1                                          # PFZ_ERR_INVALID
    with pytest.raises(_lib.PfzUnsupported, match="64"):
        _lib.jaro_topn(ctx, f, f, "jaro_winkler", 65)
    for bad in (float("nan"), -0.1, 1.5):
        with pytest.raises(_lib.PfzError) as e:
            _lib.jaro_topn(ctx, f, f, "jaro", 2, score_cutoff=bad)
        assert e.value.code == -1
    with pytest.raises(KeyError):
        _lib.jaro_topn(ctx, f, f, "ratio", 2)
    idx, score = np.zeros((2, 2), np.int32), np.zeros((2, 2))
    for scorer in (2, -1):
        assert ctx.lib.pfz_jaro_topn(ctx.h, f.h, f.h, scorer, None, 0, 2, 2, 0.0, idx.ctypes.data_as(_lib.c_vp), score.ctypes.data_as(_lib.c_vp),
                                     None) == -1
    with pytest.raises(_lib.PfzError) as e:
        _lib.jaro_topn(ctx, f, f, "jaro", 2, np.array([1, -5], np.int32))     # both skip forms in one call
    assert e.value.code == -1
    idx, score = _lib.jaro_topn(ctx, f, f, "jaro", 3, None, begin=1, end=1)    # an empty row range
    assert idx.shape == (0, 3) and score.shape == (0, 3)
    none = _lib.DeviceStrings.upload(ctx, [])
    idx, score = _lib.jaro_topn(ctx, f, none, "jaro_winkler", 3)                # an empty to-list
    assert idx.shape == (2, 3) and (idx == -1).all() and (score == 0.0).all()


# ---- 3. long lanes and row reuse -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SCORERS)
@pytest.mark.parametrize("cls", ["32x32", "32xwide", "64xall"])
def test_long_lanes_pruning_and_row_reuse(ctx, oracle_mod, cls, name):
    """One register launch per call, 32 x CUs from-strings against 1 024 to-strings (every one two or three times): every wave meets
    four groups per from-string, so its list fills and the floor prunes, and every workgroup takes four from-strings, so list, floor
    and match table are reset and reused.  ntop 1 and 5 without skip, ntop 5 under "up to" codes == the C oracle's stable sort.
    That the paths ran: 0 launches of the general kernel, 1 timed scope, and strictly fewer pairs scored in float64 than were not
    left out (a condition that the pruning ran, not a measurement).  The four counters' shares are printed.
    Measured on an MI355X (256 CUs, 8 192 from-strings), share of the pairs not left out that were scored at ntop 1 / ntop 5 / ntop 5
    under "up to" codes: 32x32 0.25 / 0.27 / 0.27, 32xwide 0.25 / 0.27 / 0.27, 64xall 0.25 / 0.26 / 0.26 (K8's arg-max on the same
    lists: 0.54 - 0.68); 0.7 - 1.8 s per case, oracle included."""
    from polyfuzz_amd import _lib
    n_from = 32 * ctx.info()["n_cu"]
    fl, tl = long_lane_lists(cls, n_from)
    n, n_to = len(fl), len(tl)
    assert n == n_from and n_to == N_TO_LONG_LANES
    want = helpers.jaro_oracle_matrix(oracle_mod, fl, tl, name)
    rng = np.random.default_rng(214)
    up_to = (-2 - rng.integers(0, 128, n)).astype(np.int32)
    up_to[::7] = -1
    up_to[-3:] = -2 - (n_to - 1)                     # no choice left
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    want5, want5_up_to = expected_topn(want, 5), expected_topn(want, 5, up_to)
    for what, skip, ntop, e in (("no skip", None, 1, [a[:, :1] for a in want5]), ("no skip", None, 5, want5), ("up to", up_to, 5, want5_up_to)):
        kept = n * n_to if skip is None else int((~_left_out(n_to, skip)).sum())
        with _k21_scopes(ctx) as box:
            idx, score, work = _lib.jaro_topn(ctx, f, t, name, ntop, skip, counters=True)
        shares = {k: round(v / (kept if k != "steps" else 1), 4) for k, v in work.items()}
        print(f"K21 long lanes {cls} {name} {what} ntop {ntop}: of {kept} pairs not left out {shares}")
        _assert_topn((idx, score), e, (cls, name, what, ntop))
        assert box["general"] == 0 and box["launches"] == 1
        assert work["pairs_scored"] <= work["pairs_alive_after_sweep1"] <= work["pairs_walked"] <= n * n_to
        assert work["pairs_scored"] < kept, (cls, name, what, ntop)
    assert (want5[0][:, 0] < want5[0][:, 1]).sum() > n // 2 and (want5[1][:, 0] == want5[1][:, 1]).sum() > n // 2      # (twins)
    assert (want5_up_to[0][-3:] == -1).all()


# ---- 4. one length -------------------------------------------------------------------------------------------------------------

def test_to_strings_of_one_length_are_all_walked(ctx, oracle_mod):
    """100 from-strings cut to 40 characters x 256 to-strings of 40: every to-string has the same length bound, which no score of
    the row exceeds, so no group can be skipped -- every pair's sweep begins"""
    from polyfuzz_amd import _lib
    fl, tl = pruning_lists()
    same = ([s for s in tl if len(s) == 40] * 40)[:256]
    from_40 = [s[:40] for s in fl[:100]]
    assert len(same) == 256 and len(from_40) == 100
    f, t = _lib.DeviceStrings.upload(ctx, from_40), _lib.DeviceStrings.upload(ctx, same)
    for name in SCORERS:
        want = helpers.jaro_oracle_matrix(oracle_mod, from_40, same, name)
        idx, score, work = _lib.jaro_topn(ctx, f, t, name, 5, counters=True)
        _assert_topn((idx, score), expected_topn(want, 5), name)
        assert work["pairs_walked"] == 100 * 256, name


# ---- 5. parts ------------------------------------------------------------------------------------------------------------------

def test_few_rows_split_over_workgroups(ctx, oracle_mod):
    """3 from-strings (one per class: <= 32, <= 64, beyond) x 4 096 to-strings, every one of them twice: every part prunes on its own
    floor and the merge must find the row's"""
    from polyfuzz_amd import _lib
    _, tl = pruning_lists()
    big = "".join(tl[:40])
    fl = [big[:20], big[30:80], big[100:200]]
    assert [len(s) for s in fl] == [20, 50, 100] and len(tl) == 4096
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for name in SCORERS:
        want = helpers.jaro_oracle_matrix(oracle_mod, fl, tl, name)
        for ntop in (5, 64):
            _assert_topn(_lib.jaro_topn(ctx, f, t, name, ntop), expected_topn(want, ntop), (name, ntop))


# ---- 6. 16-bit symbols and the LDS limit -----------------------------------------------------------------------------------------

def test_wide_alphabet_and_the_lds_limit(ctx, oracle_mod):
    """More than 255 distinct code points (16-bit symbols: every register instance and the general kernel in both of its uses), and a
    to-list whose match table is one entry beyond 60 KiB: everything goes through the general kernel, which scores every pair"""
    from polyfuzz_amd import _lib
    fl, tl = wide_alphabet_lists()
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for name in SCORERS:
        want = helpers.jaro_oracle_matrix(oracle_mod, fl, tl, name)
        with _k21_scopes(ctx) as box:
            got = _lib.jaro_topn(ctx, f, t, name, 5)
        _assert_topn(got, expected_topn(want, 5), ("wide", name))
        assert box["general"] == 3 and box["launches"] == 1      # the rows of <= 32 and of 33 .. 64 beyond 256; the long rows
    fl, tl = lds_limit_lists(LDS_LIMIT_SYMBOLS + 1, 100)
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for name in SCORERS:
        want = oracle_mod.jaro_matrix(fl, tl, name)
        with _k21_scopes(ctx) as box:
            idx, score, work = _lib.jaro_topn(ctx, f, t, name, 5, counters=True)
        _assert_topn((idx, score), expected_topn(want, 5), ("lds limit", name))
        assert box["general"] == 1 and box["launches"] == 1 and work["pairs_scored"] == len(fl) * len(tl)


# ---- 7. config 3 at full size ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SCORERS)
def test_config_3_lists(ctx, name):
    """20 000 x 20 000 titles at ntop = 5: column 0 of all rows == the oracle's fixture (K8's answers), rows [0, 500) == the stable
    sort of the full score matrix of those rows"""
    from polyfuzz_amd import _lib, datasets
    fl, tl = datasets.c3_lists(20000)
    assert len(fl) == len(tl) == 20_000
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    idx, score, work = _lib.jaro_topn(ctx, f, t, name, 5, counters=True)
    print(f"K21 {name}, 20 000 x 20 000 titles, ntop 5: {({k: round(v / 4e8, 4) for k, v in work.items()})} of 4e8 pairs")
    e_idx, e_score = helpers.load_c3_jaro_golden(name)
    np.testing.assert_array_equal(idx[:, 0], e_idx)
    np.testing.assert_array_equal(score[:, 0], e_score)
    _assert_topn((idx[:500], score[:500]), expected_topn(_lib.jaro_matrix(ctx, f, t, name, 0, 500), 5), name)
    assert 0 < work["pairs_scored"] < 4e8


# ---- 8. the pool fill mode -------------------------------------------------------------------------------------------------------

def test_pool_fill(ctx, mixed):
    """the same bytes under the allocator's fill words 0x0, 0x1 and 0x0000000100000001: no list that nobody wrote is read"""
    from polyfuzz_amd import _lib
    fl, tl, sims = mixed
    seen = []
    try:
        for fill in (_lib.Context.POOL_FILL_ZERO, _lib.Context.POOL_FILL_ONE64, _lib.Context.POOL_FILL_ONE32):
            ctx.pool_fill(fill)
            f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
            got = _lib.jaro_topn(ctx, f, t, "jaro_winkler", 5) + _lib.jaro_topn(ctx, f, t, "jaro", 5, score_cutoff=0.8)
            _assert_topn(got[:2], expected_topn(sims["jaro_winkler"], 5), f"fill {fill}")
            seen.append(b"".join(x.tobytes() for x in got))
    finally:
        ctx.pool_fill(0)
    assert seen[0] == seen[1] == seen[2]


# ---- 9. the matcher --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("winkler", [True, False])
def test_matcher(ctx, golden, winkler):
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import JaroWinkler
    name = "jaro_winkler" if winkler else "jaro"
    t = golden["titles_lists"]
    fl = t["from_list"][:50] + ["", "new york mets", "mets  york new", "", t["to_list"][3]]
    tl = t["to_list"][:90] + ["york new mets", "", "new york yankees", "new york met"] + t["to_list"][:20]
    sim = jaro_oracle.matrix(fl, tl, name)
    e_idx, e_val = expected_topn(sim, 3)
    for normalize in (False, True):
        df = JaroWinkler(winkler=winkler, normalize=normalize).match(fl, tl, top_n=3)
        assert list(df.columns) == ["From", "To", "Similarity", "To_2", "Similarity_2", "To_3", "Similarity_3"]
        _assert_frame(df, _want_frame(fl, tl, e_idx, e_val, normalize))
    m = JaroWinkler(winkler=winkler, normalize=False)
    # at min_similarity 0 the first pair of columns is the top_n = 1 frame before normalisation
    best = m.match(fl, tl)
    assert list(best.columns) == ["From", "To", "Similarity"]
    df = m.match(fl, tl, top_n=3)
    assert df["To"].tolist() == best["To"].tolist()
    np.testing.assert_array_equal(df["Similarity"].to_numpy(), best["Similarity"].to_numpy())
    assert set(m.last_timings) == {"device", "frame"}
    # re_train=False: the resident to-list and its plan serve again
    m.match(fl[:5], tl, top_n=3)
    held = m._best._to_dev
    df = m.match(fl, list(tl), top_n=3, re_train=False)
    assert m._best._to_dev is held
    _assert_frame(df, _want_frame(fl, tl, e_idx, e_val, False))
    # the clip at a to-list of 2
    df = m.match(fl, tl[:2], top_n=3)
    assert list(df.columns) == ["From", "To", "Similarity", "To_2", "Similarity_2"]
    _assert_frame(df, _want_frame(fl, tl[:2], *expected_topn(sim[:, :2], 2), False))
    # a self-match with repeats: the from-string's own first occurrence is left out and nothing else
    dup = golden["titles_self_list"]["from_list"][:60] + golden["titles_self_list"]["from_list"][:15] + ["", ""]
    s_idx, s_val = expected_topn(jaro_oracle.matrix(dup, dup, name), 3, _first_occurrence(dup))
    for normalize in (False, True):
        _assert_frame(JaroWinkler(winkler=winkler, normalize=normalize).match(dup, top_n=3), _want_frame(dup, dup, s_idx, s_val, normalize))
    assert (s_val[:15, 0] == 1.0).all() and (s_idx[:15, 0] >= 60).all()          # (the repeated strings find their twins)
    # top_n = 1 is the plain call's frame
    for normalize in (False, True):
        m1 = JaroWinkler(winkler=winkler, normalize=normalize)
        assert m1.match(fl, tl, top_n=1).equals(JaroWinkler(winkler=winkler, normalize=normalize).match(fl, tl))
    with pytest.raises(_lib.PfzUnsupported, match="64"):
        m.match(fl, tl, top_n=70)                                                # 70 after clipping: beyond the 64 of a wave
    # a cutoff: cells below it are None / 0.0, and the scores stay unscaled whatever `normalize` says
    c_idx, c_val = _with_cutoff(expected_topn(sim, 3), 0.9)
    assert 0 < (c_idx >= 0).sum() < c_idx.size
    for normalize in (False, True):
        df = JaroWinkler(winkler=winkler, normalize=normalize).match(fl, tl, top_n=3, min_similarity=0.9)
        _assert_frame(df, _want_frame(fl, tl, c_idx, c_val, False))
    df = JaroWinkler(winkler=winkler).match(fl, tl, min_similarity=0.9)          # top_n 1 with a cutoff: the new path, one pair of columns
    _assert_frame(df, _want_frame(fl, tl, c_idx[:, :1], c_val[:, :1], False))
