"""GPU parity of K8 (all-pairs Jaro / Jaro-Winkler + first arg-max) against the definition: every comparison is exact, == on
float64 scores and on indices.  The small shapes compare with the Python statement (tests/jaro_oracle.py); the shapes that reach
the pruning, the second row of a workgroup, the 16-bit symbols and the LDS limit need millions of pairs and compare with its C
restatement (oracle/jaro.c, held == the Python statement by tests/test_jaro_cpu.py).  PARITY UNPINNED beyond the oracle
(tests/test_jaro_cpu.py holds both to jellyfish wherever it is installed)."""
import contextlib
import pickle

import numpy as np
import pandas as pd
import pytest

from tests import helpers, jaro_oracle

pytestmark = pytest.mark.gpu

SCORERS = ("jaro", "jaro_winkler")


def _rand(rng, alpha, lo, hi, n):
    return ["".join(rng.choice(list(alpha), size=int(rng.integers(lo, hi + 1)))) for _ in range(n)]


def _first_occurrence(strings):
    first = {}
    for j, s in enumerate(strings):
        first.setdefault(s, j)
    return np.array([first[s] for s in strings], np.int32)


@pytest.fixture(scope="module")
def mixed(golden):
    """~120 x 250: real titles, the edge lengths of the register kernel's word classes (31 .. 65 on either side and on both;
    to-strings of 255 .. 257, where its four flag words end), strings far beyond them, characters the to-list never uses,
    code points above 255 and above 0xFFFF, dense strings over two letters, prefixes of 0..6 common characters around
    w = 0.7"""
    rng = np.random.default_rng(81)
    t = golden["titles_lists"]
    edge = [31, 32, 33, 63, 64, 65]
    base = "the quick brown fox jumps over the lazy dog and runs far away from home again"
    prefixes = ["abcdef"[:k] + "uvwxyz"[k:] + tail for k in range(7) for tail in ("", "mnopq", "qponm")]
    fl = (t["from_list"][:35] + ["", "a", "ab", "the matrix", "Z"] + [base[:n] for n in edge] + [base[::-1][:n] for n in edge] +
          ["ab" * 100, "naïve café Ωmega \U0001f600 smile", "qqq中文", "####", "\U0001f600\U0001f601"] + _rand(rng, "ab", 1, 70, 30) +
          prefixes[:14] + _rand(rng, "abcdefgh ", 60, 66, 10))
    tl = (t["to_list"][:100] + ["", "a", "ba", "the matrix", "The Matrix"] + [base[:n] for n in edge] + [base[3:3 + n] for n in edge] +
          ["ba" * 75, "naïve cafe Ωmega \U0001f601 smile \U0001f600", "中文qqq"] + [(base * 4)[:n] for n in (255, 256, 257)] + ["ab" * 150] + _rand(rng, "ab", 1, 70, 30) + prefixes +
          _rand(rng, "abcdefgh ", 60, 66, 20) + _rand(rng, "abc", 1, 9, 50))
    return fl, tl, {name: jaro_oracle.matrix(fl, tl, name) for name in SCORERS}


def test_matrix_bit_exact(ctx, mixed):
    from polyfuzz_amd import _lib
    fl, tl, want = mixed
    assert 110 <= len(fl) <= 130 and 230 <= len(tl) <= 270
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for name in SCORERS:
        got = _lib.jaro_matrix(ctx, f, t, name)
        np.testing.assert_array_equal(got, want[name], err_msg=name)
        idx, score = _lib.jaro_argmax(ctx, f, t, name)
        e_idx, e_score = jaro_oracle.argmax(want[name])
        np.testing.assert_array_equal(idx, e_idx)
        np.testing.assert_array_equal(score, e_score)
    part = _lib.jaro_matrix(ctx, f, t, "jaro_winkler", 30, 61)           # a row shard
    np.testing.assert_array_equal(part, want["jaro_winkler"][30:61])
    assert want["jaro_winkler"][fl.index("the matrix"), tl.index("the matrix")] == 1.0
    assert (want["jaro"][fl.index("")] == 0.0).all() and (want["jaro"][:, tl.index("")] == 0.0).all()


def test_invalid_scorer_is_refused(ctx):
    from polyfuzz_amd import _lib
    f = _lib.DeviceStrings.upload(ctx, ["a"])
    out = np.zeros(1)
    for scorer in (2, -1):
        assert ctx.lib.pfz_jaro_matrix_host(ctx.h, f.h, f.h, scorer, 0, 1, out.ctypes.data_as(_lib.c_vp)) == -1      # PFZ_ERR_INVALID
    with pytest.raises(KeyError):
        _lib.jaro_matrix(ctx, f, f, "ratio")


@pytest.fixture(scope="module")
def tied(golden):
    """~150 x 400 with every to-string present two or three times: ties in every row, the first index must win"""
    rng = np.random.default_rng(82)
    t = golden["titles_lists"]
    uniq = t["to_list"][:110] + _rand(rng, "ab", 1, 40, 30) + ["", "x" * 70, "the"]
    tl = uniq + uniq[::-1] + uniq[:114]
    fl = t["from_list"][:100] + _rand(rng, "ab", 1, 40, 40) + ["", "x" * 70, "y" * 66] + uniq[:7]
    return fl, tl, {name: jaro_oracle.matrix(fl, tl, name) for name in SCORERS}


def test_argmax_ties_and_skip_codes(ctx, tied):
    from polyfuzz_amd import _lib
    fl, tl, want = tied
    assert len(fl) == 150 and len(tl) == 400
    n = len(fl)
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    rng = np.random.default_rng(83)
    for name in SCORERS:
        plain = jaro_oracle.argmax(want[name])
        # a left-out index: the row's own best (the next equal string must win), -1 (nothing) for every fifth row
        one = plain[0].copy()
        one[::5] = -1
        # "everything up to": -2 - k leaves choices 0..k out; the last rows keep no candidate at all
        up_to = (-2 - rng.integers(0, len(tl) - 1, n)).astype(np.int32)
        up_to[::7] = -1
        up_to[-3:] = -2 - (len(tl) - 1)
        for skip in (None, one, up_to):
            e_idx, e_score = plain if skip is None else jaro_oracle.argmax(want[name], skip)
            idx, score = _lib.jaro_argmax(ctx, f, t, name, skip)
            np.testing.assert_array_equal(idx, e_idx, err_msg=name)
            np.testing.assert_array_equal(score, e_score, err_msg=name)
            out = _lib.DeviceTopN.alloc(ctx, n, 2)
            _lib.jaro_argmax_dev(ctx, f, t, name, out, skip)
            d_idx, d_score = _lib.best_from_topn(*out.download())
            np.testing.assert_array_equal(d_idx[:n], e_idx)
            np.testing.assert_array_equal(d_score[:n], e_score)
        assert (jaro_oracle.argmax(want[name], up_to)[0][-3:] == -1).all()
        assert (plain[0] < len(tl) - 114).all()                        # (every best has a later twin: ties did occur)
    idx2, _ = _lib.jaro_argmax(ctx, f, t, "jaro", None, 40, 90)        # a row shard
    np.testing.assert_array_equal(idx2, jaro_oracle.argmax(want["jaro"])[0][40:90])
    with pytest.raises(_lib.PfzError):
        _lib.jaro_argmax(ctx, f, t, "jaro", np.where(np.arange(n) % 2 == 0, 3, -5).astype(np.int32))     # both forms in one call


def test_few_rows_many_choices(ctx):
    """3 x 5 000: 79 groups of to-strings, split over many workgroups per from-string; the host and the device entry agree"""
    from polyfuzz_amd import _lib, datasets
    _, titles = datasets.c3_lists(5000)
    tl = titles[:5000]
    fl = [tl[1234], "the lord of the rings the return of the king", "ab"]
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for name in SCORERS:
        e_idx, e_score = jaro_oracle.argmax(jaro_oracle.matrix(fl, tl, name))
        idx, score = _lib.jaro_argmax(ctx, f, t, name)
        np.testing.assert_array_equal(idx, e_idx)
        np.testing.assert_array_equal(score, e_score)
        out = _lib.DeviceTopN.alloc(ctx, 3, 2)
        _lib.jaro_argmax_dev(ctx, f, t, name, out)
        d_idx, d_score = _lib.best_from_topn(*out.download())
        np.testing.assert_array_equal(d_idx[:3], e_idx)
        np.testing.assert_array_equal(d_score[:3], e_score)
    assert e_score[0] == 1.0 and tl[e_idx[0]] == tl[1234]


def _frame(fl, names, idx, score, normalize):
    df = pd.DataFrame({"From": fl, "To": [names[j] for j in idx], "Similarity": score})
    if normalize:           # reference _distance.py:83-86
        df["Similarity"] = (df["Similarity"] - df["Similarity"].min()) / (df["Similarity"].max() - df["Similarity"].min())
    return df


def test_matcher(ctx, golden):
    from polyfuzz_amd.models import EditDistance
    t = golden["titles_lists"]
    fl, tl = t["from_list"][:100], t["to_list"][:200]
    e_idx, e_score = jaro_oracle.argmax(jaro_oracle.matrix(fl, tl, "jaro_winkler"))
    for normalize in (False, True):
        model = EditDistance(scorer="jaro_winkler", normalize=normalize)
        df = model.match(fl, tl)
        want = _frame(fl, tl, e_idx, e_score, normalize)
        assert list(df.columns) == ["From", "To", "Similarity"]
        assert df["From"].tolist() == fl and df["To"].tolist() == want["To"].tolist()
        np.testing.assert_array_equal(df["Similarity"].to_numpy(), want["Similarity"].to_numpy())
    # re_train=False on the same list: the resident copy and its plan serve again
    model = EditDistance(scorer="jaro_winkler", normalize=False)
    model.match(fl[:10], tl)
    held = model._to_dev
    df = model.match(fl, list(tl), re_train=False)
    assert model._to_dev is held
    np.testing.assert_array_equal(df["Similarity"].to_numpy(), e_score)
    # a pickled matcher leaves its device handles behind and works after loading
    clone = pickle.loads(pickle.dumps(model))
    assert clone._to_dev is None and clone._scorer_name == "jaro_winkler"
    df = clone.match(fl, tl)
    assert df["To"].tolist() == [tl[j] for j in e_idx]
    np.testing.assert_array_equal(df["Similarity"].to_numpy(), e_score)
    # Jaro by name, and a self-match with repeats: the from-string's own first occurrence is left out
    dup = golden["titles_self_list"]["from_list"][:120] + golden["titles_self_list"]["from_list"][:30]
    s_idx, s_score = jaro_oracle.argmax(jaro_oracle.matrix(dup, dup, "jaro"), _first_occurrence(dup))
    df = EditDistance(scorer="jaro_similarity", normalize=False).match(dup)
    assert df["To"].tolist() == [dup[j] for j in s_idx]
    np.testing.assert_array_equal(df["Similarity"].to_numpy(), s_score)
    assert (s_score[:30] == 1.0).all()                  # (the repeats find their twins)


# ---- the paths only large shapes reach, against the C oracle ----------------------------------------------------------------------

@contextlib.contextmanager
def _k8_counters(ctx):
    """with _k8_counters(ctx) as box: ...K8 calls...  ->  box["scored"] = pairs whose float64 score the arg-max computed,
    box["general"] = launches of the general kernel, box["launches"] = timed K8 scopes (one per call)"""
    box = {}
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        yield box
        ctx.sync()
        box["scored"] = ctx.prof_get("k8_pairs_scored")[1]
        box["general"] = ctx.prof_get("k8_jaro_general")[1]
        box["launches"] = ctx.prof_get("k8_jaro")[1]
    finally:
        ctx.prof_enable(False)


def _left_out(n_to, skip):
    j = np.arange(n_to, dtype=np.int64)[None, :]
    sk = skip.astype(np.int64)[:, None]
    return (j == sk) | (j <= -2 - sk)


def _argmax(m, skip=None):
    """jaro_oracle.argmax, vectorised: np.argmax's first maximum over the choices `skip` leaves in (scores are >= 0)"""
    if skip is None:
        idx = m.argmax(axis=1).astype(np.int32)
        return idx, m[np.arange(len(m)), idx]
    out = _left_out(m.shape[1], skip)
    mm = np.where(out, -1.0, m)
    idx = mm.argmax(axis=1).astype(np.int32)
    score = mm[np.arange(len(m)), idx]
    none = out.all(axis=1)
    idx[none], score[none] = -1, 0.0
    return idx, score


def _dev_argmax(ctx, f, t, name, n, skip=None):
    from polyfuzz_amd import _lib
    out = _lib.DeviceTopN.alloc(ctx, n, 2)
    _lib.jaro_argmax_dev(ctx, f, t, name, out, skip)
    idx, score = _lib.best_from_topn(*out.download())
    return idx[:n], score[:n]


def _joined(rng, pool, length):
    """titles joined by blanks and cut to `length` characters"""
    s = pool[int(rng.integers(len(pool)))]
    while len(s) < length:
        s = s + " " + pool[int(rng.integers(len(pool)))]
    return s[:length]


def _twice_or_thrice(rng, uniq, n):
    """`n` strings: every one of `uniq` two or three times, at scattered positions (not in length order)"""
    assert 2 * len(uniq) <= n <= 3 * len(uniq)
    out = list(uniq) * 2 + list(uniq)[:n - 2 * len(uniq)]
    return [out[k] for k in rng.permutation(n)]


N_TO_LONG_LANES = 1024          # 16 groups: four per wave, and so four to-strings per lane


def long_lane_lists(cls, n_from):
    """(from_list of n_from strings, to_list of 1 024) of one launch class of the register kernel -- each call is one launch:
    '32x32'   both sides <= 32 characters (32-bit words);
    '32xwide' from <= 32, to 33 .. 256 (64-bit words, four flag words per lane), 64 / 65 / 128 / 129 / 192 / 193 / 255 / 256 present;
    '64xall'  from 33 .. 64 (33, 63, 64 present), to 1 .. 256.
    Every distinct to-string is there two or three times; some are from-strings, so some rows have perfect matches and twins of them."""
    from polyfuzz_amd import datasets
    titles_f, titles_t = datasets.c3_lists(20000)
    rng = np.random.default_rng({"32x32": 84, "32xwide": 85, "64xall": 86}[cls])
    n_uniq = 420
    if cls == "64xall":
        lens = [33, 63, 64] + rng.integers(33, 65, n_from - 3).tolist()
        fl = [_joined(rng, titles_f, n) for n in lens]
    else:
        fl = [s for s in titles_f if len(s) <= 32][:n_from]
    assert len(fl) == n_from
    if cls == "32x32":
        uniq = fl[5:1500:10] + [s for s in titles_t if 1 <= len(s) <= 32]
    elif cls == "32xwide":
        edge = [64, 65, 128, 129, 192, 193, 255, 256]
        uniq = [_joined(rng, titles_t, n) for n in edge + rng.integers(33, 257, 120).tolist()] + [s for s in titles_t if 33 <= len(s) <= 256]
    else:
        uniq = fl[5:1500:10] + [_joined(rng, titles_t, n) for n in [1, 2, 255, 256] + rng.integers(65, 257, 100).tolist()] + \
            [s for s in titles_t if 1 <= len(s) <= 256][:400]
    uniq = list(dict.fromkeys(uniq))[:n_uniq]
    assert len(uniq) == n_uniq
    return fl, _twice_or_thrice(rng, uniq, N_TO_LONG_LANES)


@pytest.fixture(scope="module")
def long_lanes(ctx):
    """the lists of a launch class, built once for both scorers; R = 32 x CUs from-strings: 4 x the largest grid, so the to-groups are
    not split (parts = 1) and every workgroup takes four from-strings in turn"""
    cache = {}
    n_from = 32 * ctx.info()["n_cu"]

    def get(cls):
        if cls not in cache:
            cache[cls] = long_lane_lists(cls, n_from)
        return cache[cls]
    return get


SCORED_SHARE_CAP = 0.85         # a condition (one to-string per lane gives exactly 1.0: nothing can be pruned), not a measurement


@pytest.mark.parametrize("name", SCORERS)
@pytest.mark.parametrize("cls", ["32x32", "32xwide", "64xall"])
def test_long_lanes_pruning_and_row_reuse(ctx, oracle_mod, long_lanes, cls, name):
    """One register launch per call (k8_jaro_kernel<uint32_t,8,1> / <uint64_t,8,4> with the rows of <= 32 / <uint64_t,8,4> with the
    rows of 33 .. 64), 32 x CUs from-strings against 1 024 to-strings: every lane meets four to-strings per from-string, so its
    running best prunes (the float32 bounds from m and with t, the key shortcut on the twins, the wave-level skip of sweep 2), and
    every workgroup takes four from-strings, so its LDS match table is cleared and reused.  Arg-max of all rows == the C oracle under
    the three skip forms (none; the row's own best choice -- where the from-string is in the to-list that is its first occurrence --
    so that the later twin must win; "up to" codes), through the host entry and jaro_argmax_dev.  That the paths ran: 0 launches of
    the general kernel, and the pairs scored in float64 are at most 0.85 of the pairs not left out.
    Measured on an MI355X (256 CUs, 8 192 from-strings), share of the pairs scored without skip / one choice / up to, the same for
    both scorers to four digits: 32x32 0.5773 / 0.5777 / 0.5907; 32xwide 0.5361 / 0.5367 / 0.5529; 64xall 0.6829 / 0.6835 / 0.6967
    (K8's rules simulated on the CPU in lane order: 0.58, 0.54, 0.68); 0.3 / 0.5 / 1.3 s per test, oracle included."""
    from polyfuzz_amd import _lib
    fl, tl = long_lanes(cls)
    n, n_to = len(fl), len(tl)
    lf, lt = np.array([len(s) for s in fl]), np.array([len(s) for s in tl])
    assert n == 32 * ctx.info()["n_cu"] and n_to == N_TO_LONG_LANES
    assert {"32x32": lf.max() <= 32 and lt.max() <= 32, "32xwide": lf.max() <= 32 and lt.min() >= 33 and lt.max() == 256,
            "64xall": lf.min() == 33 and lf.max() == 64 and lt.min() == 1 and lt.max() == 256}[cls]
    assert (np.diff(lt) < 0).sum() > n_to // 4 and max(tl.count(s) for s in tl[:50]) <= 3 and min(tl.count(s) for s in tl[:50]) >= 2
    want = helpers.jaro_oracle_matrix(oracle_mod, fl, tl, name)
    plain = _argmax(want)
    rng = np.random.default_rng(87)
    one = plain[0].copy()
    one[::5] = -1
    up_to = (-2 - rng.integers(0, 128, n)).astype(np.int32)
    up_to[::7] = -1
    up_to[-3:] = -2 - (n_to - 1)                     # no choice left
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for what, skip in (("no skip", None), ("one choice", one), ("up to", up_to)):
        e_idx, e_score = plain if skip is None else _argmax(want, skip)
        kept = n * n_to if skip is None else int((~_left_out(n_to, skip)).sum())
        with _k8_counters(ctx) as box:
            idx, score = _lib.jaro_argmax(ctx, f, t, name, skip)
        share = box["scored"] / kept
        print(f"K8 long lanes {cls} {name} {what}: {box['scored']} of {kept} pairs scored, share {share:.4f}")
        np.testing.assert_array_equal(idx, e_idx, err_msg=f"{cls} {name} {what}")
        np.testing.assert_array_equal(score, e_score, err_msg=f"{cls} {name} {what}")
        assert box["general"] == 0 and box["launches"] == 1
        assert share <= SCORED_SHARE_CAP, (cls, name, what, share)
        d_idx, d_score = _dev_argmax(ctx, f, t, name, n, skip)
        np.testing.assert_array_equal(d_idx, e_idx, err_msg=f"{cls} {name} {what} (device entry)")
        np.testing.assert_array_equal(d_score, e_score, err_msg=f"{cls} {name} {what} (device entry)")
    assert (plain[1] == 1.0).sum() >= (100 if cls != "32xwide" else 0)            # (from-strings that are in the to-list)
    # every to-string has a twin, the plain best is the first of its score: with it left out, a LATER choice of the same score wins
    s_idx, s_score = _argmax(want, one)
    assert (s_score[one >= 0] == plain[1][one >= 0]).all() and (s_idx[one >= 0] > one[one >= 0]).all()
    assert (_argmax(want, up_to)[0][-3:] == -1).all()


def wide_alphabet_lists():
    """~160 x 384 over about 300 code points (Latin, Greek, Cyrillic, a slice of CJK): the to-side plan packs 16-bit symbols"""
    rng = np.random.default_rng(88)
    alpha = [chr(c) for c in list(range(0x61, 0x7b)) + [0x20] + list(range(0x3b1, 0x3ca)) + list(range(0x430, 0x450)) + list(range(0x4e00, 0x4e00 + 216))]
    unused = [chr(c) for c in (0x41, 0x5a, 0x100, 0x400, 0x3000, 0x4dff, 0x4ee0)]          # below the table's end, not in the to-list
    beyond = [chr(c) for c in (0x4f00, 0x9fff, 0xffff, 0x1f600, 0x10ffff)]                  # above it
    hot = alpha[:27] + alpha[60:70] + alpha[100:110]      # (a skewed draw: matches must be frequent for the flags to matter)

    def mk(lo, hi, extra=()):
        pool = hot * 6 + alpha + list(extra)
        return "".join(pool[int(k)] for k in rng.integers(0, len(pool), int(rng.integers(lo, hi + 1))))
    tl = [mk(1, 32) for _ in range(150)] + [mk(33, 256) for _ in range(223)] + [mk(n, n) for n in (64, 65, 128, 129, 192, 193, 255, 256)] + \
        [mk(n, n) for n in (257, 280, 300)]
    tl[0] = "".join(alpha)[:32]
    for k in range(1, 10):                                 # every code point of the alphabet is used
        tl[150 + k] = "".join(alpha[(k - 1) * 34:k * 34])
    def edited(extra=(), hi=70):
        """a cut of a to-string: a fifth of its characters redrawn, a few swapped"""
        s = list(tl[int(rng.integers(len(tl)))])
        s = s[int(rng.integers(0, 3)):][:int(rng.integers(1, hi + 1))]
        pool = alpha + list(extra) * 8
        s = [c if rng.random() < 0.8 else pool[int(rng.integers(len(pool)))] for c in s]
        for _ in range(len(s) // 16):
            i, j = rng.integers(0, len(s), 2)
            s[i], s[j] = s[j], s[i]
        return "".join(s)
    fl = [""] + [mk(n, n) for n in (1, 31, 32, 33, 63, 64, 65, 70, 100, 129, 200)] + [mk(0, 70) for _ in range(20)] + \
        [edited() for _ in range(40)] + [edited(unused) for _ in range(40)] + [edited(beyond) for _ in range(30)] + \
        [edited(unused + beyond, 90) for _ in range(6)] + [tl[3], tl[160], tl[200][:64], tl[-1][:50], "".join(unused), "".join(beyond), "abc", tl[5][::-1]]
    tl = [tl[k] for k in rng.permutation(len(tl))]
    return fl, tl


def test_wide_alphabet_16bit_symbols(ctx, oracle_mod):
    """More than 255 distinct code points in the to-list: 16-bit symbols, so one call launches k8_jaro_kernel<uint32_t,16,1>,
    k8_jaro_kernel<uint64_t,16,4> (twice: the from-strings of <= 32 and of 33 .. 64) and k8_jaro_general_kernel<16> in both of its
    passes (the three to-strings beyond 256, the from-strings beyond 64).  From-characters in the alphabet, below the end of the
    symbol table but unused by the to-list, and above it.  Full matrix and arg-max == the C oracle."""
    from polyfuzz_amd import _lib
    fl, tl = wide_alphabet_lists()
    distinct = len({c for s in tl for c in s})
    assert 256 <= distinct < 7680 and 150 <= len(fl) <= 170 and len(tl) == 384
    lf, lt = np.array([len(s) for s in fl]), np.array([len(s) for s in tl])
    assert (lt <= 32).sum() >= 128 and ((lt > 32) & (lt <= 256)).sum() >= 128 and (lt > 256).sum() == 3 and lt.max() == 300
    assert lf.min() == 0 and (lf <= 32).sum() > 30 and ((lf > 32) & (lf <= 64)).sum() > 30 and (lf > 64).sum() >= 8
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for name in SCORERS:
        want = helpers.jaro_oracle_matrix(oracle_mod, fl, tl, name)
        with _k8_counters(ctx) as box:
            got = _lib.jaro_matrix(ctx, f, t, name)
        assert box["general"] == 2 and box["launches"] == 1
        np.testing.assert_array_equal(got, want, err_msg=name)
        e_idx, e_score = oracle_mod.jaro_argmax(fl, tl, name)
        np.testing.assert_array_equal(_argmax(want)[0], e_idx)
        for idx, score in (_lib.jaro_argmax(ctx, f, t, name), _dev_argmax(ctx, f, t, name, len(fl))):
            np.testing.assert_array_equal(idx, e_idx, err_msg=name)
            np.testing.assert_array_equal(score, e_score, err_msg=name)
        assert (want > 0.7).sum() > 50 and (e_score > 0).sum() >= 140


LDS_LIMIT_SYMBOLS = 7679        # (7 679 + 1) match-table entries of 8 bytes = 61 440 bytes = 60 KiB: the largest table that fits


def lds_limit_lists(distinct, max_from_len):
    """120 to-strings x 64 characters with exactly `distinct` code points among them (7 680: every character once; 7 679: one
    twice), and 48 from-strings made from the to-strings by seeded edits (cut, swap, drop, replace, repeat)"""
    assert distinct in (120 * 64, 120 * 64 - 1)
    rng = np.random.default_rng(89)
    cps = np.concatenate([np.arange(0x30, 0x7b), np.arange(0x3b1, 0x3ca), np.arange(0x4e00, 0x4e00 + 8000)])[:120 * 64].copy()
    if distinct < len(cps):
        cps[-1] = cps[17]
    cps = cps[rng.permutation(len(cps))] if distinct == len(cps) else np.concatenate([rng.permutation(cps[:-1]), cps[-1:]])
    tl = ["".join(chr(c) for c in cps[k * 64:(k + 1) * 64]) for k in range(120)]
    assert len({c for s in tl for c in s}) == distinct
    fl = []
    for k in range(48):
        s = list(tl[int(rng.integers(120))])
        kind = k % 6
        if kind == 0:
            s = s[:int(rng.integers(1, 65))]
        elif kind == 1:
            for _ in range(6):
                i, j = rng.integers(0, len(s), 2)
                s[i], s[j] = s[j], s[i]
        elif kind == 2:
            s = [c for c in s if rng.random() < 0.7]
        elif kind == 3:
            s = [c if rng.random() < 0.8 else tl[int(rng.integers(120))][int(rng.integers(64))] for c in s]
        elif kind == 4:
            s = (s[:20] + s[10:40] + s[:50])[:max_from_len]
        else:
            other = tl[int(rng.integers(120))]
            s = (s[:30] + list(other[20:60]) + s[30:])[:int(rng.integers(33, max_from_len + 1))]
        fl.append("".join(s))
    fl[-1], fl[-2] = tl[7], tl[100][:max_from_len] + tl[101][:max_from_len - 64]
    return fl, tl


@pytest.mark.parametrize("distinct", [LDS_LIMIT_SYMBOLS, LDS_LIMIT_SYMBOLS + 1])
def test_the_lds_limit_of_the_match_table(ctx, oracle_mod, distinct):
    """7 679 distinct code points in the to-list: the match table is 61 440 bytes of dynamic LDS (beside 48 static), the largest the
    register kernel is launched with -- it serves the whole call (no from-string beyond 64), 0 launches of the general kernel.
    7 680: one entry more, nothing fits, everything (from-strings up to 100 characters) is the general kernel's, one launch per call.
    Matrix and arg-max == the C oracle."""
    from polyfuzz_amd import _lib
    fits = distinct == LDS_LIMIT_SYMBOLS
    fl, tl = lds_limit_lists(distinct, 64 if fits else 100)
    assert ((distinct + 1) * 8 <= 60 * 1024) == fits and (not fits or (distinct + 1) * 8 == 61440)
    lf = np.array([len(s) for s in fl])
    assert len(fl) == 48 and len(tl) == 120 and all(len(s) == 64 for s in tl)
    assert lf.max() == (64 if fits else 100) and (lf <= 32).sum() >= 3 and ((lf > 32) & (lf <= 64)).sum() >= 10
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    for name in SCORERS:
        want = oracle_mod.jaro_matrix(fl, tl, name)
        e_idx, e_score = oracle_mod.jaro_argmax(fl, tl, name)
        with _k8_counters(ctx) as box:
            idx, score = _lib.jaro_argmax(ctx, f, t, name)
        assert box["general"] == (0 if fits else 1) and box["launches"] == 1
        np.testing.assert_array_equal(idx, e_idx, err_msg=name)
        np.testing.assert_array_equal(score, e_score, err_msg=name)
        with _k8_counters(ctx) as box:
            got = _lib.jaro_matrix(ctx, f, t, name)
        assert box["general"] == (0 if fits else 1)
        np.testing.assert_array_equal(got, want, err_msg=name)
        d_idx, d_score = _dev_argmax(ctx, f, t, name, len(fl))
        np.testing.assert_array_equal(d_idx, e_idx)
        np.testing.assert_array_equal(d_score, e_score)
        assert e_score[-1] == 1.0 and tl[e_idx[-1]] == tl[7] and (want > 0.5).sum() >= 40


def second_row_lists(n_from):
    rng = np.random.default_rng(90)
    mk = lambda alpha, n: "".join(alpha[int(k)] for k in rng.integers(0, len(alpha), n))
    lens = [128, 129, 140, 65, 64 + 64, 127] + rng.integers(65, 141, n_from - 6).tolist()
    fl = [mk("abcd", n) for n in lens]
    fl = [fl[k] for k in rng.permutation(n_from)]
    t_lens = [1, 2, 63, 64, 65, 128, 129, 192, 193, 256, 257, 300] + rng.integers(1, 301, 256 - 12).tolist()
    tl = [mk("abcd", n) for n in t_lens]
    for k in range(20):
        tl[20 + k] = fl[k * 131 % n_from]                    # (perfect matches, some of them in the second round)
    return fl, [tl[k] for k in rng.permutation(256)]


def test_general_kernel_takes_a_second_row(ctx, oracle_mod):
    """8 x CUs + 512 from-strings of 65 .. 140 characters (beyond the register kernel: all rows are the general kernel's, whose grid
    is 8 x CUs) over four letters, dense matches: 512 workgroups take a second from-string on a global-memory match table they have
    cleared, with from-side flags over three 64-bit words (128, 129 and 140 characters present).  256 to-strings of 1 .. 300: four
    groups, not split.  Arg-max of all rows, and the matrix of 64 rows either side of the first round's end, == the C oracle."""
    from polyfuzz_amd import _lib
    max_grid = 8 * ctx.info()["n_cu"]
    fl, tl = second_row_lists(max_grid + 512)
    lf, lt = np.array([len(s) for s in fl]), np.array([len(s) for s in tl])
    assert lf.min() == 65 and lf.max() == 140 and {128, 129, 140} <= set(lf.tolist()) and lt.min() == 1 and lt.max() == 300 and len(tl) == 256
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    lo, hi = max_grid - 32, max_grid + 32
    for name in SCORERS:
        e_idx, e_score = helpers.jaro_oracle_argmax(oracle_mod, fl, tl, name)
        with _k8_counters(ctx) as box:
            idx, score = _lib.jaro_argmax(ctx, f, t, name)
        assert box["general"] == 1 and box["launches"] == 1 and box["scored"] == len(fl) * len(tl)
        np.testing.assert_array_equal(idx, e_idx, err_msg=name)
        np.testing.assert_array_equal(score, e_score, err_msg=name)
        d_idx, d_score = _dev_argmax(ctx, f, t, name, len(fl))
        np.testing.assert_array_equal(d_idx, e_idx)
        np.testing.assert_array_equal(d_score, e_score)
        np.testing.assert_array_equal(_lib.jaro_matrix(ctx, f, t, name, lo, hi), oracle_mod.jaro_matrix(fl, tl, name, rows=(lo, hi)), err_msg=name)
        assert (e_score == 1.0).sum() >= 20 and (e_score[max_grid:] == 1.0).any()
