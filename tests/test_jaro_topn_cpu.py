"""K21 -- the n best choices under Jaro / Jaro-Winkler (JaroWinkler.match(top_n=, min_similarity=), _lib.jaro_topn) -- without a GPU:
the entry point in header, library and ctypes table; the matcher's gates; the lemma the moving floor rests on (no k8_core.h rule
dismisses a pair at or above the threshold, for thresholds that ARE scores of pairs and their float64 neighbours); and the selection
scheme of csrc/k21_jaro_topn.hip emulated in Python and held to the stable sort of all scores, with its two broken variants shown
to fail (in the manner of tests/test_edit_topn_cpu.py)."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from tests.test_jaro_join_cpu import host_lib

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


# ---- the entry point -------------------------------------------------------------------------------------------------------

def test_entry_point_in_header_library_and_table():
    from polyfuzz_amd import _build, _lib
    if _build.is_stale():
        _build.build()
    header = open(os.path.join(REPO, "include", "polyfuzz_hip.h")).read()
    assert "int pfz_jaro_topn(" in header and hasattr(ctypes.CDLL(_lib.lib_path()), "pfz_jaro_topn") and "pfz_jaro_topn" in _lib.SIGNATURES
    assert _lib.SIGNATURES["pfz_jaro_topn"] == _lib.SIGNATURES["pfz_fuzz_topn"] and len(_lib.SIGNATURES["pfz_jaro_topn"][1]) == 12
    assert _lib.JARO_TOPN_COUNTERS == ("pairs_walked", "pairs_alive_after_sweep1", "pairs_scored", "steps")
    sig = inspect.signature(_lib.jaro_topn)
    assert list(sig.parameters) == list(inspect.signature(_lib.fuzz_topn).parameters)
    assert sig.parameters["score_cutoff"].default == 0.0 and sig.parameters["counters"].default is False


# ---- the matcher's gates ---------------------------------------------------------------------------------------------------

def _no_device(*a, **k):
    raise AssertionError("the device was reached")


def test_matcher_gates(monkeypatch):
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import JaroWinkler
    monkeypatch.setattr(_lib.Context, "default", classmethod(_no_device))
    fl, tl = ["a", "b", "c"], ["a", "c", "d"]
    params = inspect.signature(JaroWinkler.match).parameters
    assert params["top_n"].default == 1 and params["min_similarity"].default == 0.0
    for m in (JaroWinkler(), JaroWinkler(winkler=False)):
        for bad in (0, -1, True, False, 2.0, "3", None, [2]):
            with pytest.raises(ValueError, match="top_n"):
                m.match(fl, tl, top_n=bad)
        for bad in (float("nan"), float("inf"), -1e-300, np.nextafter(1.0, 2.0), 1.5, -0.1, "0.8", None, True, [0.8]):
            with pytest.raises(ValueError, match="min_similarity"):
                m.match(fl, tl, top_n=2, min_similarity=bad)
            with pytest.raises(ValueError, match="min_similarity"):
                m.match(fl, min_similarity=bad)
        for good in ({"top_n": 2}, {"top_n": np.int64(3)}, {"min_similarity": 0.5}, {"top_n": 1, "min_similarity": 1}, {},
                     {"top_n": 2, "min_similarity": np.float32(0.25)}, {"top_n": 64, "min_similarity": 0.0}):
            with pytest.raises(AssertionError, match="the device was reached"):      # accepted: the device is what stops these
                m.match(fl, tl, **good)
            with pytest.raises(AssertionError, match="the device was reached"):
                m.match(fl, **good)
        assert not hasattr(m, "top_n")
        with pytest.raises(_lib.PfzUnsupported, match="64"):                          # 65 after clipping, before the device
            m.match(["a"], [str(k) for k in range(70)], top_n=65)
        with pytest.raises(AssertionError, match="the device was reached"):          # 70 clips to the 3 choices
            m.match(fl, tl, top_n=70)
    assert "no top_n" not in JaroWinkler.__doc__ and "top_n" in JaroWinkler.match.__doc__


# ---- the moving floor's lemma ----------------------------------------------------------------------------------------------

def _score(m, tc, la, lb, prefix, winkler):
    """csrc/k8_core.h jaro_score on m matches and tc transpositions, the definition's order of operations"""
    if m == 0:
        return 0.0
    dm = float(m)
    w = (dm / float(la) + dm / float(lb) + float(m - tc) / dm) / 3.0
    if winkler and w > 0.7:
        w = w + (float(prefix) * 0.1) * (1.0 - w)
    return w


def _attainable(max_len):
    """every score a pair of lengths <= max_len can take, either scorer"""
    got = set()
    for la in range(1, max_len + 1):
        for lb in range(la, max_len + 1):
            for m in range(1, la + 1):
                for tc in range(m // 2 + 1):
                    got.add(_score(m, tc, la, lb, 0, 0))
                    for prefix in range(1, min(4, la) + 1):
                        got.add(_score(m, tc, la, lb, prefix, 1))
    return np.array(sorted(got))


def test_no_rule_dismisses_a_pair_at_or_above_a_floor_that_is_a_score():
    """The floor of K21 is not a round number: it is the score of some pair (the last entry of a full list) or the caller's cutoff.
    As thresholds: 1 600 scores that pairs of lengths <= 20 take (evenly over the sorted set of all of them, the lowest and the highest
    included), the float64 neighbour on either side of each, and 0.0 and 1.0.  Every dismissal rule of k8_core.h -- the length bound,
    m_need, the abandon rule at every split, the two bounds behind the sweeps -- must dismiss only pairs whose score is strictly below
    the threshold: 0 violations.  (This part passes without K21: it guards the argument, the GPU tests guard the kernel.)"""
    lib = host_lib()
    scores = _attainable(20)
    assert len(scores) > 5000 and scores[0] > 0.0 and scores[-1] == 1.0
    pick = scores[np.unique(np.linspace(0, len(scores) - 1, 1600).astype(np.int64))]
    assert len(pick) >= 1500
    thr = np.concatenate([pick, np.nextafter(pick, 2.0), np.nextafter(pick, -1.0), [0.0, 1.0]])
    thr = np.unique(thr[(thr >= 0.0) & (thr <= 1.0)])
    assert len(thr) >= 4500
    dismissed = np.zeros(len(thr), np.int64)
    bad = lib.k20_host_dismissals(20, len(thr), thr.ctypes.data_as(ctypes.c_void_p), dismissed.ctypes.data_as(ctypes.c_void_p))
    print(f"{len(thr)} thresholds, {int(dismissed.sum())} dismissals, {bad} violations")
    assert bad == 0
    assert dismissed[0] == 0 and (dismissed[1:] > 0).all()                # (nothing at 0.0; every other threshold does dismiss)


# ---- the scheme, emulated --------------------------------------------------------------------------------------------------

def _len_bound(la, lb, winkler):
    """what jaro_len_ok holds against the floor, exactly: every character of the shorter string matched, none transposed, the
    longest prefix the lengths allow"""
    mn = min(la, lb)
    return _score(mn, 0, la, lb, min(4, mn), winkler) if mn else 0.0


def _left_out(j, skip, up_to):
    return j <= skip if up_to else j == skip


def _expected(scores, out, ntop, cutoff):
    keep = np.flatnonzero(~out & (scores >= cutoff))
    order = keep[np.argsort(-scores[keep], kind="stable")][:ntop]
    idx, val = np.full(ntop, -1, np.int64), np.zeros(ntop)
    idx[:len(order)], val[:len(order)] = order, scores[order]
    return idx, val


def _model(la, lens, scores, keys, winkler, ntop, cutoff, skip, up_to, parts, rng, strict=True, key_shortcut=False):
    """One from-string of length `la` against to-strings of lengths `lens` with float64 scores `scores`, as k21_topn_kernel selects:
    the to-strings sorted by length (stable) into groups of 64; group g belongs to wave g % (4 * parts), the four waves of a part
    sharing the floor word W; a wave visits its groups from the one nearest |a| outwards, alternately up and down, and keeps ONE
    sorted list of ntop (score, index) keys.  Per group F = max(cutoff, W) is read once; the group is skipped unless a choice still in
    has its length bound >= F, and a direction ends where every real string of the group fails and lies on the far side of |a|; a
    pair is dismissed where its score -- standing in for the bounds, which are never below it -- is < F (strict=False: <= F, the
    broken variant); a scored pair >= cutoff is offered to the list; a full list raises W to its last entry's score.
    key_shortcut: K8's "same (m, t, |b|, prefix) as the lane's best: skip", the other broken variant.  The waves of a part take turns
    in random order.  Returns (idx[ntop], score[ntop], pairs scored)."""
    n_to = len(lens)
    order = np.argsort(lens, kind="stable")
    n_groups = (n_to + 63) // 64
    orig = np.full(n_groups * 64, -1, np.int64)
    orig[:n_to] = order
    g_len = np.where(orig >= 0, lens[np.maximum(orig, 0)], 0)
    g_max = [int(g_len[g * 64:(g + 1) * 64].max()) for g in range(n_groups)]
    below = (lambda s, f: s < f) if strict else (lambda s, f: s <= f and f > 0.0)
    lists, scored = [], 0
    for part in range(parts):
        W = 0.0
        waves = []
        for w in range(4):
            mine = list(range(w + 4 * part, n_groups, 4 * parts))
            lo = next((k for k, g in enumerate(mine) if g_max[g] >= la), len(mine))
            waves.append({"groups": mine, "up": lo, "down": lo - 1, "turn_up": True, "list": [], "lane_best": [None] * 64})
        live = [w for w in waves if w["groups"]]
        while live:
            wv = live[int(rng.integers(len(live)))]
            K = len(wv["groups"])
            if not (wv["up"] < K or wv["down"] >= 0):
                live.remove(wv)
                continue
            go_up = wv["up"] < K and (wv["turn_up"] or wv["down"] < 0)
            wv["turn_up"] = not go_up
            if go_up:
                g = wv["groups"][wv["up"]]
                wv["up"] += 1
            else:
                g = wv["groups"][wv["down"]]
                wv["down"] -= 1
            F = max(cutoff, W)
            lanes = [(int(orig[s]), int(g_len[s])) for s in range(g * 64, g * 64 + 64)]
            real = [j >= 0 for j, _ in lanes]
            out = [not r or _left_out(j, skip, up_to) for (j, _), r in zip(lanes, real)]
            fails = [below(_len_bound(la, lb, winkler), F) for _, lb in lanes]
            if not any(not o and not f for o, f in zip(out, fails)):
                if not any(r and not (f and (lb >= la if go_up else lb <= la)) for r, f, (_, lb) in zip(real, fails, lanes)):
                    if go_up:
                        wv["up"] = K
                    else:
                        wv["down"] = -1
                continue
            for lane, ((j, lb), o, f) in enumerate(zip(lanes, out, fails)):
                if o or f or below(scores[j], F):
                    continue
                if key_shortcut:
                    if wv["lane_best"][lane] is not None and keys[j] == wv["lane_best"][lane][1]:
                        continue
                    if wv["lane_best"][lane] is None or scores[j] > wv["lane_best"][lane][0]:
                        wv["lane_best"][lane] = (scores[j], keys[j])
                scored += 1
                if scores[j] >= cutoff:
                    wv["list"].append((-scores[j], j))
            wv["list"] = sorted(wv["list"])[:ntop]
            if len(wv["list"]) == ntop:
                W = max(W, -wv["list"][-1][0])
        lists += [w["list"] for w in waves]
    best = sorted(k for l in lists for k in l)[:ntop]
    idx, val = np.full(ntop, -1, np.int64), np.zeros(ntop)
    for p, (s, j) in enumerate(best):
        idx[p], val[p] = j, -s
    return idx, val, scored


def _cases():
    """(la, lens, scores, keys, winkler, skip, up_to, parts): few distinct lengths, hundreds of to-strings each, (m, t, prefix) drawn
    from a handful of values -- heavy ties, many of them in one lane's path, and scores that equal their length bound; both skip forms;
    rows with fewer choices than ntop; an empty from-string"""
    rng = np.random.default_rng(2121)
    out = []
    for la, pool, n_to in ((12, [6, 8, 9, 12, 16, 18, 24], 1500), (12, [12], 700), (5, [0, 1, 5, 10, 25], 900), (0, [0, 1, 2, 3], 600),
                           (30, [10, 28, 29, 30, 31, 32, 90], 2100), (7, [3, 7, 7, 7, 14], 40), (9, [9, 18], 3)):
        for winkler in (0, 1):
            lens = rng.choice(pool, n_to)
            keys, scores = [], np.zeros(n_to)
            for j, lb in enumerate(lens.tolist()):
                mn = min(la, lb)
                m = max(0, mn - int(rng.choice([0, 0, 0, 1, 2, 5])))
                tc = int(rng.choice([0, 0, 1])) if m >= 2 else 0
                prefix = min(4, mn, m) if rng.random() < 0.6 else min(int(rng.integers(0, 5)), mn, m)
                keys.append((m, tc, lb, prefix))
                scores[j] = _score(m, tc, la, lb, prefix, winkler)
                assert scores[j] <= _len_bound(la, lb, winkler)
            for parts in (1, 3):
                out.append((la, lens, scores, keys, winkler, -1, 0, parts))
                out.append((la, lens, scores, keys, winkler, int(rng.integers(n_to)), 0, parts))      # one choice left out
                out.append((la, lens, scores, keys, winkler, int(rng.integers(n_to)), 1, parts))      # everything up to it
            out.append((la, lens, scores, keys, winkler, n_to - 3, 1, 2))                             # two choices left
            out.append((la, lens, scores, keys, winkler, n_to - 1, 1, 1))                             # none
    # twins in one lane's path: 512 to-strings of one length, the second 256 copies of the first -- eight groups, wave w has the
    # groups w and w + 4, so a lane meets a string and then its copy; the copy belongs in every top-n its original is in
    combos = [(m, tc, 30, p) for m in range(1, 31) for tc in range(m // 2 + 1) for p in range(0, min(4, m) + 1)]
    for winkler in (0, 1):
        half = [combos[int(k)] for k in rng.choice(len(combos), 256, replace=False)]
        keys = half + half
        scores = np.array([_score(m, tc, 30, lb, p, winkler) for m, tc, lb, p in keys])
        for skip, up_to in ((-1, 0), (int(np.argmax(scores)), 0), (100, 1)):
            out.append((30, np.full(512, 30), scores, keys, winkler, skip, up_to, 1))
    return out


NTOPS = (1, 2, 5, 64)


def _run(**variant):
    rng = np.random.default_rng(21)
    wrong = total = pruned = 0
    for la, lens, scores, keys, winkler, skip, up_to, parts in _cases():
        out = np.array([_left_out(j, skip, up_to) for j in range(len(lens))])
        attained = float(np.sort(scores)[len(scores) // 2])
        for ntop in NTOPS:
            for cutoff in (0.0, 0.7, attained, float(np.nextafter(attained, 2.0))):
                e_idx, e_val = _expected(scores, out, ntop, cutoff)
                idx, val, scored = _model(la, lens, scores, keys, winkler, ntop, cutoff, skip, up_to, parts, rng, **variant)
                wrong += not (np.array_equal(idx, e_idx) and np.array_equal(val, e_val))
                total += 1
                pruned += scored < int((~out).sum())
    return wrong, total, pruned


def test_selection_scheme_equals_the_stable_sort():
    wrong, total, pruned = _run()
    assert wrong == 0 and total > 1000
    assert pruned >= total // 4               # (the floor did leave pairs out: the model is not the exhaustive walk)


def test_the_two_broken_variants_are_caught():
    """K8's equal-key shortcut carried over loses the later twins of a lane's best; dismissing at "<= floor" loses choices that tie
    with the list's last entry and have the lower index.  These inputs must show both, or the test above proves nothing about them."""
    wrong_key, total, _ = _run(key_shortcut=True)
    wrong_tie, _, _ = _run(strict=False)
    print(f"equal-key shortcut: {wrong_key} of {total} cases wrong; dismissal at <= floor: {wrong_tie} of {total}")
    assert wrong_key >= 10 and wrong_tie >= 10
