"""EditDistance.top_n without a device: the selection scheme of csrc/topn_wave.h and of K9's top-n kernel, emulated in Python and held
to the stable sort of all scores (in the manner of tests/test_symmetric_logic_cpu.py), and the matcher's own surface -- the
attribute, its validation, pickling, the scorers without a top-n form."""
import pickle

import numpy as np
import pytest


# ---- the argument, emulated -------------------------------------------------------------------------------------------

def _sim(d, la, lb):
    """K9's score (csrc/k9_core.h lev_similarity): 1.0 - d / max in float64, 1.0 for two empty strings; the length bound is the same
    formula on d = ||a| - |b||"""
    m = max(la, lb)
    return 1.0 - float(d) / float(m) if m else 1.0


def _left_out(j, skip, up_to):
    return j <= skip if up_to else j == skip


def _expected(scores, out, ntop):
    """np.argsort(-scores, kind="stable")[:ntop] over the choices left in; -1 / 0.0 beyond them"""
    keep = np.flatnonzero(~out)
    order = keep[np.argsort(-scores[keep], kind="stable")][:ntop]
    idx, val = np.full(ntop, -1, np.int64), np.zeros(ntop)
    idx[:len(order)], val[:len(order)] = order, scores[order]
    return idx, val


def _model(la, lens, dist, ntop, skip, up_to, parts, rng, strict=True):
    """One from-string of length `la` against to-strings of lengths `lens` at distances `dist`, as the top-n kernel selects:
    the to-strings sorted by length (stable) into groups of 64; group g belongs to wave g % (4 * parts), the waves w, w + 4, ...
    of one part sharing a threshold; a wave visits its groups from the one nearest |a| outwards, alternately up and down, keeps ONE
    sorted list of ntop (score, index) keys, and after every group a full list raises the part's threshold to its last entry's
    score; a group is walked unless every choice it still offers has its length bound strictly below the threshold (strict=False:
    at or below -- the broken variant), and a direction ends where that holds for every string of the group, the left-out ones
    too, on the far side of |a|.  The waves of a part take turns in random order (on the device they run side by side).
    Returns (idx[ntop], score[ntop], pairs walked)."""
    n_to = len(lens)
    order = np.argsort(lens, kind="stable")
    n_groups = (n_to + 63) // 64
    orig = np.full(n_groups * 64, -1, np.int64)
    orig[:n_to] = order
    g_len = np.where(orig >= 0, lens[np.maximum(orig, 0)], 0)
    g_max = [int(g_len[g * 64:(g + 1) * 64].max()) for g in range(n_groups)]
    lists, walked = [], 0
    for part in range(parts):
        thr = 0.0
        waves = []
        for w in range(4):
            base, stride = w + 4 * part, 4 * parts
            mine = list(range(base, n_groups, stride))
            lo = next((k for k, g in enumerate(mine) if g_max[g] >= la), len(mine))
            waves.append({"groups": mine, "up": lo, "down": lo - 1, "turn_up": True, "list": []})
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
            lanes = [(int(orig[s]), int(g_len[s])) for s in range(g * 64, g * 64 + 64)]
            real = [j >= 0 for j, _ in lanes]
            out = [not r or _left_out(j, skip, up_to) for (j, _), r in zip(lanes, real)]
            bound = [_sim(abs(la - lb), la, lb) for _, lb in lanes]
            below = [b < thr if strict else b <= thr for b in bound]
            if not any(not o and not b for o, b in zip(out, below)):
                if not any(r and not (b and (lb >= la if go_up else lb <= la)) for r, b, (_, lb) in zip(real, below, lanes)):
                    if go_up:
                        wv["up"] = K
                    else:
                        wv["down"] = -1
                continue
            walked += sum(real)
            for (j, lb), o in zip(lanes, out):
                if not o:
                    wv["list"].append((-_sim(dist[j], la, lb), j))
            wv["list"] = sorted(wv["list"])[:ntop]
            if len(wv["list"]) == ntop:
                thr = max(thr, -wv["list"][-1][0])
        lists += [w["list"] for w in waves]
    best = sorted(k for l in lists for k in l)[:ntop]
    idx, val = np.full(ntop, -1, np.int64), np.zeros(ntop)
    for p, (s, j) in enumerate(best):
        idx[p], val[p] = j, -s
    return idx, val, walked


def _cases():
    """(la, lens, dist, skip, up_to, parts): few distinct lengths, hundreds of to-strings each (several groups of one length: equal
    bounds), d = the length difference plus 0 .. 2 -- integer-valued, heavy ties, and many scores that EQUAL their bound; lengths on
    both sides of |a| whose bounds coincide (|a| = 12: 6 and 24, 8 and 18, 9 and 16); both skip forms; rows with fewer choices than ntop"""
    rng = np.random.default_rng(2024)
    out = []
    for la, pool, n_to in ((12, [6, 8, 9, 12, 16, 18, 24], 1500), (12, [12], 700), (5, [0, 1, 5, 10, 25], 900), (0, [0, 1, 2, 3], 600),
                           (30, [10, 28, 29, 30, 31, 32, 90], 2100), (7, [3, 7, 7, 7, 14], 40), (9, [9, 18], 3)):
        lens = rng.choice(pool, n_to)
        extra = rng.choice([0, 0, 0, 1, 2], n_to)
        dist = np.minimum(np.abs(la - lens) + extra, np.maximum(la, lens))
        for parts in (1, 3):
            out.append((la, lens, dist, -1, 0, parts))
            out.append((la, lens, dist, int(rng.integers(n_to)), 0, parts))           # one choice left out
            out.append((la, lens, dist, int(rng.integers(n_to)), 1, parts))           # everything up to it
        out.append((la, lens, dist, n_to - 3, 1, 2))                                  # two choices left: fewer than any ntop > 2
        out.append((la, lens, dist, n_to - 1, 1, 1))                                  # none
    return out


NTOPS = (1, 2, 5, 64)


def test_selection_scheme_equals_the_stable_sort():
    rng = np.random.default_rng(7)
    pruned = 0
    for la, lens, dist, skip, up_to, parts in _cases():
        scores = np.array([_sim(d, la, lb) for d, lb in zip(dist, lens)])
        out = np.array([_left_out(j, skip, up_to) for j in range(len(lens))])
        for ntop in NTOPS:
            e_idx, e_val = _expected(scores, out, ntop)
            idx, val, walked = _model(la, lens, dist, ntop, skip, up_to, parts, rng)
            np.testing.assert_array_equal(idx, e_idx, err_msg=f"la {la} n_to {len(lens)} ntop {ntop} skip {skip}/{up_to} parts {parts}")
            np.testing.assert_array_equal(val, e_val)
            pruned += walked < len(lens)
    assert pruned >= 20               # (the threshold did leave groups out: the model is not the exhaustive walk)


def test_skipping_at_an_equal_bound_is_caught():
    """the broken variant -- skip where bound <= threshold -- loses choices that tie with the list's last entry and have the lower
    index: this test's inputs must show it, or the test above proves nothing about the strictness"""
    rng = np.random.default_rng(7)
    wrong = total = 0
    for la, lens, dist, skip, up_to, parts in _cases():
        scores = np.array([_sim(d, la, lb) for d, lb in zip(dist, lens)])
        out = np.array([_left_out(j, skip, up_to) for j in range(len(lens))])
        for ntop in NTOPS:
            e_idx, _ = _expected(scores, out, ntop)
            idx, _, _ = _model(la, lens, dist, ntop, skip, up_to, parts, rng, strict=False)
            wrong += not np.array_equal(idx, e_idx)
            total += 1
    print(f"broken variant: {wrong} of {total} cases wrong")
    assert wrong >= 10


# ---- the matcher's surface --------------------------------------------------------------------------------------------

def test_top_n_attribute():
    from polyfuzz_amd.models import EditDistance
    m = EditDistance(scorer="levenshtein")
    assert m.top_n == 1
    m.top_n = 5
    assert m.top_n == 5
    m.top_n = np.int64(3)
    assert m.top_n == 3 and type(m.top_n) is int
    for bad in (0, -1, True, False, 2.0, "3", None, [2]):
        with pytest.raises(ValueError):
            m.top_n = bad
    assert m.top_n == 3
    clone = pickle.loads(pickle.dumps(m))
    assert clone.top_n == 3 and clone._scorer_name == "levenshtein" and clone._to_dev is None
    assert pickle.loads(pickle.dumps(EditDistance())).top_n == 1
    assert "top_n" in EditDistance.__doc__


@pytest.mark.parametrize("scorer", ["jaro", "jaro_winkler", "WRatio", "partial_ratio", "token_set_ratio"])
def test_scorers_without_a_top_n_form_raise_before_any_device_call(scorer, monkeypatch):
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import EditDistance

    def no_device(*a, **k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(_lib.Context, "default", classmethod(no_device))
    m = EditDistance(scorer=scorer)
    m.top_n = 3                                       # (setting it alone does not raise)
    with pytest.raises(NotImplementedError) as e:
        m.match(["a", "b"], ["a", "c", "d"])
    assert not isinstance(e.value, _lib.PfzError)
    for name in ("ratio", "levenshtein", "osa"):
        assert name in str(e.value)


def test_more_than_64_columns_after_clipping_is_unsupported(monkeypatch):
    from polyfuzz_amd import _lib
    from polyfuzz_amd.models import EditDistance

    def no_device(*a, **k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(_lib.Context, "default", classmethod(no_device))
    m = EditDistance(scorer="osa")
    m.top_n = 65
    with pytest.raises(_lib.PfzUnsupported, match="64"):
        m.match(["a"], [str(k) for k in range(70)])
