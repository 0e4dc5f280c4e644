"""K20, the threshold join and the components under Jaro / Jaro-Winkler (pfz_jaro_join, pfz_jaro_components), beside K8's arg-max on
the same lists and the blocked join (K16) it replaces on this score, as arms of one run, in one process:

  titles     BASELINE configuration 3, the 20 000 x 20 000 IMDB titles, two-list form;
  companies  the 100 000 company names against themselves: the two-list form on a second upload, the self-join, the components;
both under jaro_winkler and jaro at t = 0.95, 0.9, 0.8.

usage: python tools/bench_jaro_join.py [--titles 20000] [--companies 100000] [--repeats 5] [--blocked 32,128] [--out FILE]

The lists are resident, the plan built.  Arms per data set and scorer:
  A  pfz_jaro_argmax_dev (K8's arg-max, the result left on the device);
  B  jaro_join on two handles;         C  the self-join (companies);         D  jaro_components (companies);
  E  BlockedEditDistance(scorer, candidates=32 / 128).join on the titles -- the matcher's whole call, blocking included, wall clock --
     with its pair recall against B;
the joins with the capacity set to the exact total (learned in the warm-up), so no timed call repeats itself.  B, C and D are host
entries: a pass ends when the result (the CSR; the labels) is in host memory.  Every arm is warmed, then the arms are timed in turn
over `repeats` rounds with device events around each pass; the median is reported, and B / A as it comes out.  One further pass per
threshold arm brings the four work counters.
Checked in the run: B's rows with hits against A's answers (a row has hits iff A's best reaches t; its maximum is A's score), C's
total against D's pairs.
Prints one JSON object; --out also writes it (default: profiles/jaro_join_<commit>.json).  Run it under a time limit."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np

SCORERS = ("jaro_winkler", "jaro")
THRESHOLDS = (0.95, 0.9, 0.8)


def _commit():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "worktree"


def _stats(ms):
    return {"pass_ms_median": float(np.median(ms)), "pass_ms_min": float(min(ms)), "pass_ms_max": float(max(ms)),
            "pass_ms_all": [round(x, 4) for x in ms]}


def check_maxima(join, best, thr):
    """B against A: a row has hits iff A's best reaches t; its maximum is A's score"""
    row_ptr, idx, score = join
    a_idx, a_score = best
    counts = np.diff(row_ptr)
    has = (a_idx >= 0) & (a_score >= thr)
    assert np.array_equal(counts > 0, has), "rows with hits differ from the rows whose best reaches the threshold"
    if not has.any():
        return 0
    row_max = np.maximum.reduceat(score, row_ptr[:-1][has])
    assert np.array_equal(row_max.view(np.int64), a_score[has].view(np.int64)), "a row's maximum is not the arg-max's score"
    return int(has.sum())


def measure(ctx, _lib, name, f, t, scorer, self_forms, repeats):
    n_from, n_to = f.n, t.n
    arms = [("argmax", None)] + [("join", thr) for thr in THRESHOLDS]
    if self_forms:
        arms += [(kind, thr) for thr in THRESHOLDS for kind in ("self_join", "components")]
    totals, last = {}, {}
    out = _lib.DeviceTopN.alloc(ctx, max(n_from, 1), 2)

    def run(arm, counters=False):
        kind, thr = arm
        if kind == "argmax":
            return _lib.jaro_argmax_dev(ctx, f, t, scorer, out)
        if kind == "join":
            return _lib.jaro_join(ctx, f, t, scorer, thr, capacity=totals.get(arm), counters=counters)
        if kind == "self_join":
            return _lib.jaro_join(ctx, f, None, scorer, thr, capacity=totals.get(arm), counters=counters)
        return _lib.jaro_components(ctx, f, scorer, thr, counters=counters)
    for arm in arms:                                  # warm-up: code objects, the pool's blocks, clocks; the exact totals
        for _ in range(2):
            last[arm] = run(arm)
            if arm[0].endswith("join"):
                totals[arm] = max(len(last[arm][1]), 1)
        print(f"[bench_jaro_join] {name} {scorer} warmed {arm}", file=sys.stderr, flush=True)
    ctx.sync()
    best = tuple(x[:n_from] for x in _lib.best_from_topn(*out.download()))
    ms = {arm: [] for arm in arms}
    for k in range(repeats):
        for arm in arms:
            ctx.event_record(0)
            run(arm)
            ctx.event_record(1)
            ctx.sync()
            ms[arm].append(ctx.event_elapsed_ms(0, 1))
        print(f"[bench_jaro_join] {name} {scorer} round {k + 1} of {repeats}", file=sys.stderr, flush=True)
    res = {"shape": [n_from, n_to], "A_argmax_dev": _stats(ms[arms[0]])}
    base = res["A_argmax_dev"]["pass_ms_median"]
    letter = {"join": "B_join", "self_join": "C_self_join", "components": "D_components"}
    for arm in arms[1:]:
        kind, thr = arm
        r = _stats(ms[arm])
        r["over_A"] = r["pass_ms_median"] / base
        work = run(arm, counters=True)[-1]
        all_pairs = n_from * n_to if kind == "join" else n_from * (n_from - 1) // 2
        r.update({"counters": work, "window_share": work["pairs_in_window"] / all_pairs,
                  "alive_share": work["pairs_alive_after_sweep1"] / all_pairs, "scored_share": work["pairs_scored"] / all_pairs})
        if kind == "join":
            r["hits"] = len(last[arm][1])
            r["rows_checked_against_A"] = check_maxima(last[arm], best, thr)
        elif kind == "self_join":
            r["hits"] = len(last[arm][1])
        else:
            label, pairs, components = last[arm]
            assert pairs == len(last[("self_join", thr)][1])
            r.update({"hits": pairs, "components": components})
        res[f"{letter[kind]}_t{thr}"] = r
    return res, last


def blocked(from_list, to_list, scorer, candidates, exact, repeats):
    """arm E: the blocked join's wall clock (the matcher's whole call) and its pair recall against B's pairs"""
    from polyfuzz_amd.models import BlockedEditDistance
    res = {}
    for c in candidates:
        m = BlockedEditDistance(scorer=scorer, candidates=c, top_n=1, normalize=False)
        for thr in THRESHOLDS:
            frame = m.join(from_list, to_list, thr)                    # (warm)
            ms = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                m.join(from_list, to_list, thr)
                ms.append((time.perf_counter() - t0) * 1e3)
            row_ptr, idx, _ = exact[("join", thr)]
            r = _stats(ms)
            r.update({"pairs": len(frame), "exact_pairs": len(idx), "pair_recall": len(frame) / len(idx) if len(idx) else None})
            res[f"E_blocked{c}_t{thr}"] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--titles", type=int, default=20_000)
    ap.add_argument("--companies", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--blocked", default="32,128")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import polyfuzz_amd
    from polyfuzz_amd import _lib, datasets
    ctx = polyfuzz_amd.Context.default()
    cands = [int(c) for c in args.blocked.split(",") if c]
    res = {"commit": _commit(), "device": ctx.info()["name"], "repeats": args.repeats,
           "entries": "A: device entry (enqueued, timed to its end); B, C, D: host entries, a join's capacity is the exact total; "
                      "E: the matcher's call, wall clock", "data": {}}
    if args.titles > 0:
        fl, tl = datasets.c3_lists(args.titles)
        f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
        res["data"]["titles"] = {}
        for s in SCORERS:
            r, last = measure(ctx, _lib, "titles", f, t, s, False, args.repeats)
            r.update(blocked(fl, tl, s, cands, last, max(1, args.repeats // 2)))
            res["data"]["titles"][s] = r
    if args.companies > 0:
        names = datasets.load_company_names()[:args.companies]
        f, t = _lib.DeviceStrings.upload(ctx, names), _lib.DeviceStrings.upload(ctx, names)
        res["data"]["companies"] = {s: measure(ctx, _lib, "companies", f, t, s, True, args.repeats)[0] for s in SCORERS}
    print(json.dumps(res))
    out = args.out or os.path.join(REPO, "profiles", f"jaro_join_{res['commit']}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
