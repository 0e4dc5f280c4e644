"""K19, the n best choices under K7's scorers (pfz_fuzz_topn), beside K7's arg-max and K18's threshold join on the same lists, as
arms of one run in one process: BASELINE configuration 3, the 20 000 x 20 000 IMDB titles, both lists resident (forms and plan
built), under WRatio and partial_ratio.

usage: python tools/bench_fuzz_topn.py [--titles 20000] [--repeats 5] [--out FILE]

Arms per scorer:
  A  fuzz_extract_one_dev (K7's arg-max: seeds, a bound cache and a second sweep against one rising floor; the result stays on
     the device);
  B  fuzz_join at 0.9 (K18: the same walk against a fixed floor), the capacity set to the exact total learned in the warm-up;
  T  fuzz_topn at ntop = 1 / 5 / 10 / 64, score_cutoff 0 (K19: that walk, the floor rising with the wave's list); a pass ends with
     the result in host memory.
Every arm is warmed, then the arms are timed in turn over `repeats` rounds with device events around each call; the median is
reported, T / A as it comes out, and the growth from ntop = 1.  One further pass per arm brings the work counters: pairs bounded,
pairs scored, and the share of all pairs that was scored.
Checked in the run: column 0 of every T arm against A's answers (index and score bits), and the columns of a smaller ntop against
the first columns of ntop = 64.
Prints one JSON object; --out also writes it (default: profiles/fuzz_topn_<commit>.json).  Run it under a time limit."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np

SCORERS = ("WRatio", "partial_ratio")
NTOPS = (1, 5, 10, 64)
JOIN_T = 0.9


def _commit():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "worktree"


def _stats(ms):
    return {"pass_ms_median": float(np.median(ms)), "pass_ms_min": float(min(ms)), "pass_ms_max": float(max(ms)),
            "pass_ms_all": [round(x, 4) for x in ms]}


def measure(ctx, _lib, f, t, scorer, repeats):
    n_pairs = f.n * t.n
    out = _lib.DeviceTopN.alloc(ctx, f.n, 2)
    arms = [("argmax", None), ("join", JOIN_T)] + [("topn", n) for n in NTOPS]
    state = {"capacity": None}

    def run(arm, counters=False):
        kind, p = arm
        if kind == "argmax":
            return _lib.fuzz_extract_one_dev(ctx, f, t, scorer, out, counters=counters)
        if kind == "join":
            return _lib.fuzz_join(ctx, f, t, scorer, p * 100.0, capacity=state["capacity"], counters=counters)
        return _lib.fuzz_topn(ctx, f, t, scorer, p, counters=counters)
    last = {}
    for arm in arms:                                  # warm-up: code objects, the pool's blocks, clocks; the join's exact total
        for _ in range(2):
            last[arm] = run(arm)
            if arm[0] == "join":
                state["capacity"] = max(len(last[arm][1]), 1)
        print(f"[bench_fuzz_topn] {scorer} warmed {arm}", file=sys.stderr, flush=True)
    ctx.sync()
    best = _lib.best_from_topn(*out.download())
    best = best[0][:f.n], best[1][:f.n]
    ms = {arm: [] for arm in arms}
    for k in range(repeats):
        for arm in arms:
            ctx.event_record(0)
            run(arm)
            ctx.event_record(1)
            ctx.sync()
            ms[arm].append(ctx.event_elapsed_ms(0, 1))
        print(f"[bench_fuzz_topn] {scorer} round {k + 1} of {repeats}", file=sys.stderr, flush=True)
    res = {"shape": [f.n, t.n]}
    a = _stats(ms[arms[0]])
    work = run(arms[0], counters=True)
    a.update({"counters": work, "scored_share": work["pairs_scored"] / n_pairs})
    res["A_argmax"] = a
    b = _stats(ms[arms[1]])
    work = run(arms[1], counters=True)[-1]
    b.update({"over_A": b["pass_ms_median"] / a["pass_ms_median"], "hits": len(last[arms[1]][1]), "counters": work,
              "scored_share": work["scored"] / n_pairs})
    res[f"B_join_t{JOIN_T}"] = b
    widest = last[("topn", NTOPS[-1])]
    base = None
    for arm in arms[2:]:
        ntop = arm[1]
        idx, score = last[arm]
        assert np.array_equal(idx[:, 0], best[0]) and np.array_equal(score[:, 0].view(np.int64), best[1].view(np.int64)), \
            f"column 0 at ntop = {ntop} is not the arg-max's answer"
        assert np.array_equal(idx, widest[0][:, :ntop]) and np.array_equal(score.view(np.int64), widest[1][:, :ntop].view(np.int64)), \
            f"ntop = {ntop} is not the head of ntop = {NTOPS[-1]}"
        r = _stats(ms[arm])
        base = base or r["pass_ms_median"]
        work = run(arm, counters=True)[-1]
        r.update({"over_A": r["pass_ms_median"] / a["pass_ms_median"], "over_ntop_1": r["pass_ms_median"] / base, "counters": work,
                  "scored_share": work["scored"] / n_pairs, "checked_against_A": True})
        res[f"T_topn_{ntop}"] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--titles", type=int, default=20_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import polyfuzz_amd
    from polyfuzz_amd import _lib, datasets
    ctx = polyfuzz_amd.Context.default()
    res = {"commit": _commit(), "device": ctx.info()["name"], "repeats": args.repeats,
           "entries": "A leaves its result on the device; B and T end with the result in host memory", "data": {}}
    fl, tl = datasets.c3_lists(args.titles)
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    res["data"]["titles"] = {s: measure(ctx, _lib, f, t, s, args.repeats) for s in SCORERS}
    print(json.dumps(res))
    out = args.out or os.path.join(REPO, "profiles", f"fuzz_topn_{res['commit']}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
