"""K21, the n best choices under Jaro / Jaro-Winkler (pfz_jaro_topn), beside K8's arg-max and K20's threshold join on the same lists, as
arms of one run, in one process -- the protocol of tools/bench_topn.py and tools/bench_jaro_join.py.

usage: python tools/bench_jaro_topn.py [--titles 20000] [--companies 100000] [--repeats 9] [--out FILE]
                                       [--regress-parent FILE ...] [--regress-this FILE ...]

titles: BASELINE configuration 3, the 20 000 x 20 000 IMDB titles, both lists resident, the to-side plan built.  Arms per scorer:
  A  jaro_argmax (K8, the yardstick of the run);
  T  jaro_topn at ntop = 1 / 5 / 10 / 64, score_cutoff 0;      C  jaro_topn at ntop = 5, score_cutoff 0.9;
  J  jaro_join at 0.9 (K20), its capacity the exact total, for context.
companies: the 100 000 company names against themselves (two handles, no skip): A and T at ntop = 5.
All of them are the host entries: a pass ends when the result is in host memory.  Every arm is warmed (two passes), then the arms are
timed in turn over `repeats` rounds (>= 9) with device events around each pass.  One further, untimed pass per top-n arm brings the
four work counters.  Checked in the run: column 0 of every top-n arm at cutoff 0 == the arg-max, indices and float64 bits; under the
cutoff, wherever the arg-max reaches it.
--regress-parent / --regress-this: outputs (--out) of tools/bench_jaro.py and tools/bench_jaro_join.py of the parent commit's build
and of this one, taken in the same session (files of one tool share a basename prefix up to the last '_'); every timed arm's medians go
into the result side by side as `argmax_regression`, with the parent's own run-to-run spread as the margin.
Prints one JSON object; --out also writes it (default: profiles/jaro_topn_<commit>.json).  Run it under a time limit."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np

SCORERS = ("jaro_winkler", "jaro")
NTOPS = (1, 5, 10, 64)
CUTOFF = 0.9


def _commit():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "worktree"


def _stats(ms):
    return {"pass_ms_median": float(np.median(ms)), "pass_ms_min": float(min(ms)), "pass_ms_max": float(max(ms)),
            "pass_ms_all": [round(x, 4) for x in ms]}


def _timed_arms(node, path=""):
    """{path: pass_ms_median} of every timed arm in a bench output, whatever its nesting"""
    out = {}
    if isinstance(node, dict):
        if "pass_ms_median" in node:
            out[path] = node["pass_ms_median"]
        for k, v in node.items():
            out.update(_timed_arms(v, f"{path}/{k}" if path else k))
    return out


def _regression(parent_files, this_files):
    """per tool (the files' basename up to the last '_') and timed arm: the medians of every run of the parent's build and of this
    one, and whether this build's median of medians is at most the parent's plus the parent's own run-to-run spread (max - min)"""
    def by_tool(files):
        tools = {}
        for p in files:
            tools.setdefault(os.path.basename(p).rsplit("_", 1)[0], []).append(_timed_arms(json.load(open(p))))
        return tools
    parent, this = by_tool(parent_files), by_tool(this_files)
    out = {"protocol": "one process per run, the two builds in turn, same session", "tools": {}}
    for tool in parent:
        arms = {}
        for arm in parent[tool][0]:
            p, t = [r[arm] for r in parent[tool]], [r[arm] for r in this[tool]]
            spread = max(p) - min(p)
            arms[arm] = {"parent_pass_ms_medians": p, "this_pass_ms_medians": t, "parent_spread_ms": spread,
                         "this_median_over_parent_median": float(np.median(t) / np.median(p)),
                         "within_parent_spread": bool(np.median(t) <= np.median(p) + spread)}
        out["tools"][tool] = {"runs": [len(parent[tool]), len(this[tool])], "arms": arms}
    return out


def measure(ctx, _lib, name, f, t, scorer, arms, repeats):
    """arms: ("argmax",), ("topn", ntop, cutoff), ("join", threshold)"""
    pairs = f.n * t.n
    totals, last = {}, {}

    def run(arm, counters=False):
        if arm[0] == "argmax":
            return _lib.jaro_argmax(ctx, f, t, scorer)
        if arm[0] == "topn":
            return _lib.jaro_topn(ctx, f, t, scorer, arm[1], score_cutoff=arm[2], counters=counters)
        return _lib.jaro_join(ctx, f, t, scorer, arm[1], capacity=totals.get(arm))
    for arm in arms:                                  # warm-up: code objects, the pool's blocks, clocks; a join's exact total
        for _ in range(2):
            last[arm] = run(arm)
            if arm[0] == "join":
                totals[arm] = max(len(last[arm][1]), 1)
        print(f"[bench_jaro_topn] {name} {scorer} warmed {arm}", file=sys.stderr, flush=True)
    ctx.sync()
    ms = {arm: [] for arm in arms}
    for k in range(repeats):
        for arm in arms:
            ctx.event_record(0)
            run(arm)
            ctx.event_record(1)
            ctx.sync()
            ms[arm].append(ctx.event_elapsed_ms(0, 1))
        print(f"[bench_jaro_topn] {name} {scorer} round {k + 1} of {repeats}", file=sys.stderr, flush=True)
    a_idx, a_score = last[("argmax",)]
    res = {"shape": [f.n, t.n], "A_argmax": _stats(ms[("argmax",)])}
    base = res["A_argmax"]["pass_ms_median"]
    for arm in arms[1:]:
        r = _stats(ms[arm])
        r["over_A"] = r["pass_ms_median"] / base
        if arm[0] == "topn":
            _, ntop, cutoff = arm
            idx, score, work = run(arm, counters=True)
            rows = (a_idx >= 0) & (a_score >= cutoff)           # column 0 is the arg-max wherever the arg-max reaches the cutoff
            assert np.array_equal(idx[rows, 0], a_idx[rows]) and np.array_equal(score[rows, 0].view(np.int64), a_score[rows].view(np.int64)), arm
            assert (idx[~rows, 0] == -1).all(), arm
            r.update({"counters": work, "rows_checked_against_A": int(rows.sum()), "walked_share": work["pairs_walked"] / pairs,
                      "alive_share": work["pairs_alive_after_sweep1"] / pairs, "scored_share": work["pairs_scored"] / pairs,
                      "steps_per_pair": work["steps"] / pairs})
            res[f"T_top{ntop}" if cutoff == 0.0 else f"C_top{ntop}_cutoff{cutoff}"] = r
        else:
            r["hits"] = len(last[arm][1])
            res[f"J_join_t{arm[1]}"] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--titles", type=int, default=20_000)
    ap.add_argument("--companies", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--regress-parent", nargs="*", default=[])
    ap.add_argument("--regress-this", nargs="*", default=[])
    args = ap.parse_args()
    import polyfuzz_amd
    from polyfuzz_amd import _lib, datasets
    ctx = polyfuzz_amd.Context.default()
    repeats = max(args.repeats, 9)
    res = {"commit": _commit(), "device": ctx.info()["name"], "repeats": repeats,
           "entries": "host entries: a pass ends with the result in host memory; a join's capacity is the exact total", "data": {}}
    if args.titles > 0:
        fl, tl = datasets.c3_lists(args.titles)
        f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
        arms = [("argmax",)] + [("topn", k, 0.0) for k in NTOPS] + [("topn", 5, CUTOFF), ("join", CUTOFF)]
        res["data"]["titles"] = {s: measure(ctx, _lib, "titles", f, t, s, arms, repeats) for s in SCORERS}
    if args.companies > 0:
        names = datasets.load_company_names()[:args.companies]
        f, t = _lib.DeviceStrings.upload(ctx, names), _lib.DeviceStrings.upload(ctx, names)
        arms = [("argmax",), ("topn", 5, 0.0)]
        res["data"]["companies"] = {s: measure(ctx, _lib, "companies", f, t, s, arms, repeats) for s in SCORERS}
    if args.regress_parent and args.regress_this:
        res["argmax_regression"] = _regression(args.regress_parent, args.regress_this)
    print(json.dumps(res))
    out = args.out or os.path.join(REPO, "profiles", f"jaro_topn_{res['commit']}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
