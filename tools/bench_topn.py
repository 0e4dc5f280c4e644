"""The top-n forms of K4 (ratio) and K9 (Levenshtein, OSA) beside their arg-max entries on BASELINE configuration 3, the
20 000 x 20 000 IMDB titles, in one process -- the protocol of tools/bench_lev.py.

usage: python tools/bench_topn.py [--n 20000] [--repeats 9] [--out FILE]
                                  [--bench-lev-parent FILE ...] [--bench-lev-this FILE ...]

Both lists resident, the to-side plan built.  Arms, per scorer: the arg-max entry as it is (pfz_indel_argmax / pfz_lev_argmax), and
pfz_indel_topn / pfz_lev_topn at ntop = 1, 5, 10 and 64; for ratio also the arg-max entry with PFZ_K4_NO_QUAD=1 -- the one-string
kernel without a list, which separates the price of leaving the quad / octo kernels out from the price of the list.  All of them are
the host entries: a pass ends when the (rows x ntop) result is in host memory, so the ntop = 64 arms carry a 15 MB download.  Every
arm is warmed (three passes), then the arms are timed in turn over `repeats` rounds (>= 9) with device events around each pass; one
further profiled pass per arm (pfz_prof_*) gives the kernels' own time (k9_lev: the launches and the merge, no copy; k4_indel: up to
the entry's return) and, for K9, the number of pairs whose recurrence was walked.
--bench-lev-parent / --bench-lev-this: outputs of tools/bench_lev.py (--out) of the parent commit's build and of this one, taken in
the same session; their arg-max medians go into the result side by side, with the parent's own run-to-run spread as the margin.
Prints one JSON object; --out also writes it (default: profiles/topn_<commit>.json).  Run it under a time limit (timeout 600 ...)."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np

NTOPS = (1, 5, 10, 64)


def _commit():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "worktree"


def _argmax_regression(parent_files, this_files):
    """the arg-max arms of tools/bench_lev.py, parent build against this one: per arm the medians of every run, and whether this
    build's median of medians is at most the parent's median of medians plus the parent's own run-to-run spread (max - min)"""
    def load(files):
        return [json.load(open(p))["arms"] for p in files]
    parent, this = load(parent_files), load(this_files)
    out = {"protocol": "tools/bench_lev.py, one process per run, same session", "runs": [len(parent), len(this)], "arms": {}}
    for arm in parent[0]:
        p = [r[arm]["pass_ms_median"] for r in parent]
        t = [r[arm]["pass_ms_median"] for r in this]
        spread = max(p) - min(p)
        out["arms"][arm] = {"parent_pass_ms_medians": p, "this_pass_ms_medians": t, "parent_spread_ms": spread,
                            "this_median_over_parent_median": float(np.median(t) / np.median(p)),
                            "within_parent_spread": bool(np.median(t) <= np.median(p) + spread)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20_000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-lev-parent", nargs="*", default=[])
    ap.add_argument("--bench-lev-this", nargs="*", default=[])
    args = ap.parse_args()
    import polyfuzz_amd
    from polyfuzz_amd import _lib, datasets
    ctx = polyfuzz_amd.Context.default()
    fl, tl = datasets.c3_lists(args.n)
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    plan = _lib.indel_plan_info(ctx, t)

    def run(arm):
        scorer, form = arm
        if form == "argmax_no_quad":
            os.environ["PFZ_K4_NO_QUAD"] = "1"
            try:
                _lib.indel_argmax(ctx, f, t)
            finally:
                del os.environ["PFZ_K4_NO_QUAD"]
        elif scorer == "ratio":
            _lib.indel_argmax(ctx, f, t) if form == "argmax" else _lib.indel_topn(ctx, f, t, form)
        else:
            _lib.lev_argmax(ctx, f, t, scorer) if form == "argmax" else _lib.lev_topn(ctx, f, t, scorer, form)
    arms = []
    for scorer in ("ratio", "levenshtein", "osa"):
        arms += [(scorer, "argmax")] + ([(scorer, "argmax_no_quad")] if scorer == "ratio" else []) + [(scorer, k) for k in NTOPS]
    for arm in arms:                              # warm-up: code objects, the pool's blocks, clocks
        for _ in range(3):
            run(arm)
    ctx.sync()
    ms = {arm: [] for arm in arms}
    for _ in range(max(args.repeats, 9)):
        for arm in arms:
            ctx.event_record(0)
            run(arm)
            ctx.event_record(1)
            ctx.sync()
            ms[arm].append(ctx.event_elapsed_ms(0, 1))
    pairs = len(fl) * len(tl)
    res = {"commit": _commit(), "shape": [len(fl), len(tl)], "data": "datasets.c3_lists (IMDB titles)", "device": ctx.info()["name"],
           "repeats": max(args.repeats, 9), "plan": plan, "entries": "host entries: a pass ends with the result in host memory",
           "arms": {}}
    for arm in arms:
        scorer, form = arm
        ctx.prof_enable(True)
        ctx.prof_reset()
        run(arm)
        ctx.sync()
        kernel_ms, _ = ctx.prof_get("k4_indel" if scorer == "ratio" else "k9_lev")
        _, walked = ctx.prof_get("k9_pairs_walked")
        ctx.prof_enable(False)
        med, base = float(np.median(ms[arm])), float(np.median(ms[(scorer, "argmax")]))
        r = {"pass_ms_median": med, "pass_ms_min": float(min(ms[arm])), "pass_ms_max": float(max(ms[arm])),
             "pass_ms_all": [round(x, 4) for x in ms[arm]], "kernel_ms_profiled_pass": kernel_ms,
             "pass_over_argmax_pass_of_this_run": med / base}
        if scorer != "ratio":
            r["k9_pairs_walked"] = walked
            r["share_of_pairs_walked"] = walked / pairs
        res["arms"][f"{scorer}_{form if isinstance(form, str) else 'top' + str(form)}"] = r
    a = res["arms"]
    res["ratio_one_string_kernel_over_quad_octo"] = {
        "argmax_no_quad_over_argmax": a["ratio_argmax_no_quad"]["pass_ms_median"] / a["ratio_argmax"]["pass_ms_median"],
        "top1_over_argmax": a["ratio_top1"]["pass_ms_median"] / a["ratio_argmax"]["pass_ms_median"],
        "top1_over_argmax_no_quad": a["ratio_top1"]["pass_ms_median"] / a["ratio_argmax_no_quad"]["pass_ms_median"]}
    if args.bench_lev_parent and args.bench_lev_this:
        res["argmax_regression"] = _argmax_regression(args.bench_lev_parent, args.bench_lev_this)
    print(json.dumps(res))
    out = args.out or os.path.join(REPO, "profiles", f"topn_{res['commit']}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
