"""K11, the threshold join under Levenshtein / OSA similarity (pfz_lev_join), beside K9's all-pairs arg-max of the same run, on the
two data sets the package is measured on, in one process:

  titles     BASELINE configuration 3, the 20 000 x 20 000 IMDB titles, two-list form;
  companies  the 100 000 company names against themselves, self-join -- and the two-list form on the same list (a second upload),
             which walks every unordered pair twice and the diagonal.

usage: python tools/bench_join.py [--titles 20000] [--companies 100000] [--repeats 9] [--company-repeats 5] [--out FILE]

Both lists resident, the to-side plan built.  Arms, per data set and scorer: pfz_lev_argmax (every from-string's best; the
comparison the join is held to is THIS pass, of this run), and pfz_lev_join at t = 0.9, 0.8 and 0.6 with the capacity set to the
exact total (learned in the warm-up), so no timed call repeats itself.  All are host entries: a pass ends when the result is in
host memory.  Every arm is warmed, then the arms are timed in turn over `repeats` rounds with device events around each pass.  Two
further passes per join arm: one with the work counters -- pairs inside the length window and pairs walked to their end as shares
of all pairs, recurrence steps of live lanes as a share of all steps (every to-character of every pair) --, one profiled
(pfz_prof_*) for the split of the call: k11_join, the walk up to the total's arrival on the host, and k11_sort_unpack, the hits
sorted and turned into CSR; what is left of a pass is the download.
Prints one JSON object; --out also writes it (default: profiles/join_<commit>.json).  Run it under a time limit."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np

THRESHOLDS = (0.9, 0.8, 0.6)
SCORERS = ("levenshtein", "osa")


def _commit():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "worktree"


def _stats(ms):
    return {"pass_ms_median": float(np.median(ms)), "pass_ms_min": float(min(ms)), "pass_ms_max": float(max(ms)),
            "pass_ms_all": [round(x, 4) for x in ms]}


def measure(ctx, _lib, name, f, t, self_join, lens_from, lens_to, repeats):
    """one data set: f against t (two-list), and, for self_join, f against itself beside it"""
    n_from, n_to = len(lens_from), len(lens_to)
    forms = ("self", "two_list") if self_join else ("two_list",)
    if self_join:
        srt = np.sort(lens_from.astype(np.int64))
        all_pairs = {"self": n_from * (n_from - 1) // 2, "two_list": n_from * n_to}
        all_steps = {"self": int((np.arange(n_from, dtype=np.int64) * srt).sum()), "two_list": n_from * int(lens_to.sum())}
    else:
        all_pairs, all_steps = {"two_list": n_from * n_to}, {"two_list": n_from * int(lens_to.sum())}
    out = {"shape": [n_from, n_to], "forms": list(forms), "scorers": {}}
    for scorer in SCORERS:
        arms = [("argmax", None, None)] + [("join", form, thr) for form in forms for thr in THRESHOLDS]
        totals, hits = {}, {}

        def run(arm, counters=False):
            kind, form, thr = arm
            if kind == "argmax":
                return _lib.lev_argmax(ctx, f, t, scorer)
            return _lib.lev_join(ctx, f, None if form == "self" else t, scorer, thr, capacity=totals.get(arm), counters=counters)
        for arm in arms:                                  # warm-up: code objects, the pool's blocks, clocks; the exact totals
            for _ in range(2):
                r = run(arm)
                if arm[0] == "join":
                    hits[arm] = len(r[1])
                    totals[arm] = max(hits[arm], 1)
            print(f"[bench_join] {name} {scorer} warmed {arm}", file=sys.stderr, flush=True)
        ctx.sync()
        ms = {arm: [] for arm in arms}
        for k in range(repeats):
            for arm in arms:
                ctx.event_record(0)
                run(arm)
                ctx.event_record(1)
                ctx.sync()
                ms[arm].append(ctx.event_elapsed_ms(0, 1))
            print(f"[bench_join] {name} {scorer} round {k + 1} of {repeats}", file=sys.stderr, flush=True)
        res = {"argmax": _stats(ms[arms[0]])}
        base = res["argmax"]["pass_ms_median"]
        for arm in arms[1:]:
            _, form, thr = arm
            *_, work = run(arm, counters=True)
            ctx.prof_enable(True)
            ctx.prof_reset()
            run(arm)
            ctx.sync()
            walk_ms, sort_ms = ctx.prof_get("k11_join")[0], ctx.prof_get("k11_sort_unpack")[0]
            ctx.prof_enable(False)
            r = _stats(ms[arm])
            r.update({"hits": hits[arm],
                      "pass_over_argmax_pass_of_this_run": r["pass_ms_median"] / base,
                      "walk_ms_profiled_pass": walk_ms, "sort_unpack_ms_profiled_pass": sort_ms,
                      "pairs_in_window_share": work["pairs_in_window"] / all_pairs[form],
                      "pairs_finished_share": work["pairs_finished"] / all_pairs[form],
                      "steps_share": work["steps"] / all_steps[form], "counters": work})
            res[f"join_{form}_t{thr}"] = r
        if self_join:
            for thr in THRESHOLDS:
                res[f"join_self_t{thr}"]["two_list_pass_over_self_pass"] = \
                    res[f"join_two_list_t{thr}"]["pass_ms_median"] / res[f"join_self_t{thr}"]["pass_ms_median"]
        out["scorers"][scorer] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--titles", type=int, default=20_000)
    ap.add_argument("--companies", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--company-repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import polyfuzz_amd
    from polyfuzz_amd import _lib, datasets
    ctx = polyfuzz_amd.Context.default()
    lens = lambda strings: np.array([len(s) for s in strings], np.int64)
    res = {"commit": _commit(), "device": ctx.info()["name"], "thresholds": list(THRESHOLDS),
           "entries": "host entries: a pass ends with the result in host memory; the join's capacity is the exact total",
           "repeats": {"titles": args.repeats, "companies": args.company_repeats}, "data": {}}
    if args.titles > 0:
        fl, tl = datasets.c3_lists(args.titles)
        f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
        res["data"]["titles"] = measure(ctx, _lib, "titles", f, t, False, lens(fl), lens(tl), args.repeats)
    if args.companies > 0:
        names = datasets.load_company_names()[:args.companies]
        f, t = _lib.DeviceStrings.upload(ctx, names), _lib.DeviceStrings.upload(ctx, names)
        res["data"]["companies"] = measure(ctx, _lib, "companies", f, t, True, lens(names), lens(names), args.company_repeats)
    print(json.dumps(res))
    out = args.out or os.path.join(REPO, "profiles", f"join_{res['commit']}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
