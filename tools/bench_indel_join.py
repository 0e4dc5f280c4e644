"""K13, the threshold join and the components under the Indel similarity (pfz_indel_join, pfz_indel_components), beside K11 / K12
under Levenshtein at the same thresholds and K4's all-pairs arg-max, as arms of one run, on the two data sets the package is
measured on, in one process:

  titles     BASELINE configuration 3, the 20 000 x 20 000 IMDB titles, two-list form;
  companies  the 100 000 company names against themselves: self-join, the two-list form on a second upload, and the components.

usage: python tools/bench_indel_join.py [--titles 20000] [--companies 100000] [--repeats 9] [--company-repeats 5] [--out FILE]

Both lists resident, the to-side plan built.  Arms per data set: pfz_indel_argmax (K4: every from-string's best under the same
metric, every pair walked), and per threshold t = 0.9, 0.8, 0.6 and form pfz_indel_join and pfz_lev_join (Levenshtein) with the
capacity set to the exact total (learned in the warm-up), so no timed call repeats itself; on the companies also
pfz_indel_components and pfz_lev_components.  All are host entries: a pass ends when the result (the CSR; the labels) is in host
memory.  Every arm is warmed twice, then the arms are timed in turn over `repeats` rounds with device events around each pass.
Two further passes per K13 join arm: one with the work counters -- pairs inside the length window and pairs walked to their end as
shares of all pairs, recurrence steps of live lanes as a share of all steps (every to-character of every pair) --, one profiled
(pfz_prof_*) for the split of the call: k13_join, the walk up to the total's arrival on the host, and k13_sort_unpack; what is left
of a pass is the download.  The components arms get the counter pass too.
Prints one JSON object; --out also writes it (default: profiles/indel_join_<commit>.json).  Run it under a time limit."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np

THRESHOLDS = (0.9, 0.8, 0.6)


def _commit():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "worktree"


def _stats(ms):
    return {"pass_ms_median": float(np.median(ms)), "pass_ms_min": float(min(ms)), "pass_ms_max": float(max(ms)),
            "pass_ms_all": [round(x, 4) for x in ms]}


def measure(ctx, _lib, name, f, t, self_join, lens_from, lens_to, repeats):
    """one data set: f against t (two-list), and, for self_join, f against itself and the components beside it"""
    n_from, n_to = len(lens_from), len(lens_to)
    forms = ("self", "two_list") if self_join else ("two_list",)
    all_pairs, all_steps = {"two_list": n_from * n_to}, {"two_list": n_from * int(lens_to.sum())}
    if self_join:
        srt = np.sort(lens_from.astype(np.int64))
        all_pairs["self"] = n_from * (n_from - 1) // 2
        all_steps["self"] = int((np.arange(n_from, dtype=np.int64) * srt).sum())
    arms = [("indel_argmax", None, None)]
    arms += [(kind, form, thr) for form in forms for thr in THRESHOLDS for kind in ("indel_join", "lev_join")]
    if self_join:
        arms += [(kind, "self", thr) for thr in THRESHOLDS for kind in ("indel_components", "lev_components")]
    totals, hits = {}, {}

    def run(arm, counters=False):
        kind, form, thr = arm
        to = None if form == "self" else t
        if kind == "indel_argmax":
            return _lib.indel_argmax(ctx, f, t)
        if kind == "indel_join":
            return _lib.indel_join(ctx, f, to, thr, capacity=totals.get(arm), counters=counters)
        if kind == "lev_join":
            return _lib.lev_join(ctx, f, to, "levenshtein", thr, capacity=totals.get(arm), counters=counters)
        if kind == "indel_components":
            return _lib.indel_components(ctx, f, thr, counters=counters)
        return _lib.lev_components(ctx, f, "levenshtein", thr, counters=counters)
    for arm in arms:                                  # warm-up: code objects, the pool's blocks, clocks; the exact totals
        for _ in range(2):
            r = run(arm)
            if arm[0].endswith("_join"):
                hits[arm] = len(r[1])
                totals[arm] = max(hits[arm], 1)
            elif arm[0].endswith("_components"):
                hits[arm] = r[1]
        print(f"[bench_indel_join] {name} warmed {arm}", file=sys.stderr, flush=True)
    ctx.sync()
    ms = {arm: [] for arm in arms}
    for k in range(repeats):
        for arm in arms:
            ctx.event_record(0)
            run(arm)
            ctx.event_record(1)
            ctx.sync()
            ms[arm].append(ctx.event_elapsed_ms(0, 1))
        print(f"[bench_indel_join] {name} round {k + 1} of {repeats}", file=sys.stderr, flush=True)
    res = {"shape": [n_from, n_to], "forms": list(forms), "indel_argmax": _stats(ms[arms[0]])}
    base = res["indel_argmax"]["pass_ms_median"]
    for arm in arms[1:]:
        kind, form, thr = arm
        r = _stats(ms[arm])
        r["hits"] = hits[arm]
        r["pass_over_indel_argmax_pass_of_this_run"] = r["pass_ms_median"] / base
        *_, work = run(arm, counters=True)
        r.update({"pairs_in_window_share": work["pairs_in_window"] / all_pairs[form],
                  "pairs_finished_share": work["pairs_finished"] / all_pairs[form],
                  "steps_share": work["steps"] / all_steps[form], "counters": work})
        if kind == "indel_join":
            ctx.prof_enable(True)
            ctx.prof_reset()
            run(arm)
            ctx.sync()
            r["walk_ms_profiled_pass"], r["sort_unpack_ms_profiled_pass"] = ctx.prof_get("k13_join")[0], ctx.prof_get("k13_sort_unpack")[0]
            ctx.prof_enable(False)
        if kind.startswith("indel_"):
            lev = _stats(ms[("lev_" + kind[6:], form, thr)])
            r["pass_over_lev_pass_same_t"] = r["pass_ms_median"] / lev["pass_ms_median"]
        res[f"{kind}_{form}_t{thr}"] = r
    return res


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
           "entries": "host entries: a pass ends with the result in host memory; a join's capacity is the exact total",
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
    out = args.out or os.path.join(REPO, "profiles", f"indel_join_{res['commit']}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
