"""K9 (Levenshtein, OSA) beside K4 (ratio) and K8 (jaro) on BASELINE configuration 3, the 20 000 x 20 000 IMDB titles, in one
process.

usage: python tools/bench_lev.py [--n 20000] [--repeats 9] [--out FILE]

Both lists resident, the to-side plan built (it is K4's, shared).  The four arms -- ratio, jaro, levenshtein, osa -- are warmed
(three passes each), then timed in turn over `repeats` rounds (>= 9), each pass with device events around it; a further profiled
pass (pfz_prof_*) gives the kernels' own time (k4_indel / k8_jaro / k9_lev: every launch of the pass, the merge included;
k9_lev_general: the general kernel's launches in it) and, for K9, the number of pairs whose recurrence was walked -- the others
fell to the length bound.  K4 and K8 are the yardsticks: one sweep of the LCS recurrence per pair, two sweeps of Jaro's, one sweep
of about twice the LCS step for K9 -- over the pairs it walks.  Prints one JSON object; --out also writes it to a file.  Run it
under a time limit (timeout 300 ...)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20_000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import polyfuzz_amd
    from polyfuzz_amd import _lib, datasets
    ctx = polyfuzz_amd.Context.default()
    fl, tl = datasets.c3_lists(args.n)
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    out = _lib.DeviceTopN.alloc(ctx, len(fl), 2)
    plan = _lib.indel_plan_info(ctx, t)

    def run(arm):
        if arm == "ratio":
            _lib.indel_argmax_dev(ctx, f, t, out)
        elif arm == "jaro":
            _lib.jaro_argmax_dev(ctx, f, t, arm, out)
        else:
            _lib.lev_argmax_dev(ctx, f, t, arm, out)
    arms = ("ratio", "jaro", "levenshtein", "osa")
    for arm in arms:                              # warm-up: code objects, the pool's blocks, clocks
        for _ in range(3):
            run(arm)
    ctx.sync()
    ms = {arm: [] for arm in arms}
    for _ in range(args.repeats):
        for arm in arms:
            ctx.event_record(0)
            run(arm)
            ctx.event_record(1)
            ctx.sync()
            ms[arm].append(ctx.event_elapsed_ms(0, 1))
    lens = np.array([len(s) for s in fl])
    res = {"shape": [len(fl), len(tl)], "data": "datasets.c3_lists (IMDB titles)", "device": ctx.info()["name"], "repeats": args.repeats,
           "plan": plan, "from_strings_beyond_64": int((lens > 64).sum()), "to_strings_beyond_64": int(sum(len(s) > 64 for s in tl)),
           "to_char_steps_per_sweep": len(fl) * plan["char_steps"], "arms": {}}
    pairs = len(fl) * len(tl)
    for arm in arms:
        ctx.prof_enable(True)
        ctx.prof_reset()
        run(arm)
        ctx.sync()
        kernel_ms, _ = ctx.prof_get({"ratio": "k4_indel", "jaro": "k8_jaro"}.get(arm, "k9_lev"))
        _, walked = ctx.prof_get("k9_pairs_walked")
        general_ms, _ = ctx.prof_get("k9_lev_general")
        ctx.prof_enable(False)
        med = float(np.median(ms[arm]))
        r = {"pass_ms_median": med, "pass_ms_min": float(min(ms[arm])), "pass_ms_max": float(max(ms[arm])),
             "pass_ms_all": [round(x, 4) for x in ms[arm]], "kernel_ms_profiled_pass": kernel_ms,
             "pairs_per_s": pairs / (med * 1e-3)}
        if arm in _lib.LEV_SCORERS:
            r["general_kernel_ms_of_it"] = general_ms       # (from-strings beyond the register kernel's 64 characters)
            r["k9_pairs_walked"] = walked
            r["share_of_pairs_walked"] = walked / pairs
        if arm != "ratio":
            r["pass_over_ratio_pass"] = med / float(np.median(ms["ratio"]))
            r["pass_over_jaro_pass"] = med / float(np.median(ms["jaro"]))
        res["arms"][arm] = r
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
