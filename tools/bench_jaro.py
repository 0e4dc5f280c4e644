"""K8 (Jaro, Jaro-Winkler) beside K4 (ratio) on BASELINE configuration 3, the 20 000 x 20 000 IMDB titles, in one process.

usage: python tools/bench_jaro.py [--n 20000] [--repeats 9] [--out FILE]

Both lists resident, the to-side plan built (it is K4's, shared).  The three arms -- ratio, jaro, jaro_winkler -- are warmed
up and then timed in turn, `repeats` rounds of one best-choice pass each (the `_dev` entries: result left on the device),
with device events around the pass; a further profiled pass (pfz_prof_*) gives the kernels' own time (k4_indel / k8_jaro:
every launch of the pass, the merge included; k8_jaro_general: the general kernel's launches in it) and, for K8, the number
of pairs whose float64 score was computed.
Work figure: to-character steps = from-strings x sum of the padded to-string lengths (pfz_indel_plan_info), one sweep for K4,
two for K8.  Prints one JSON object; --out also writes it to a file.  Run it under a time limit (timeout 300 ...)."""
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
        else:
            _lib.jaro_argmax_dev(ctx, f, t, arm, out)
    arms = ("ratio", "jaro", "jaro_winkler")
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
        kernel_ms, _ = ctx.prof_get("k4_indel" if arm == "ratio" else "k8_jaro")
        _, scored = ctx.prof_get("k8_pairs_scored")
        general_ms, _ = ctx.prof_get("k8_jaro_general")
        ctx.prof_enable(False)
        med = float(np.median(ms[arm]))
        r = {"pass_ms_median": med, "pass_ms_min": float(min(ms[arm])), "pass_ms_max": float(max(ms[arm])),
             "pass_ms_all": [round(x, 4) for x in ms[arm]], "kernel_ms_profiled_pass": kernel_ms,
             "pairs_per_s": pairs / (med * 1e-3)}
        if arm != "ratio":
            r["general_kernel_ms_of_it"] = general_ms       # (strings beyond the register kernel's 64 / 256 characters)
            r["pairs_scored_in_float64"] = scored
            r["share_of_pairs_scored_in_float64"] = scored / pairs
            r["pass_over_ratio_pass"] = med / float(np.median(ms["ratio"]))
        res["arms"][arm] = r
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
