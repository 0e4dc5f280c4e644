"""BlockedEditDistance (TF-IDF candidates rescored by K10) beside the all-pairs EditDistance on BASELINE configuration 3, the
20 000 x 20 000 IMDB titles, and on the 100 000 company names against themselves, in one process.

usage: python tools/bench_blocked.py [--n 20000] [--repeats 5] [--names 100000] [--skip-all-pairs-100k] [--commit ID] [--out FILE]

Titles, both lists resident (re_train=False after a first match), per scorer (ratio, levenshtein, osa, jaro, jaro_winkler):
  * BlockedEditDistance(scorer, candidates=c, top_n=1).match for c = 8, 32, 128: the wall time of a call (median of `repeats`) and
    its split into the TF-IDF stage, the K10 call (the to-list's K4 plan is cached: no preparation in it) and the frame
    (BlockedEditDistance.last_timings), and the K10 kernels' own time from one profiled pass;
  * EditDistance(scorer).match on the unchanged all-pairs path, in the same run, and the all-pairs arg-max entries alone
    (pfz_indel_argmax / pfz_lev_argmax / pfz_jaro_argmax: what the parent commit's profiles quote);
  * recall: the share of from-rows whose blocked best SCORE equals the all-pairs best score (scores, not indices: a tie may pick
    another index), and the share of rows that got no candidate at all.
Company names, self-match: the blocked time for candidates = 32 (levenshtein), the build time of the K4 plan of the 100 000 names
(K10 reads its code unit -> symbol table) measured on a fresh upload, and ONE all-pairs EditDistance("levenshtein") pass for
comparison (skipped with --skip-all-pairs-100k; run the tool under a time limit sized from the 20k figure x 25).
Prints one JSON object; --out also writes it (default: profiles/blocked_<commit>.json)."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np

SCORERS = ("ratio", "levenshtein", "osa", "jaro", "jaro_winkler")
CANDIDATES = (8, 32, 128)


def _commit():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "worktree"


def _median_ms(fn, repeats):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), [round(x, 3) for x in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--names", type=int, default=100_000)
    ap.add_argument("--skip-all-pairs-100k", action="store_true")
    ap.add_argument("--commit", default=None, help="the commit the tree was built from, where git cannot tell")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import polyfuzz_amd
    from polyfuzz_amd import _lib, datasets
    from polyfuzz_amd.models import BlockedEditDistance, EditDistance
    ctx = polyfuzz_amd.Context.default()
    fl, tl = datasets.c3_lists(args.n)
    res = {"commit": args.commit or _commit(), "device": ctx.info()["name"], "repeats": args.repeats,
           "titles": {"shape": [len(fl), len(tl)], "data": "datasets.c3_lists (IMDB titles)", "scorers": {}}}
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    entry = {"ratio": lambda: _lib.indel_argmax(ctx, f, t), "levenshtein": lambda: _lib.lev_argmax(ctx, f, t, "levenshtein"),
             "osa": lambda: _lib.lev_argmax(ctx, f, t, "osa"), "jaro": lambda: _lib.jaro_argmax(ctx, f, t, "jaro"),
             "jaro_winkler": lambda: _lib.jaro_argmax(ctx, f, t, "jaro_winkler")}
    for name in SCORERS:
        r = {}
        for _ in range(2):
            best = entry[name]()[1]                                   # (warm: code objects, the plan, the pool's blocks)
        r["all_pairs_argmax_entry_ms"], r["all_pairs_argmax_entry_ms_all"] = _median_ms(entry[name], args.repeats)
        ed = EditDistance(scorer=name, normalize=False)
        ed.match(fl, tl)
        r["all_pairs_match_ms"], r["all_pairs_match_ms_all"] = _median_ms(lambda: ed.match(fl, tl, re_train=False), args.repeats)
        r["blocked"] = {}
        for c in CANDIDATES:
            m = BlockedEditDistance(scorer=name, candidates=c, top_n=1, normalize=False)
            df = m.match(fl, tl)
            m.match(fl, tl, re_train=False)
            splits = []

            def once():
                m.match(fl, tl, re_train=False)
                splits.append(dict(m.last_timings))
            med, every = _median_ms(once, args.repeats)
            ctx.prof_enable(True)
            ctx.prof_reset()
            m.match(fl, tl, re_train=False)
            ctx.sync()
            k_ms = ctx.prof_get("k10_pairs")[0]
            ctx.prof_enable(False)
            got = df["Similarity"].to_numpy()
            none = df["To"].isna().to_numpy()
            r["blocked"][str(c)] = {
                "match_ms": med, "match_ms_all": every,
                "tfidf_ms": float(np.median([s["tfidf"] for s in splits])), "k10_call_ms": float(np.median([s["k10"] for s in splits])),
                "frame_ms": float(np.median([s["frame"] for s in splits])), "k10_kernels_ms_profiled_pass": k_ms,
                "recall_best_score_equals_all_pairs": float(np.mean(got == best)),
                "share_of_rows_without_candidate": float(np.mean(none)),
                "all_pairs_match_over_blocked_match": r["all_pairs_match_ms"] / med}
        res["titles"]["scorers"][name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)

    names = datasets.load_company_names()[:args.names]
    big = {"shape": [len(names), len(names)], "data": "datasets.load_company_names, self-match"}
    fresh = _lib.DeviceStrings.upload(ctx, names)
    ctx.sync()
    t0 = time.perf_counter()
    big["k4_plan"] = _lib.indel_plan_info(ctx, fresh)
    ctx.sync()
    big["k4_plan_build_ms"] = (time.perf_counter() - t0) * 1e3
    m = BlockedEditDistance(scorer="levenshtein", candidates=32, top_n=1, normalize=False)
    m.match(names)
    splits = []

    def once_big():
        m.match(names)
        splits.append(dict(m.last_timings))
    big["blocked_match_ms"], big["blocked_match_ms_all"] = _median_ms(once_big, max(3, args.repeats))
    for key in ("tfidf", "k10", "frame"):
        big[f"blocked_{key}_ms"] = float(np.median([s[key] for s in splits]))
    big["k10_includes_the_plan_build"] = True            # (a self-match uploads its list anew on every call: no cached plan)
    big["share_of_rows_without_candidate"] = float(np.mean(m.match(names)["To"].isna().to_numpy()))
    res["company_names"] = big
    out = args.out or os.path.join(REPO, "profiles", f"blocked_{res['commit']}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)

    def write():
        with open(out, "w") as fh:
            json.dump(res, fh, indent=1)
    write()                                              # (what is measured so far is kept if the long pass below is cut short)
    if not args.skip_all_pairs_100k:
        ed = EditDistance(scorer="levenshtein", normalize=False)
        t0 = time.perf_counter()
        ed.match(names)
        big["all_pairs_levenshtein_match_ms_one_pass"] = (time.perf_counter() - t0) * 1e3
        write()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
