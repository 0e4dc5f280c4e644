"""K18, the threshold join and the components over K7's scorers (pfz_fuzz_join, pfz_fuzz_components), beside K7's arg-max on the
same lists, as arms of one run, on the two data sets the package is measured on, in one process:

  titles     BASELINE configuration 3, the 20 000 x 20 000 IMDB titles, two-list form, WRatio and partial_ratio at t = 0.95, 0.9, 0.8;
  companies  the 100 000 company names against themselves under WRatio at t = 0.95, 0.9: the two-list form on a second upload,
             the self-join and the components.

usage: python tools/bench_fuzz_join.py [--titles 20000] [--companies 100000] [--repeats 5] [--out FILE]

The lists are resident, forms and plan built.  Arms per data set and scorer:
  A  fuzz_extract_one (K7's arg-max);
  B  fuzz_join on two handles;         C  the self-join (companies);         D  fuzz_components (companies);
the joins with the capacity set to the exact total (learned in the warm-up), so no timed call repeats itself.  All are host entries:
a pass ends when the result (best choices; the CSR; the labels) is in host memory.  Every arm is warmed, then the arms are timed in
turn over `repeats` rounds with device events around each pass; the median is reported, and B / A as it comes out.  One further
pass per threshold arm brings the work counters (pairs bounded, pairs scored, hits).
Checked in the run: B's per-row maxima against A's answers (wherever A's best reaches the cutoff: score bits, and the smallest
to-index among the maxima), and D's labels against scipy's connected components of C's CSR.
Prints one JSON object; --out also writes it (default: profiles/fuzz_join_<commit>.json).  Run it under a time limit."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np

TITLE_ARMS = {"WRatio": (0.95, 0.9, 0.8), "partial_ratio": (0.95, 0.9, 0.8)}
COMPANY_ARMS = {"WRatio": (0.95, 0.9)}


def _commit():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "worktree"


def _stats(ms):
    return {"pass_ms_median": float(np.median(ms)), "pass_ms_min": float(min(ms)), "pass_ms_max": float(max(ms)),
            "pass_ms_all": [round(x, 4) for x in ms]}


def check_maxima(join, best, cutoff):
    """B against A: a row has hits iff A's best reaches the cutoff; its maximum is A's score, its first maximum A's index"""
    row_ptr, idx, score = join
    a_idx, a_score = best
    n = len(a_idx)
    counts = np.diff(row_ptr)
    has = a_score >= cutoff
    assert np.array_equal(counts > 0, has), "rows with hits differ from the rows whose best reaches the cutoff"
    if not has.any():
        return 0
    row_max = np.maximum.reduceat(score, row_ptr[:-1][has])
    assert np.array_equal(row_max.view(np.int64), a_score[has].view(np.int64)), "a row's maximum is not the arg-max's score"
    is_max = score == np.repeat(row_max, counts[has])
    first = np.full(n, np.iinfo(np.int32).max, np.int64)
    np.minimum.at(first, np.repeat(np.arange(n), counts)[is_max], idx[is_max])
    assert np.array_equal(first[has], a_idx[has]), "a row's first maximum is not the arg-max's choice"
    return int(has.sum())


def check_labels(label, join, n):
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    row_ptr, idx, _ = join
    n_comp, lab = connected_components(sp.csr_matrix((np.ones(len(idx), np.int8), idx, row_ptr), shape=(n, n)), directed=False)
    first = np.full(n_comp, n, np.int64)
    np.minimum.at(first, lab, np.arange(n))
    assert np.array_equal(label, first[lab].astype(np.int32)), "the labels are not the components of the self-join's CSR"
    return int(n_comp)


def measure(ctx, _lib, name, f, t, scorer, thresholds, self_forms, repeats):
    n_from, n_to = f.n, t.n
    arms = [("argmax", None)] + [("join", thr) for thr in thresholds]
    if self_forms:
        arms += [(kind, thr) for thr in thresholds for kind in ("self_join", "components")]
    totals, last = {}, {}

    def run(arm, counters=False):
        kind, thr = arm
        if kind == "argmax":
            return _lib.fuzz_extract_one(ctx, f, t, scorer)
        if kind == "join":
            return _lib.fuzz_join(ctx, f, t, scorer, thr * 100.0, capacity=totals.get(arm), counters=counters)
        if kind == "self_join":
            return _lib.fuzz_join(ctx, f, None, scorer, thr * 100.0, capacity=totals.get(arm), counters=counters)
        return _lib.fuzz_components(ctx, f, scorer, thr * 100.0, counters=counters)
    for arm in arms:                                  # warm-up: code objects, the pool's blocks, clocks; the exact totals
        for _ in range(2):
            last[arm] = run(arm)
            if arm[0].endswith("join"):
                totals[arm] = max(len(last[arm][1]), 1)
        print(f"[bench_fuzz_join] {name} {scorer} warmed {arm}", file=sys.stderr, flush=True)
    ctx.sync()
    ms = {arm: [] for arm in arms}
    for k in range(repeats):
        for arm in arms:
            ctx.event_record(0)
            run(arm)
            ctx.event_record(1)
            ctx.sync()
            ms[arm].append(ctx.event_elapsed_ms(0, 1))
        print(f"[bench_fuzz_join] {name} {scorer} round {k + 1} of {repeats}", file=sys.stderr, flush=True)
    res = {"shape": [n_from, n_to], "A_argmax": _stats(ms[arms[0]])}
    base = res["A_argmax"]["pass_ms_median"]
    letter = {"join": "B_join", "self_join": "C_self_join", "components": "D_components"}
    for arm in arms[1:]:
        kind, thr = arm
        r = _stats(ms[arm])
        r["over_A"] = r["pass_ms_median"] / base
        work = run(arm, counters=True)[-1]
        all_pairs = n_from * n_to if kind == "join" else n_from * (n_from - 1) // 2
        r.update({"counters": work, "bounded_share": work["bounded"] / all_pairs, "scored_share": work["scored"] / all_pairs})
        if kind == "join":
            r["hits"] = len(last[arm][1])
            r["rows_checked_against_A"] = check_maxima(last[arm], last[arms[0]], thr * 100.0)
        elif kind == "self_join":
            r["hits"] = len(last[arm][1])
        else:
            label, pairs, components = last[arm]
            assert pairs == len(last[("self_join", thr)][1])
            assert check_labels(label, last[("self_join", thr)], n_from) == components
            r.update({"hits": pairs, "components": components, "labels_checked_against_scipy": True})
        res[f"{letter[kind]}_t{thr}"] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--titles", type=int, default=20_000)
    ap.add_argument("--companies", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import polyfuzz_amd
    from polyfuzz_amd import _lib, datasets
    ctx = polyfuzz_amd.Context.default()
    res = {"commit": _commit(), "device": ctx.info()["name"], "repeats": args.repeats, "window_sweeps": "in the scoring lane",
           "entries": "host entries: a pass ends with the result in host memory; a join's capacity is the exact total", "data": {}}
    if args.titles > 0:
        fl, tl = datasets.c3_lists(args.titles)
        f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
        res["data"]["titles"] = {s: measure(ctx, _lib, "titles", f, t, s, thr, False, args.repeats) for s, thr in TITLE_ARMS.items()}
    if args.companies > 0:
        names = datasets.load_company_names()[:args.companies]
        f, t = _lib.DeviceStrings.upload(ctx, names), _lib.DeviceStrings.upload(ctx, names)
        res["data"]["companies"] = {s: measure(ctx, _lib, "companies", f, t, s, thr, True, args.repeats) for s, thr in COMPANY_ARMS.items()}
    print(json.dumps(res))
    out = args.out or os.path.join(REPO, "profiles", f"fuzz_join_{res['commit']}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
