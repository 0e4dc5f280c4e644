"""K12, the connected components of "Levenshtein / OSA similarity >= t" (pfz_lev_components), beside the route it replaces, on the two
lists the package is measured on, resident, in one process:

  titles     the 20 000 IMDB titles of BASELINE configuration 3 (its to-list), against themselves;
  companies  the 100 000 company names, against themselves.

usage: python tools/bench_components.py [--titles 20000] [--companies 100000] [--repeats 9] [--company-repeats 5] [--out FILE]
       [--commit TEXT]

Arms, per list, scorer and threshold (0.9, 0.8, 0.6):
  A  the route before K12: _lib.lev_join, self-join, capacity set to the exact total (learned in the warm-up, so no timed call
     repeats itself) -- the walk, the sort of the hits, the CSR and its download: the DEVICE part, timed with device events around
     the call --, then a union-find over the CSR on the host (scipy.sparse.csgraph.connected_components, compiled code, and the
     relabelling to the smallest position): the HOST part, timed with the wall clock.
  B  _lib.lev_components: the same walk with every hit united on the device, the forest flattened, n labels downloaded; device
     events around the call.
Every arm is warmed twice, then the arms are timed in turn over `repeats` rounds; medians with min and max.  The labels of the
two arms are compared (==) in the warm-up.  Reported besides: hits, components, the largest component; the device bytes a call
allocates, COMPUTED from the buffers the two entries allocate (the pool keeps no high-water mark; the plan of the list, which
both share, and the general kernel's columns, equal in both, are left out): A is O(hits), B is O(n); one profiled pass per arm
for the split (pfz_prof_*): k11_join / k11_sort_unpack, the rest of A's device part being the download, and k12_walk /
k12_flatten.
Prints one JSON object; --out also writes it (default: profiles/components_<commit>.json).  Run it under a time limit."""
import argparse
import json
import os
import subprocess
import sys
import time

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
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)), "ms_all": [round(x, 4) for x in ms]}


def labels_from_csr(n, row_ptr, idx):
    """label[i] = the smallest position of i's component of the graph whose edges are the CSR's pairs"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    graph = csr_matrix((np.ones(len(idx), np.int8), idx, row_ptr), shape=(n, n))
    _, comp = connected_components(graph, directed=False)
    _, first = np.unique(comp, return_index=True)             # (positions ascend: the first of a component is its smallest)
    return first[comp].astype(np.int32)


def _pow2_at_least(x, floor=1024):
    p = floor
    while p < x:
        p <<= 1
    return p


def measure(ctx, _lib, name, dev, n, repeats):
    out = {"n": n, "scorers": {}}
    for scorer in SCORERS:
        res = {}
        totals = {}
        for thr in THRESHOLDS:                                 # warm-up: code objects, the pool's blocks, clocks; totals; equality
            for _ in range(2):
                row_ptr, idx, _, _ = _lib.lev_join(ctx, dev, None, scorer, thr, capacity=totals.get(thr))
                totals[thr] = max(len(idx), 1)
                label, pairs, components = _lib.lev_components(ctx, dev, scorer, thr)
            host = labels_from_csr(n, row_ptr, idx)
            res[thr] = {"hits": int(pairs), "hits_equal_k11_total": bool(pairs == len(idx)), "components": int(components),
                        "largest_component": int(np.bincount(label).max()), "labels_equal": bool(np.array_equal(host, label))}
            print(f"[bench_components] {name} {scorer} t={thr} warmed: {res[thr]}", file=sys.stderr, flush=True)
        ctx.sync()
        ms = {(arm, thr): [] for arm in ("a_device", "a_host", "b") for thr in THRESHOLDS}
        for k in range(repeats):
            for thr in THRESHOLDS:
                ctx.event_record(0)
                row_ptr, idx, _, _ = _lib.lev_join(ctx, dev, None, scorer, thr, capacity=totals[thr])
                ctx.event_record(1)
                ctx.sync()
                ms["a_device", thr].append(ctx.event_elapsed_ms(0, 1))
                t0 = time.perf_counter()
                labels_from_csr(n, row_ptr, idx)
                ms["a_host", thr].append((time.perf_counter() - t0) * 1e3)
                ctx.event_record(0)
                _lib.lev_components(ctx, dev, scorer, thr)
                ctx.event_record(1)
                ctx.sync()
                ms["b", thr].append(ctx.event_elapsed_ms(0, 1))
            print(f"[bench_components] {name} {scorer} round {k + 1} of {repeats}", file=sys.stderr, flush=True)
        for thr in THRESHOLDS:
            hits = res[thr]["hits"]
            ctx.prof_enable(True)
            ctx.prof_reset()
            _lib.lev_join(ctx, dev, None, scorer, thr, capacity=totals[thr])
            _lib.lev_components(ctx, dev, scorer, thr)
            ctx.sync()
            prof = {k: ctx.prof_get(k)[0] for k in ("k11_join", "k11_sort_unpack", "k12_walk", "k12_flatten")}
            ctx.prof_enable(False)
            a_dev, a_host, b = _stats(ms["a_device", thr]), _stats(ms["a_host", thr]), _stats(ms["b", thr])
            res[thr].update({
                "arm_a_join_device": a_dev, "arm_a_union_find_host": a_host, "arm_b_components": b,
                "b_over_a_device": b["ms_median"] / a_dev["ms_median"],
                "b_over_a_whole": b["ms_median"] / (a_dev["ms_median"] + a_host["ms_median"]),
                "profiled_pass_ms": prof,
                # keys + sorted keys + row_ptr + (idx, dist, sim) + the rows of the launches | rows + parent + label
                "arm_a_call_device_bytes_computed": 8 * totals[thr] + 8 * _pow2_at_least(hits) + 8 * (n + 1) + 16 * hits + 4 * n,
                "arm_b_call_device_bytes_computed": 12 * n})
        out["scorers"][scorer] = {f"t{thr}": res[thr] for thr in THRESHOLDS}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--titles", type=int, default=20_000)
    ap.add_argument("--companies", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--company-repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="what to record as the measured commit (default: git's HEAD)")
    args = ap.parse_args()
    import polyfuzz_amd
    from polyfuzz_amd import _lib, datasets
    ctx = polyfuzz_amd.Context.default()
    res = {"commit": args.commit or _commit(), "device": ctx.info()["name"], "thresholds": list(THRESHOLDS),
           "arms": "A: lev_join self-join (device events, result in host memory) then scipy connected_components on the CSR (wall clock); "
                   "B: lev_components (device events, labels in host memory)",
           "repeats": {"titles": args.repeats, "companies": args.company_repeats}, "data": {}}
    if args.titles > 0:
        titles = datasets.c3_lists(args.titles)[1]
        res["data"]["titles"] = measure(ctx, _lib, "titles", _lib.DeviceStrings.upload(ctx, titles), len(titles), args.repeats)
    if args.companies > 0:
        names = datasets.load_company_names()[:args.companies]
        res["data"]["companies"] = measure(ctx, _lib, "companies", _lib.DeviceStrings.upload(ctx, names), len(names), args.company_repeats)
    print(json.dumps(res))
    out = args.out or os.path.join(REPO, "profiles", f"components_{res['commit']}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
