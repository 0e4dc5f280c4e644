"""K14, the cosine threshold join and its components (pfz_dense_join, pfz_dense_components), beside the route they replace, on
clustered fp32 vectors, resident, in one process.

usage: python tools/bench_dense_join.py [--n 100000] [--dims 384,768] [--clusters 10000] [--repeats 5] [--out FILE] [--commit TEXT]

Data: gen(n, d, k, seed) of tests/dense_join_cases.py, restated here -- k cluster centres, every row a centre plus 0.45 x noise
(cosine within a cluster about 0.83 at these widths: at t = 0.8 nearly every pair of a cluster is a hit, at t = 0.9 nearly none).
Arms, per width and threshold (0.9, 0.8); every call leaves its result in host memory, device events around the call:
  A  the route before K14 to the same pairs: _lib.dense_topn of the list against a second handle of itself with ntop = the
     largest row count of the result (known from arm B: a caller would have to guess it) and lower_bound = the float32 just below
     the threshold, then the download of the n x ntop table.  The whole fp32 score panel is written and read back.
  B  _lib.dense_join in its two-list form on the same two handles: all T^2 tiles, no panel.  A's pairs and score bits == B's.
  C  _lib.dense_join, the self-join: T (T + 1) / 2 tiles, every unordered pair once.
  D  _lib.dense_components: C's tiles with every hit united on the device, n labels downloaded.  Beside it the host's way from
     C's CSR: scipy.sparse.csgraph.connected_components (wall clock); the labels are compared (==).
Capacities are the exact totals learned in the warm-up, so no timed call repeats itself.  Every arm is warmed twice, then the
arms are timed in turn over `repeats` rounds; medians with min and max.  One profiled pass per arm for the split (pfz_prof_*).
Prints one JSON object; --out also writes it (default: profiles/dense_join_<commit>.json).  Exit status 1 when A's pairs differ
from B's, D's pairs from C's total or D's labels from scipy's, in any case.  Run it under a time limit."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import numpy as np

from bench_components import labels_from_csr

THRESHOLDS = (0.9, 0.8)


def _commit():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "worktree"


def _stats(ms):
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)), "ms_all": [round(x, 4) for x in ms]}


def gen(n, d, k, seed, noise=0.45):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((k, d))
    lab = rng.integers(0, k, n)
    return (c[lab] + noise * rng.standard_normal((n, d))).astype(np.float32)


def _timed(ctx, fn):
    ctx.event_record(0)
    out = fn()
    ctx.event_record(1)
    ctx.sync()
    return ctx.event_elapsed_ms(0, 1), out


def _topn_pairs(idx, val):
    """(rows, cols, scores) of a top-n table, by row then column"""
    rows, slot = np.nonzero(idx >= 0)
    cols, vals = idx[rows, slot], val[rows, slot]
    order = np.lexsort((cols, rows))
    return rows[order], cols[order], vals[order]


def measure(ctx, _lib, n, d, k, repeats):
    x = gen(n, d, k, 14)
    f, g = _lib.DeviceDense.upload(ctx, x), _lib.DeviceDense.upload(ctx, x)
    del x
    out = {}
    for thr in THRESHOLDS:
        below = float(np.nextafter(_lib.dense_threshold32(thr), np.float32(-np.inf)))
        cap_b = cap_c = None
        for _ in range(2):                                   # warm-up: code objects, the pool's blocks, clocks; totals; equality
            b_ptr, b_idx, b_sim, b_counts = _lib.dense_join(ctx, f, g, thr, capacity=cap_b, counters=True)
            c_ptr, c_idx, c_sim, c_counts = _lib.dense_join(ctx, f, None, thr, capacity=cap_c, counters=True)
            cap_b, cap_c = max(len(b_idx), 1), max(len(c_idx), 1)
            ntop = max(int(np.diff(b_ptr).max()), 1)
            a_idx, a_val = _lib.dense_topn(ctx, f, g, ntop, below).download()
            label, pairs, components, d_counts = _lib.dense_components(ctx, f, thr, counters=True)
        a_rows, a_cols, a_vals = _topn_pairs(a_idx, a_val)
        b_rows = np.repeat(np.arange(n), np.diff(b_ptr))
        res = {"ntop_of_arm_a": ntop, "hits_two_lists": int(len(b_idx)), "hits_self_join": int(len(c_idx)),
               "a_pairs_equal_b": bool(np.array_equal(a_rows, b_rows) and np.array_equal(a_cols, b_idx)
                                       and a_vals.view(np.uint32).tobytes() == b_sim.view(np.uint32).tobytes()),
               "components": int(components), "largest_component": int(np.bincount(label).max()),
               "d_pairs_equal_c_total": bool(pairs == len(c_idx)),
               "labels_equal_scipy_on_c": bool(np.array_equal(labels_from_csr(n, c_ptr, c_idx), label)),
               "counters_b": b_counts, "counters_c": c_counts, "counters_d": d_counts}
        print(f"[bench_dense_join] {n} x {d} t={thr} warmed: {res}", file=sys.stderr, flush=True)
        arms = {
            "a": lambda: _lib.dense_topn(ctx, f, g, ntop, below).download(),
            "b": lambda: _lib.dense_join(ctx, f, g, thr, capacity=cap_b),
            "c": lambda: _lib.dense_join(ctx, f, None, thr, capacity=cap_c),
            "d": lambda: _lib.dense_components(ctx, f, thr),
        }
        ms = {arm: [] for arm in list(arms) + ["c_host_components"]}
        for r in range(repeats):
            for arm, fn in arms.items():
                t, got = _timed(ctx, fn)
                ms[arm].append(t)
                if arm == "c":
                    t0 = time.perf_counter()
                    labels_from_csr(n, got[0], got[1])
                    ms["c_host_components"].append((time.perf_counter() - t0) * 1e3)
            print(f"[bench_dense_join] {n} x {d} t={thr} round {r + 1} of {repeats}", file=sys.stderr, flush=True)
        prof = {}
        for arm, fn in arms.items():
            ctx.prof_enable(True)
            ctx.prof_reset()
            fn()
            ctx.sync()
            names = {"a": ("k5_gemm_panel", "k5_row_topn"), "b": ("k14_join", "k14_sort_unpack"), "c": ("k14_join", "k14_sort_unpack"),
                     "d": ("k14_components",)}[arm]
            prof[arm] = {k: ctx.prof_get(k)[0] for k in names}
            ctx.prof_enable(False)
        st = {arm: _stats(v) for arm, v in ms.items()}
        res.update({"arm_a_topn_panel": st["a"], "arm_b_join_two_lists": st["b"], "arm_c_self_join": st["c"],
                    "arm_d_components": st["d"], "host_components_of_c_csr": st["c_host_components"],
                    "b_over_a": st["b"]["ms_median"] / st["a"]["ms_median"], "c_over_b": st["c"]["ms_median"] / st["b"]["ms_median"],
                    "d_over_c": st["d"]["ms_median"] / st["c"]["ms_median"], "profiled_pass_ms": prof})
        out[f"t{thr}"] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--dims", default="384,768")
    ap.add_argument("--clusters", type=int, default=10_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="what to record as the measured commit (default: git's HEAD)")
    args = ap.parse_args()
    import polyfuzz_amd
    from polyfuzz_amd import _lib
    ctx = polyfuzz_amd.Context.default()
    res = {"commit": args.commit or _commit(), "device": ctx.info()["name"], "thresholds": list(THRESHOLDS), "n": args.n,
           "clusters": args.clusters, "repeats": args.repeats,
           "arms": "A: dense_topn (ntop = the largest row count, lower bound just below t) + download; B: dense_join, two handles of "
                   "the list; C: dense_join, self-join; D: dense_components; all with device events, results in host memory",
           "data": {}}
    for d in (int(v) for v in args.dims.split(",")):
        res["data"][f"{args.n}x{d}"] = measure(ctx, _lib, args.n, d, args.clusters, args.repeats)
    print(json.dumps(res))
    out = args.out or os.path.join(REPO, "profiles", f"dense_join_{res['commit']}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    # a timing of arms that do not agree is not a result: say so with the exit status (the JSON above shows which)
    broken = [f"{shape} {t}: {key}" for shape, per_t in res["data"].items() for t, e in per_t.items()
              for key in ("a_pairs_equal_b", "d_pairs_equal_c_total", "labels_equal_scipy_on_c") if not e[key]]
    if broken:
        print("[bench_dense_join] the arms disagree -- " + "; ".join(broken), file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
