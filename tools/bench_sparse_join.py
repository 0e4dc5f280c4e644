"""K15, the sparse-cosine threshold join and its components (pfz_cossim_join, pfz_cossim_components), beside the route they
replace, on the shipped company names, resident, in one process.

usage: python tools/bench_sparse_join.py [--repeats 5] [--out FILE] [--commit TEXT] [--only self100k|c2]

Data: "self100k", the 100 000 company names against themselves, and "c2", the 10 000 x 10 000 lists of config 2
(datasets.c2_lists); fitted and vectorised as TFIDF.match does.  Thresholds 0.9, 0.8, 0.6.
Arms, per data set and threshold; every call leaves its result in host memory, device events around the call:
  A  the route before K15 to the same pairs: _lib.cossim_topn with lower_bound = t - 1e-6 and ntop = the fullest row's count
     (known from arm B plus a margin of 8: a caller would have to guess it), then the download of the n x ntop table; the host
     keeps float64(score) >= t.  Not run where the table would exceed 2^26 cells (recorded as skipped, with the ntop it needs).
  B  _lib.sparse_join in its two-list form (self100k: on a second handle of the list).  A's pairs and score bits == B's.
  C  (self100k) _lib.sparse_join, the self-join: every unordered pair once.
  D  (self100k) _lib.sparse_components: C's walk with every hit united on the device, n labels downloaded; the labels are compared
     (==) with the host's union of C's CSR (scipy.sparse.csgraph.connected_components).
Capacities are the exact totals learned in the warm-up, so no timed call repeats itself.  Every arm is warmed twice, then the
arms are timed in turn over `repeats` rounds; medians with min and max; the counters of B, C and D beside them.  One profiled
pass per arm for the split (pfz_prof_*).  A second run with POLYFUZZ_HIP_LIB on a -DPFZ_K15_NO_BOUND build
(tools/build_variant.sh) and another --out gives the block bound's worth.
Prints one JSON object; --out also writes it (default: profiles/sparse_join_<commit>.json).  Exit status 1 when A's pairs differ
from B's, D's pairs from C's total or D's labels from the host's, in any case.  Run it under a time limit."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import numpy as np

from bench_components import labels_from_csr

THRESHOLDS = (0.9, 0.8, 0.6)
MAX_TABLE_CELLS = 1 << 26


def _commit():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "worktree"


def _stats(ms):
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)), "ms_all": [round(x, 4) for x in ms]}


def _timed(ctx, fn):
    ctx.event_record(0)
    out = fn()
    ctx.event_record(1)
    ctx.sync()
    return ctx.event_elapsed_ms(0, 1), out


def _table_pairs(idx, val, t):
    """(rows, cols, scores) of a top-n table's entries with float64(score) >= t, by row then column; None: a row is full of them"""
    passes = (idx >= 0) & (val.astype(np.float64) >= t)
    if passes[:, -1].any():
        return None
    rows, slot = np.nonzero(passes)
    cols, vals = idx[rows, slot], val[rows, slot]
    order = np.lexsort((cols, rows))
    return rows[order], cols[order], vals[order]


def measure(ctx, _lib, name, from_dev, index, self_dev, repeats):
    """from_dev against index in the two-list form; self_dev: the matrix the index was built from (arms C and D), or None"""
    n = from_dev.n_rows
    out = {}
    for thr in THRESHOLDS:
        cap_b = cap_c = None
        res = {}
        for _ in range(2):                                   # warm-up: code objects, the pool's blocks, clocks; totals; equality
            b_ptr, b_idx, b_sim, b_counts = _lib.sparse_join(ctx, index, from_dev, thr, capacity=cap_b, counters=True)
            cap_b = max(len(b_idx), 1)
            ntop = int(np.diff(b_ptr).max()) + 8
            run_a = n * ntop <= MAX_TABLE_CELLS
            if run_a:
                a_idx, a_val = _lib.cossim_topn(ctx, index, from_dev, ntop, thr - 1e-6).download()
            if self_dev is not None:
                c_ptr, c_idx, c_sim, c_counts = _lib.sparse_join(ctx, index, self_dev, thr, self_join=True, capacity=cap_c, counters=True)
                cap_c = max(len(c_idx), 1)
                label, pairs, components, d_counts = _lib.sparse_components(ctx, index, self_dev, thr, counters=True)
        res.update({"ntop_of_arm_a": ntop, "hits_two_lists": int(len(b_idx)), "fullest_row": ntop - 8, "rows_with_a_hit": int((np.diff(b_ptr) > 0).sum()),
                    "counters_b": b_counts})
        if run_a:
            a = _table_pairs(a_idx, a_val, thr)
            b_rows = np.repeat(np.arange(n), np.diff(b_ptr))
            res["a_pairs_equal_b"] = bool(a is not None and np.array_equal(a[0], b_rows) and np.array_equal(a[1], b_idx)
                                          and a[2].view(np.uint32).tobytes() == b_sim.view(np.uint32).tobytes())
            del a, a_idx, a_val
        else:
            res["a_pairs_equal_b"] = None
            res["arm_a_skipped"] = f"a table of {n} x {ntop} cells exceeds {MAX_TABLE_CELLS}"
        if self_dev is not None:
            res.update({"hits_self_join": int(len(c_idx)), "components": int(components), "largest_component": int(np.bincount(label).max()),
                        "d_pairs_equal_c_total": bool(pairs == len(c_idx)),
                        "labels_equal_host_on_c": bool(np.array_equal(labels_from_csr(n, c_ptr, c_idx), label)),
                        "counters_c": c_counts, "counters_d": d_counts})
        print(f"[bench_sparse_join] {name} t={thr} warmed: {res}", file=sys.stderr, flush=True)
        arms = {"b": lambda: _lib.sparse_join(ctx, index, from_dev, thr, capacity=cap_b)}
        scopes = {"a": ("k3_cossim_topn",), "b": ("k15_join", "k15_sort_unpack"), "c": ("k15_join", "k15_sort_unpack"), "d": ("k15_components",)}
        if run_a:
            arms["a"] = lambda: _lib.cossim_topn(ctx, index, from_dev, ntop, thr - 1e-6).download()
        if self_dev is not None:
            arms["c"] = lambda: _lib.sparse_join(ctx, index, self_dev, thr, self_join=True, capacity=cap_c)
            arms["d"] = lambda: _lib.sparse_components(ctx, index, self_dev, thr)
        ms = {arm: [] for arm in arms}
        for r in range(repeats):
            for arm, fn in arms.items():
                ms[arm].append(_timed(ctx, fn)[0])
        prof = {}
        for arm, fn in arms.items():
            ctx.prof_enable(True)
            ctx.prof_reset()
            fn()
            ctx.sync()
            prof[arm] = {k: ctx.prof_get(k)[0] for k in scopes[arm]}
            ctx.prof_enable(False)
        st = {arm: _stats(v) for arm, v in ms.items()}
        labels = {"a": "arm_a_topn_table", "b": "arm_b_join_two_lists", "c": "arm_c_self_join", "d": "arm_d_components"}
        res.update({labels[arm]: st[arm] for arm in st})
        if run_a:
            res["b_over_a"] = st["b"]["ms_median"] / st["a"]["ms_median"]
        if self_dev is not None:
            res["c_over_b"] = st["c"]["ms_median"] / st["b"]["ms_median"]
            res["d_over_c"] = st["d"]["ms_median"] / st["c"]["ms_median"]
        res["profiled_pass_ms"] = prof
        print(f"[bench_sparse_join] {name} t={thr} timed: " + ", ".join(f"{a} {st[a]['ms_median']:.3f} ms" for a in sorted(st)),
              file=sys.stderr, flush=True)
        out[f"t{thr}"] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="what to record as the measured commit (default: git's HEAD)")
    ap.add_argument("--only", default=None, choices=("self100k", "c2"))
    args = ap.parse_args()
    import polyfuzz_amd
    from polyfuzz_amd import _lib, datasets
    from polyfuzz_amd.models import TFIDF
    ctx = polyfuzz_amd.Context.default()
    res = {"commit": args.commit or _commit(), "device": ctx.info()["name"], "library": os.path.basename(_lib.lib_path()),
           "thresholds": list(THRESHOLDS), "repeats": args.repeats,
           "arms": "A: cossim_topn (ntop = the fullest row's count + 8, lower bound t - 1e-6) + download; B: sparse_join, two handles; "
                   "C: sparse_join, self-join; D: sparse_components; all with device events, results in host memory",
           "data": {}}
    if args.only in (None, "self100k"):
        names = datasets.load_company_names()
        m = TFIDF()
        dev, _ = m._extract_tf_idf(names, None, True)
        other = m._dev_vec.transform(m._upload(names))
        res["data"]["self100k"] = dict(index=m._dev_index.info(), **measure(ctx, _lib, "self100k", other, m._dev_index, dev, args.repeats))
        del m, dev, other
    if args.only in (None, "c2"):
        frm, to = datasets.c2_lists()
        m = TFIDF()
        dev, _ = m._extract_tf_idf(frm, to, True)
        res["data"]["c2"] = dict(index=m._dev_index.info(), **measure(ctx, _lib, "c2", dev, m._dev_index, None, args.repeats))
    print(json.dumps(res))
    out = args.out or os.path.join(REPO, "profiles", f"sparse_join_{res['commit']}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    # a timing of arms that do not agree is not a result: say so with the exit status (the JSON above shows which)
    broken = [f"{name} {t}: {key}" for name, per_t in res["data"].items() for t, e in per_t.items() if t != "index"
              for key in ("a_pairs_equal_b", "d_pairs_equal_c_total", "labels_equal_host_on_c") if e.get(key) is False]
    if broken:
        print("[bench_sparse_join] the arms disagree -- " + "; ".join(broken), file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
