"""K23, the Hamming threshold join and its components (pfz_hamming_join, pfz_hamming_components), beside the route they replace, on
clustered packed binary codes, resident, in one process.

usage: python tools/bench_hamming_join.py [--n 100000] [--dims 768,64] [--clusters 10000] [--repeats 5] [--out FILE] [--commit TEXT]

Data: gen(n, d, k, seed) of tests/hamming_join_cases.py, restated here -- k random base codes, every row a base code with each bit
flipped with probability 0.05 (two rows of a cluster differ in about 0.095 d bits: 73 of 768, 6 of 64; two rows of different
clusters in about d / 2).  Cutoffs: min_similarity 0.9 and 0.8 turned into distances by _lib.hamming_max_distance, and at 64 bits
also max_distance = 3, the SimHash rule.  Arms, per width and cutoff; every call leaves its result in host memory, device events
around the call:
  A  the route before K23 to the same pairs: _lib.dense_topn of the list against a second bit handle of itself with ntop = the
     largest row count of the result (known from arm B: a caller would have to guess it) and lower_bound = the float32 just below
     the cutoff's score, then the download of the n x ntop table.  The whole fp32 score panel is written and read back.
  B  _lib.hamming_join in its two-list form on the same two handles: all T^2 tiles, no panel.  A's pairs and score bits == B's.
  C  _lib.hamming_join, the self-join: T (T + 1) / 2 tiles, every unordered pair once.
  D  _lib.hamming_components: C's tiles with every hit united on the device, n labels downloaded.  Beside it the host's way from
     C's CSR: scipy.sparse.csgraph.connected_components (wall clock); the labels are compared (==).
Capacities are the exact totals learned in the warm-up, so no timed call repeats itself.  Every arm is warmed twice, then the
arms are timed in turn over `repeats` rounds; medians with min and max.  One profiled pass per arm for the split (pfz_prof_*).
Prints one JSON object; --out also writes it (default: profiles/hamming_join_<commit>.json).  Exit status 1 when A's pairs differ
from B's, D's pairs from C's total or D's labels from scipy's, in any case.  Run it under a time limit."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import numpy as np

from bench_components import labels_from_csr
from bench_dense_join import _commit, _stats, _timed, _topn_pairs

SIMILARITIES = (0.9, 0.8)
SIMHASH = (64, 3)            # at this width also max_distance = 3


def gen(n, d, k, seed, flip=0.05):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 2, (k, d), dtype=np.uint8)
    lab = rng.integers(0, k, n)
    return np.packbits(base[lab] ^ (rng.random((n, d)) < flip), axis=1)


def measure(ctx, _lib, n, d, k, repeats):
    x = gen(n, d, k, 23)
    f, g = _lib.DeviceDense.upload_bits(ctx, x), _lib.DeviceDense.upload_bits(ctx, x)
    del x
    cutoffs = [(f"t{t}", _lib.hamming_max_distance(d, t)) for t in SIMILARITIES] + ([(f"h{SIMHASH[1]}", SIMHASH[1])] if d == SIMHASH[0] else [])
    out = {}
    for tag, hmax in cutoffs:
        below = float(np.nextafter(_lib.hamming_similarity(np.array([hmax]), d)[0], np.float32(-np.inf)))
        cap_b = cap_c = None
        for _ in range(2):                                   # warm-up: code objects, the pool's blocks, clocks; totals; equality
            b_ptr, b_idx, b_dist, b_counts = _lib.hamming_join(ctx, f, g, hmax, capacity=cap_b, counters=True)
            c_ptr, c_idx, c_dist, c_counts = _lib.hamming_join(ctx, f, None, hmax, capacity=cap_c, counters=True)
            cap_b, cap_c = max(len(b_idx), 1), max(len(c_idx), 1)
            ntop = max(int(np.diff(b_ptr).max()), 1)
            a_idx, a_val = _lib.dense_topn(ctx, f, g, ntop, below).download()
            label, pairs, components, d_counts = _lib.hamming_components(ctx, f, hmax, counters=True)
        a_rows, a_cols, a_vals = _topn_pairs(a_idx, a_val)
        b_rows = np.repeat(np.arange(n), np.diff(b_ptr))
        res = {"max_distance": int(hmax), "ntop_of_arm_a": ntop, "hits_two_lists": int(len(b_idx)), "hits_self_join": int(len(c_idx)),
               "a_pairs_equal_b": bool(np.array_equal(a_rows, b_rows) and np.array_equal(a_cols, b_idx)
                                       and a_vals.tobytes() == _lib.hamming_similarity(b_dist, d).tobytes()),
               "components": int(components), "largest_component": int(np.bincount(label).max()),
               "d_pairs_equal_c_total": bool(pairs == len(c_idx)),
               "labels_equal_scipy_on_c": bool(np.array_equal(labels_from_csr(n, c_ptr, c_idx), label)),
               "counters_b": b_counts, "counters_c": c_counts, "counters_d": d_counts}
        print(f"[bench_hamming_join] {n} x {d} {tag} warmed: {res}", file=sys.stderr, flush=True)
        arms = {
            "a": lambda: _lib.dense_topn(ctx, f, g, ntop, below).download(),
            "b": lambda: _lib.hamming_join(ctx, f, g, hmax, capacity=cap_b),
            "c": lambda: _lib.hamming_join(ctx, f, None, hmax, capacity=cap_c),
            "d": lambda: _lib.hamming_components(ctx, f, hmax),
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
            print(f"[bench_hamming_join] {n} x {d} {tag} round {r + 1} of {repeats}", file=sys.stderr, flush=True)
        prof = {}
        for arm, fn in arms.items():
            ctx.prof_enable(True)
            ctx.prof_reset()
            fn()
            ctx.sync()
            names = {"a": ("k5_gemm_panel", "k5_row_topn"), "b": ("k23_join", "k23_sort_unpack"), "c": ("k23_join", "k23_sort_unpack"),
                     "d": ("k23_components",)}[arm]
            prof[arm] = {k: ctx.prof_get(k)[0] for k in names}
            ctx.prof_enable(False)
        st = {arm: _stats(v) for arm, v in ms.items()}
        pairs_b = float(n) * n
        res.update({"arm_a_topn_panel": st["a"], "arm_b_join_two_lists": st["b"], "arm_c_self_join": st["c"],
                    "arm_d_components": st["d"], "host_components_of_c_csr": st["c_host_components"],
                    "b_over_a": st["b"]["ms_median"] / st["a"]["ms_median"], "c_over_b": st["c"]["ms_median"] / st["b"]["ms_median"],
                    "d_over_c": st["d"]["ms_median"] / st["c"]["ms_median"], "profiled_pass_ms": prof,
                    # the tile kernels alone, per 2.05e9 pairs: the unit of k5_hamming_panel's own step in DESIGN.md section 4
                    "k23_join_ms_per_2.05e9_pairs": prof["b"]["k23_join"] / pairs_b * 2.05e9,
                    "k5_gemm_panel_ms_per_2.05e9_pairs": prof["a"]["k5_gemm_panel"] / pairs_b * 2.05e9})
        out[tag] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--dims", default="768,64")
    ap.add_argument("--clusters", type=int, default=10_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="what to record as the measured commit (default: git's HEAD)")
    args = ap.parse_args()
    import polyfuzz_amd
    from polyfuzz_amd import _lib
    ctx = polyfuzz_amd.Context.default()
    res = {"commit": args.commit or _commit(), "device": ctx.info()["name"], "similarities": list(SIMILARITIES), "n": args.n,
           "clusters": args.clusters, "repeats": args.repeats,
           "arms": "A: dense_topn on two bit handles (ntop = the largest row count, lower bound just below the cutoff's score) + "
                   "download; B: hamming_join, two handles of the list; C: hamming_join, self-join; D: hamming_components; all with "
                   "device events, results in host memory",
           "data": {}}
    for d in (int(v) for v in args.dims.split(",")):
        res["data"][f"{args.n}x{d}"] = measure(ctx, _lib, args.n, d, args.clusters, args.repeats)
    print(json.dumps(res))
    out = args.out or os.path.join(REPO, "profiles", f"hamming_join_{res['commit']}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    # a timing of arms that do not agree is not a result: say so with the exit status (the JSON above shows which)
    broken = [f"{shape} {t}: {key}" for shape, per_t in res["data"].items() for t, e in per_t.items()
              for key in ("a_pairs_equal_b", "d_pairs_equal_c_total", "labels_equal_scipy_on_c") if not e[key]]
    if broken:
        print("[bench_hamming_join] the arms disagree -- " + "; ".join(broken), file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
