"""K22, the cosine threshold join and its components searched on the 16-bit matrix cores and scored exactly (pfz_dense_join16,
pfz_dense_components16), beside K14 (pfz_dense_join, pfz_dense_components) on the same clustered fp32 vectors, resident, in one
process.

usage: python tools/bench_dense_join16.py [--n 100000] [--dims 768,384] [--clusters 10000] [--repeats 5] [--out FILE] [--commit TEXT]
                                          [--k14-only]

Data and method are tools/bench_dense_join.py's: gen(n, d, k, seed) -- k cluster centres, every row a centre plus 0.45 x noise --,
the lists resident, the arms timed in turn with device events over `repeats` rounds after two warm-up rounds, medians with min and
max, one profiled pass per arm for the split (pfz_prof_*).  Arms, per width and threshold (0.9, 0.8); every call leaves its result
in host memory:
  B  _lib.dense_join, two handles of the list (all T^2 tiles)      B16  _lib.dense_join16 on the same two lists, per search type
  C  _lib.dense_join, the self-join                                 C16  _lib.dense_join16, the self-join
  D  _lib.dense_components                                          D16  _lib.dense_components16
The search copies (DeviceDense.derive16) are made once, outside the timed calls, as the fp32 uploads are.  Capacities are the exact
totals learned in the warm-up and the candidate buffer has room for the candidates counted there, so no timed call repeats itself
or its search.  Per case and type it reports the candidates against the hits, the split search / rescore / sort-unpack, and the
number of pairs on which K22 and K14 differ: each is a pair whose score lies within float32 rounding of the threshold, one summed
by the fp32 matrix core and one in float64 -- reported, not asserted.  --k14-only times B, C and D alone (a build without K22: the
parent's library through POLYFUZZ_HIP_LIB).
Prints one JSON object; --out also writes it (default: profiles/dense_join16_<commit>.json).  Exit status 1 when D16's labels are
not the components of C16's pairs.  Run it under a time limit."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import numpy as np

from bench_components import labels_from_csr
from bench_dense_join import THRESHOLDS, _commit, _stats, _timed, gen

TYPES = ("bfloat16", "float16")


def _keys(row_ptr, idx):
    return np.repeat(np.arange(len(row_ptr) - 1, dtype=np.int64), np.diff(row_ptr)) << 32 | idx.astype(np.int64)


def measure(ctx, _lib, n, d, k, repeats, k14_only):
    x = gen(n, d, k, 14)
    f, g = _lib.DeviceDense.upload(ctx, x), _lib.DeviceDense.upload(ctx, x)
    del x
    copies = {} if k14_only else {t: (f.derive16(t), g.derive16(t)) for t in TYPES}
    out = {}
    for thr in THRESHOLDS:
        arms, res, cap = {}, {}, {}
        for _ in range(2):                                   # warm-up: code objects, the pool's blocks, clocks; totals
            b = _lib.dense_join(ctx, f, g, thr, capacity=cap.get("b"))
            c = _lib.dense_join(ctx, f, None, thr, capacity=cap.get("c"))
            _lib.dense_components(ctx, f, thr)
            cap["b"], cap["c"] = max(len(b[1]), 1), max(len(c[1]), 1)
            for t, (f16, g16) in copies.items():
                b16 = _lib.dense_join16(ctx, f16, g16, f, g, thr, capacity=cap.get(("b", t)), counters=True, cand_capacity=cap.get(("bc", t)))
                c16 = _lib.dense_join16(ctx, f16, None, f, None, thr, capacity=cap.get(("c", t)), counters=True, cand_capacity=cap.get(("cc", t)))
                label, pairs, components, d_counts = _lib.dense_components16(ctx, f16, f, thr, counters=True, cand_capacity=cap.get(("cc", t)))
                cap["b", t], cap["c", t] = max(len(b16[1]), 1), max(len(c16[1]), 1)
                cap["bc", t], cap["cc", t] = max(b16[3]["candidates"], 1), max(c16[3]["candidates"], 1)
                res[t] = {"hits_two_lists": len(b16[1]), "candidates_two_lists": b16[3]["candidates"], "hits_self_join": len(c16[1]),
                          "candidates_self_join": c16[3]["candidates"], "counters_two_lists": b16[3], "counters_self_join": c16[3],
                          "components": int(components),
                          "pairs_differing_from_k14_two_lists": int(len(np.setxor1d(_keys(b16[0], b16[1]), _keys(b[0], b[1])))),
                          "pairs_differing_from_k14_self_join": int(len(np.setxor1d(_keys(c16[0], c16[1]), _keys(c[0], c[1])))),
                          "labels_are_components_of_c16": bool(np.array_equal(labels_from_csr(n, c16[0], c16[1]), label) and pairs == len(c16[1]))}
        res["k14"] = {"hits_two_lists": len(b[1]), "hits_self_join": len(c[1])}
        print(f"[bench_dense_join16] {n} x {d} t={thr} warmed: {res}", file=sys.stderr, flush=True)
        arms["k14_b"] = lambda: _lib.dense_join(ctx, f, g, thr, capacity=cap["b"])
        arms["k14_c"] = lambda: _lib.dense_join(ctx, f, None, thr, capacity=cap["c"])
        arms["k14_d"] = lambda: _lib.dense_components(ctx, f, thr)
        for t, (f16, g16) in copies.items():
            arms[f"{t}_b"] = lambda t=t, f16=f16, g16=g16: _lib.dense_join16(ctx, f16, g16, f, g, thr, capacity=cap["b", t], cand_capacity=cap["bc", t])
            arms[f"{t}_c"] = lambda t=t, f16=f16: _lib.dense_join16(ctx, f16, None, f, None, thr, capacity=cap["c", t], cand_capacity=cap["cc", t])
            arms[f"{t}_d"] = lambda t=t, f16=f16: _lib.dense_components16(ctx, f16, f, thr, cand_capacity=cap["cc", t])
        ms = {arm: [] for arm in arms}
        for r in range(repeats):
            for arm, fn in arms.items():
                ms[arm].append(_timed(ctx, fn)[0])
            print(f"[bench_dense_join16] {n} x {d} t={thr} round {r + 1} of {repeats}", file=sys.stderr, flush=True)
        prof = {}
        for arm, fn in arms.items():
            ctx.prof_enable(True)
            ctx.prof_reset()
            fn()
            ctx.sync()
            names = ("k14_join", "k14_sort_unpack", "k14_components") if arm.startswith("k14") else ("k22_search", "k22_rescore", "k22_sort_unpack")
            prof[arm] = {k: ctx.prof_get(k)[0] for k in names}
            ctx.prof_enable(False)
        res["ms"] = {arm: _stats(v) for arm, v in ms.items()}
        res["profiled_pass_ms"] = prof
        for t in copies:
            for arm in "bcd":
                res[t][f"{arm}_over_k14"] = res["ms"][f"{t}_{arm}"]["ms_median"] / res["ms"][f"k14_{arm}"]["ms_median"]
        out[f"t{thr}"] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--dims", default="768,384")
    ap.add_argument("--clusters", type=int, default=10_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="what to record as the measured commit (default: git's HEAD)")
    ap.add_argument("--k14-only", action="store_true")
    args = ap.parse_args()
    import polyfuzz_amd
    from polyfuzz_amd import _lib
    ctx = polyfuzz_amd.Context.default()
    res = {"commit": args.commit or _commit(), "device": ctx.info()["name"], "library": os.path.relpath(_lib.lib_path(), REPO), "thresholds": list(THRESHOLDS),
           "n": args.n, "clusters": args.clusters, "repeats": args.repeats,
           "arms": "k14_b / _c / _d: dense_join two lists, self-join, dense_components; <type>_b / _c / _d: dense_join16 two lists, "
                   "self-join, dense_components16; device events, results in host memory, search copies resident",
           "data": {}}
    for d in (int(v) for v in args.dims.split(",")):
        res["data"][f"{args.n}x{d}"] = measure(ctx, _lib, args.n, d, args.clusters, args.repeats, args.k14_only)
    print(json.dumps(res))
    out = args.out or os.path.join(REPO, "profiles", f"dense_join16_{res['commit']}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    broken = [f"{shape} {t} {ty}" for shape, per_t in res["data"].items() for t, e in per_t.items() for ty in TYPES
              if ty in e and not e[ty]["labels_are_components_of_c16"]]
    if broken:
        print("[bench_dense_join16] the components are not those of the join's pairs -- " + "; ".join(broken), file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
