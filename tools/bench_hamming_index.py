"""K24, the block index behind Hamming.join / .components (pfz_hamming_join_indexed, pfz_hamming_components_indexed), beside K23's tile
program (pfz_hamming_join, pfz_hamming_components) on the same resident handles, in one process.

usage: python tools/bench_hamming_index.py [--arm sweep|scale] [--n 100000] [--dims 64,256,768] [--scale-n 100000,1000000]
                                           [--k23-max-n 1000000] [--repeats 3] [--skip-factor 4] [--out FILE] [--commit TEXT]

Data, two generators:
  clustered  gen(n, d, k, seed) of tests/hamming_join_cases.py restated -- n / 10 random base codes, every row a base code with each
             bit flipped with probability 0.05
  uniform    random codes; the last quarter of the rows are near-copies of earlier rows with 0 .. 5 flipped bits (the draws of the
             4 096-row list of tests/hamming_index_cases.py)
Arm `sweep` (what yields the constant R, kK24AutoRatio of csrc/k24_core.h): the self-join of n codes, at 64 bits for
max_distance = 0 .. 12, at the other widths for min_similarity 0.95, 0.9, 0.8, 0.7, 0.6 turned into distances.  Per point: K23's
call and the forced-blocks call, whole calls with their sorts and the download, device events, medians over `repeats` rounds after
two warm-up calls with the capacity learned there; rho = (index ms / checks) / (K23 ms / all pairs).  A point whose checks exceed
skip-factor x all pairs is not timed on the index (auto would never choose it; the call may take minutes) and says so.  One
profiled pass of the index call gives its split: keys, sort, ranges (searches and scan), probe, sort_unpack.
Arm `scale`: uniform 64-bit codes at max_distance 3, self-join and components, for every n of --scale-n; K23 beside it up to
--k23-max-n, "not run" beyond.
Row pointers, indices and distances are compared == between the two routes, labels and counts too; exit status 1 on any difference.
Prints one JSON object; --out also writes it (default: profiles/hamming_index_<commit>.json).  Run it under a time limit."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import numpy as np

from bench_dense_join import _commit, _stats, _timed

SIMILARITIES = (0.95, 0.9, 0.8, 0.7, 0.6)
SCOPES = ("k24_keys", "k24_sort", "k24_ranges", "k24_probe", "k24_sort_unpack")


def clustered(n, d, seed=24, flip=0.05):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 2, (max(n // 10, 1), d), dtype=np.uint8)
    out = np.empty((n, d // 8), np.uint8)
    for lo in range(0, n, 20000):                      # in slabs: the flips of 100 000 x 768 bits as float64 are 600 MB
        hi = min(lo + 20000, n)
        lab = rng.integers(0, len(base), hi - lo)
        out[lo:hi] = np.packbits(base[lab] ^ (rng.random((hi - lo, d)) < flip), axis=1)
    return out


def uniform(n, d, seed=24):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (n, d // 8), dtype=np.uint8)
    q = n // 4
    src = rng.integers(0, n - q, q)
    flips = rng.integers(0, 6, q)
    x[n - q:] = x[src]
    for k in range(5):                                 # flip k + 1 of 5 drawn bit positions (a repeat flips back: still a near-copy)
        at = rng.integers(0, d, q)
        rows = np.nonzero(flips > k)[0]
        x[n - q + rows, at[rows] // 8] ^= (128 >> (at[rows] % 8)).astype(np.uint8)
    return x


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a[:3], b[:3]))


def point(ctx, _lib, dev, n, hmax, repeats, skip_factor, with_k23=True, with_components=False):
    """one (list, distance): both routes of the self-join, equal results, medians, rho, the split"""
    all_pairs = n * (n - 1) // 2
    res = {"max_distance": int(hmax), "all_pairs": all_pairs}
    try:
        plan = _lib.hamming_index_plan(dev.dim, hmax)
    except _lib.PfzUnsupported as e:
        res["index"] = f"not indexable: {e}"
        return res, True
    res["blocks"], res["ratio_in_library"] = plan["blocks"], plan["ratio"]
    # `checks` first, from a call that never probes when they are many: auto
    auto = _lib.hamming_join_indexed(ctx, dev, None, hmax, auto=True, counters=True)
    checks, cap = auto[3]["checks"], max(auto[3]["pairs"], 1)
    res.update({"checks": checks, "hits": auto[3]["pairs"], "checks_over_all": checks / all_pairs, "auto_route": auto[3]["route"]})
    ok = True
    arms = {}
    if with_k23:
        base = _lib.hamming_join(ctx, dev, None, hmax, capacity=cap)
        ok &= _same(auto, base)
        arms["k23_join"] = lambda: _lib.hamming_join(ctx, dev, None, hmax, capacity=cap)
    if checks > skip_factor * all_pairs:
        res["index"] = f"not timed: checks are {checks / all_pairs:.1f} x all pairs"
    else:
        got = _lib.hamming_join_indexed(ctx, dev, None, hmax, capacity=cap, counters=True)
        ok &= _same(got, auto) and got[3]["route"] == 1 and got[3]["checks"] == checks
        res["items"] = got[3]["items"]
        arms["k24_join"] = lambda: _lib.hamming_join_indexed(ctx, dev, None, hmax, capacity=cap)
        arms["auto_join"] = lambda: _lib.hamming_join_indexed(ctx, dev, None, hmax, auto=True, capacity=cap)
        if with_components:
            label, pairs, comps = _lib.hamming_components_indexed(ctx, dev, hmax)
            ok &= pairs == auto[3]["pairs"]
            res["components"] = int(comps)
            arms["k24_components"] = lambda: _lib.hamming_components_indexed(ctx, dev, hmax)
            if with_k23:
                k_label, k_pairs, k_comps = _lib.hamming_components(ctx, dev, hmax)
                ok &= np.array_equal(label, k_label) and (k_pairs, k_comps) == (pairs, comps)
                arms["k23_components"] = lambda: _lib.hamming_components(ctx, dev, hmax)
    res["results_equal"] = bool(ok)
    ms = {arm: [] for arm in arms}
    for arm, fn in arms.items():
        fn()                                           # (the second warm-up call of the arm)
    for _ in range(repeats):
        for arm, fn in arms.items():
            ms[arm].append(_timed(ctx, fn)[0])
    res.update({arm: _stats(v) for arm, v in ms.items()})
    if "k24_join" in arms:
        ctx.prof_enable(True)
        ctx.prof_reset()
        arms["k24_join"]()
        ctx.sync()
        res["index_split_ms"] = {k: ctx.prof_get(k)[0] for k in SCOPES}
        ctx.prof_enable(False)
        if with_k23 and checks:
            res["rho"] = (res["k24_join"]["ms_median"] / checks) / (res["k23_join"]["ms_median"] / all_pairs)
            res["k24_over_k23"] = res["k24_join"]["ms_median"] / res["k23_join"]["ms_median"]
    print(f"[bench_hamming_index] {n} x {dev.dim} hmax {hmax}: " + json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)})
          + " " + " ".join(f"{a} {res[a]['ms_median']:.3f} ms" for a in arms), file=sys.stderr, flush=True)
    return res, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", default="sweep", choices=("sweep", "scale"))
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--dims", default="64,256,768")
    ap.add_argument("--scale-n", default="100000,1000000")
    ap.add_argument("--k23-max-n", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-factor", type=float, default=4.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="what to record as the measured commit (default: git's HEAD)")
    args = ap.parse_args()
    import polyfuzz_amd
    from polyfuzz_amd import _lib
    ctx = polyfuzz_amd.Context.default()
    res = {"commit": args.commit or _commit(), "device": ctx.info()["name"], "arm": args.arm, "repeats": args.repeats,
           "skip_factor": args.skip_factor, "data": {}}
    ok = True
    if args.arm == "sweep":
        for d in (int(v) for v in args.dims.split(",")):
            cutoffs = list(range(13)) if d == 64 else sorted({_lib.hamming_max_distance(d, t) for t in SIMILARITIES})
            for name, make in (("clustered", clustered), ("uniform", uniform)):
                dev = _lib.DeviceDense.upload_bits(ctx, make(args.n, d))
                per = res["data"][f"{name} {args.n}x{d}"] = {}
                for hmax in cutoffs:
                    per[f"h{hmax}"], same = point(ctx, _lib, dev, args.n, hmax, args.repeats, args.skip_factor)
                    ok &= same
        rhos = [e["rho"] for per in res["data"].values() for e in per.values() if "rho" in e]
        if rhos:
            res["rho_max"] = max(rhos)
            res["ratio_rounded_up_to_a_power_of_two"] = 1 << max(0, int(np.ceil(np.log2(max(rhos)))))
    else:
        for n in (int(v) for v in args.scale_n.split(",")):
            dev = _lib.DeviceDense.upload_bits(ctx, uniform(n, 64))
            e, same = point(ctx, _lib, dev, n, 3, args.repeats, args.skip_factor, with_k23=n <= args.k23_max_n, with_components=True)
            if n > args.k23_max_n:
                e["k23_join"] = e["k23_components"] = "not run"
            res["data"][f"uniform {n}x64"] = {"h3": e}
            ok &= same
    print(json.dumps(res))
    out = args.out or os.path.join(REPO, "profiles", f"hamming_index_{res['commit']}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    if not ok:
        print("[bench_hamming_index] the routes disagree -- see results_equal in the JSON above", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
