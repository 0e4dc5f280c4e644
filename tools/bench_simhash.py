"""K25, the SimHash fingerprints behind SimHash.join / .components / .match (pfz_simhash), in one process, device events, medians.

usage: python tools/bench_simhash.py [--arm kernel|calls|quality|all] [--n 100000] [--big-n 1000000] [--repeats 7] [--out FILE] [--commit TEXT]

Arm `kernel`: the resident list of the first n company names (and big-n names of synth.company_names): the pfz_simhash call at 64
and 256 bits (fingerprint launch, scan, compaction, the row download) and its profiled split, beside pfz_tfidf_transform of the same
names with a vocabulary fitted on them -- on a fresh handle every time: the handle of the fit holds its n-grams already --, timed the same way.  `ratio` = K25's launches over the transform's device time.
Arm `calls`: whole calls on the n names -- SimHash.join / .components at max_distance 3 / 6 / 10 with their last_timings split
(fingerprint = pack + upload + K25, device = the Hamming stage, frame), and beside them TFIDF.join / .components at 0.9 / 0.8 and
EditDistance("levenshtein").components at 0.9; big-n names: SimHash.components at distance 3.  Wall-clock milliseconds.
Arm `quality`: pair recall and precision of the SimHash self-join at 3 / 6 / 10 of 64 bits (and at 128 bits with the distances
doubled) against the pairs of TFIDF.join at 0.9 / 0.8 on the n names.
Prints one JSON object; --out also writes it (default: profiles/simhash_<commit>.json).  Run it under a time limit."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import numpy as np

from bench_dense_join import _commit, _stats, _timed

K25_SCOPES = ("k25_fingerprint", "k25_compact")
K1_SCOPES = ("k1_extract", "k2_rows_short", "k2_rows_long", "k2_df_hist", "k2_finalize")


def _split(ctx, fn, scopes):
    ctx.prof_enable(True)
    ctx.prof_reset()
    fn()
    ctx.sync()
    out = {k: ctx.prof_get(k)[0] for k in scopes}
    ctx.prof_enable(False)
    return out


def kernel_arm(ctx, _lib, names, repeats):
    res = {"strings": len(names), "characters": int(sum(map(len, names)))}
    dev = _lib.DeviceStrings.upload(ctx, names)
    params = _lib.TfidfParams(3, 3, 1, 1)
    vec = _lib.DeviceTfidf.fit(ctx, params, dev)
    # A transform of the list the vocabulary was fitted on finds the fit's n-grams cached on the handle and only normalises; every
    # timed transform therefore gets a handle of its own, uploaded beforehand, that no kernel has seen (K25 keeps nothing on a handle)
    fresh = [_lib.DeviceStrings.upload(ctx, names) for _ in range(repeats + 3)]
    arms = {"tfidf_transform": lambda: vec.transform(fresh.pop())}
    for bits in (64, 256):
        arms[f"simhash_{bits}"] = lambda bits=bits: _lib.simhash(ctx, dev, params, bits)
    ms = {a: [] for a in arms}
    for fn in arms.values():
        fn()
        fn()
    for _ in range(repeats):
        for a, fn in arms.items():
            ms[a].append(_timed(ctx, fn)[0])
    res.update({a: _stats(v) for a, v in ms.items()})
    res["tfidf_transform"]["split_ms"] = _split(ctx, arms["tfidf_transform"], K1_SCOPES)
    res["tfidf_transform_cached_ngrams"] = _stats([_timed(ctx, lambda: vec.transform(dev))[0] for _ in range(repeats)])
    for bits in (64, 256):
        e = res[f"simhash_{bits}"]
        e["split_ms"] = _split(ctx, arms[f"simhash_{bits}"], K25_SCOPES)
        e["launches_over_transform_device_time"] = sum(e["split_ms"].values()) / max(sum(res["tfidf_transform"]["split_ms"].values()), 1e-9)
        e["call_over_transform_call"] = e["ms_median"] / res["tfidf_transform"]["ms_median"]
    _, row, windows = _lib.simhash(ctx, dev, params, 64)
    res["windowless"], res["windows"] = int((row < 0).sum()), int(windows.sum())
    print("[bench_simhash] kernel " + json.dumps(res), file=sys.stderr, flush=True)
    return res


def _wall(fn, repeats):
    fn()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def calls_arm(names, big, repeats):
    from polyfuzz_amd.models import TFIDF, EditDistance, SimHash
    res = {"strings": len(names)}
    for hmax in (3, 6, 10):
        for what in ("join", "components"):
            m = SimHash()
            parts = {"fingerprint": [], "device": [], "frame": []}

            def run():
                out = getattr(m, what)(names, max_distance=hmax)
                for k in parts:
                    parts[k].append(m.last_timings[k])
                return out
            e = _stats(_wall(run, repeats))
            e.update({f"{k}_ms_median": float(np.median(v[1:])) for k, v in parts.items()})
            e["counts"] = {k: int(v) for k, v in m.last_counts.items()}
            res[f"simhash_{what}_h{hmax}"] = e
            print(f"[bench_simhash] simhash {what} h{hmax} " + json.dumps(e), file=sys.stderr, flush=True)
    for t in (0.9, 0.8):
        for what in ("join", "components"):
            m = TFIDF()
            e = _stats(_wall(lambda: getattr(m, what)(names, min_similarity=t), repeats))
            e["counts"] = {k: int(v) for k, v in m.last_counts.items()}
            res[f"tfidf_{what}_{t}"] = e
            print(f"[bench_simhash] tfidf {what} {t} " + json.dumps(e), file=sys.stderr, flush=True)
    m = EditDistance(scorer="levenshtein")
    e = _stats(_wall(lambda: m.components(names, 0.9), max(1, repeats // 3)))
    e["counts"] = {k: int(v) for k, v in m.last_counts.items()}
    res["levenshtein_components_0.9"] = e
    if big:
        m = SimHash()
        e = _stats(_wall(lambda: m.components(big, max_distance=3), max(1, repeats // 2)))
        e.update({"strings": len(big), "counts": {k: int(v) for k, v in m.last_counts.items()}, "last_timings": m.last_timings})
        res["simhash_components_h3_big"] = e
    print("[bench_simhash] calls done", file=sys.stderr, flush=True)
    return res


def _pair_keys(frame, position):
    a = np.array([position[s] for s in frame["From"]], np.int64)
    b = np.array([position[s] for s in frame["To"]], np.int64)
    return set((np.minimum(a, b) * (1 << 32) + np.maximum(a, b)).tolist())


def quality_arm(names):
    """on the distinct names (a frame names strings, and equal strings are trivially pairs of both matchers)"""
    from polyfuzz_amd.models import TFIDF, SimHash
    names = sorted(set(names))
    position = {s: i for i, s in enumerate(names)}
    truth = {t: _pair_keys(TFIDF().join(names, min_similarity=t), position) for t in (0.9, 0.8)}
    res = {"distinct_strings": len(names), "tfidf_pairs": {str(t): len(v) for t, v in truth.items()}}
    for bits, scale in ((64, 1), (128, 2)):
        for hmax in (3, 6, 10):
            got = _pair_keys(SimHash(bits=bits).join(names, max_distance=hmax * scale), position)
            e = {"pairs": len(got)}
            for t, want in truth.items():
                both = len(got & want)
                e[f"recall_vs_{t}"] = both / max(len(want), 1)
                e[f"precision_vs_{t}"] = both / max(len(got), 1)
            res[f"{bits}_bits_h{hmax * scale}"] = e
    print("[bench_simhash] quality " + json.dumps(res), file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", default="all", choices=("kernel", "calls", "quality", "all"))
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--big-n", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="what to record as the measured commit (default: git's HEAD)")
    args = ap.parse_args()
    import polyfuzz_amd
    from polyfuzz_amd import _lib, datasets, synth
    ctx = polyfuzz_amd.Context.default()
    names = list(datasets.load_company_names()[:args.n])
    big = list(synth.company_names(args.big_n, 25)) if args.big_n else []
    res = {"commit": args.commit or _commit(), "device": ctx.info()["name"], "repeats": args.repeats}
    if args.arm in ("kernel", "all"):
        res["kernel"] = {"names": kernel_arm(ctx, _lib, names, args.repeats)}
        if big:
            res["kernel"]["synthetic"] = kernel_arm(ctx, _lib, big, args.repeats)
    if args.arm in ("calls", "all"):
        res["calls"] = calls_arm(names, big, args.repeats)
    if args.arm in ("quality", "all"):
        res["quality"] = quality_arm(names)
    print(json.dumps(res))
    out = args.out or os.path.join(REPO, "profiles", f"simhash_{res['commit']}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
