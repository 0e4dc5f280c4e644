"""K17, BlockedEditDistance.join / .components behind a TF-IDF THRESHOLD join (blocking_similarity), beside today's table path
(`candidates`) and beside the exact all-pairs join (K11), in one process:

  companies  the 100 000 company names against themselves, "levenshtein", t = 0.9 / 0.8.  Arms, in turn: EditDistance.join and
             .components (K11 / K12: every pair), candidates = 32 / 128 (K16), blocking_similarity = 0.8 / 0.6 / 0.5 / 0.4 (K17);
  titles     BASELINE configuration 3, the 20 000 x 20 000 IMDB titles, "jaro_winkler", t = 0.9, both lists resident
             (re_train=False after a first call).  Jaro has no all-pairs join: the reference pairs are K8's matrix
             (pfz_jaro_matrix_host) thresholded on the host in row slices;
  slices     the S table: the companies arm at blocking_similarity = 0.6, t = 0.9 under what-if builds of the library with
             another kPairSlice (tools/build_variant.sh <out.so> -DPFZ_PAIR_SLICE=n, 0: whole rows), one child process each,
             one after the other: --slice-libs 64=variants/a.so,128=...,0=...  The shipped library is measured the same way.

usage: python tools/bench_blocked_threshold.py [--companies 100000] [--titles 20000] [--repeats 5] [--slice-libs S=LIB,...]
                                                [--commit ID] [--out FILE]

Per arm: the wall time of the matcher's call (median of `repeats`, after two warming calls), its split (last_timings: the blocking
stage -- for K17 the TF-IDF vectoriser, K15 and its sort --, the K16 / K17 entry, the frame), the device scopes of one profiled
pass (k15_join, k15_sort, k16_keys_sort, k17_items, k16_pairs_join, k16_pairs_join_general, k16_compact), the counters (keys or
table cells, pairs scored, hits, work items) and the PAIR RECALL against the exact join, computed exactly: both are CSR.
Prints one JSON object; --out also writes it (default: profiles/blocked_threshold_<commit>.json).  Run it under a time limit."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np

THRESHOLDS = (0.9, 0.8)
BLOCKING = (0.8, 0.6, 0.5, 0.4)
CANDIDATES = (32, 128)
SCOPES = ("k15_join", "k15_sort", "k16_keys_sort", "k17_items", "k16_pairs_join", "k16_pairs_join_general", "k16_compact")


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


def _keys(frame_rows, idx, n_to):
    return frame_rows.astype(np.int64) * n_to + idx


def _csr_keys(row_ptr, idx, n_to):
    return _keys(np.repeat(np.arange(len(row_ptr) - 1, dtype=np.int64), np.diff(row_ptr)), idx, n_to)


def _arm(ctx, _lib, m, from_list, to_list, t, exact_keys, repeats, kw, components):
    """one matcher at one threshold: the join (and, for a self-join, the components)"""
    n_to = len(from_list if to_list is None else to_list)
    for _ in range(2):
        m.join(from_list, to_list, t, **kw)
    splits = []

    def once():
        m.join(from_list, to_list, t, **kw)
        splits.append(dict(m.last_timings))
    j = {}
    j["join_ms"], j["join_ms_all"] = _median_ms(once, repeats)
    for key in ("tfidf", "k16", "frame"):
        j[f"{key}_ms"] = float(np.median([s[key] for s in splits]))
    j["counters"] = dict(m.last_counts)
    ctx.prof_enable(True)
    ctx.prof_reset()
    m.join(from_list, to_list, t, **kw)
    ctx.sync()
    j["scopes_ms_profiled_pass"] = {s: ctx.prof_get(s)[0] for s in SCOPES}
    ctx.prof_enable(False)
    # the same hits as indices: the matcher's own blocking stage, then the binding
    _, f_dev, t_dev, cand, *_ = m._block(from_list, to_list, kw.get("re_train", True), m.blocking_similarity)
    join = _lib.pairs_join if m.blocking_similarity is None else _lib.pairs_join_keys
    row_ptr, idx, _ = join(ctx, f_dev, None if to_list is None else t_dev, cand, m._scorer_name, t)
    got = _csr_keys(row_ptr, idx, n_to)
    assert len(got) == j["counters"]["pairs"]
    common = int(np.isin(got, exact_keys, assume_unique=True).sum())
    j["hits_that_are_exact_hits"] = common
    j["exact_hits"] = int(len(exact_keys))
    j["pair_recall"] = common / max(1, len(exact_keys))
    if components:
        for _ in range(2):
            m.components(from_list, t)
        j["components_ms"], j["components_ms_all"] = _median_ms(lambda: m.components(from_list, t), repeats)
        j["components_counters"] = dict(m.last_counts)
    return j


def _arms(ctx, _lib, scorer, from_list, to_list, exact, repeats, thresholds):
    from polyfuzz_amd.models import BlockedEditDistance
    kw = {} if to_list is None else {"re_train": False}
    out = {}
    arms = [(f"candidates_{c}", {"candidates": c}) for c in CANDIDATES] + [(f"blocking_{b}", {"blocking_similarity": b}) for b in BLOCKING]
    for label, args in arms:
        m = BlockedEditDistance(scorer=scorer, top_n=1, normalize=False, **args)
        m.join(from_list, to_list, thresholds[0])                          # (fits the TF-IDF side, uploads the to-list)
        r = {}
        for t in thresholds:
            r[f"t{t}"] = _arm(ctx, _lib, m, from_list, to_list, t, exact[t], repeats, kw, to_list is None)
            print(f"[bench_blocked_threshold] {scorer} {label} t {t}: {json.dumps(r[f't{t}'])}", file=sys.stderr, flush=True)
        out[label] = r
    return out


def _slice_arm(args):
    """the child of the S table: the library POLYFUZZ_HIP_LIB names (or the shipped one) on the companies arm at b = 0.6, t = 0.9"""
    import polyfuzz_amd
    from polyfuzz_amd import datasets
    from polyfuzz_amd.models import BlockedEditDistance
    ctx = polyfuzz_amd.Context.default()
    names = datasets.load_company_names()[:args.companies]
    m = BlockedEditDistance(scorer="levenshtein", normalize=False, blocking_similarity=0.6)
    for _ in range(3):
        m.join(names, None, 0.9)
    splits = []

    def once():
        m.join(names, None, 0.9)
        splits.append(dict(m.last_timings))
    r = {}
    r["join_ms"], r["join_ms_all"] = _median_ms(once, args.repeats)
    r["k16_ms"] = float(np.median([s["k16"] for s in splits]))
    r["k16_ms_all"] = [round(s["k16"], 3) for s in splits]
    r["counters"] = dict(m.last_counts)
    ctx.prof_enable(True)
    scopes = []
    for _ in range(args.repeats):
        ctx.prof_reset()
        m.join(names, None, 0.9)
        ctx.sync()
        scopes.append({s: ctx.prof_get(s)[0] for s in SCOPES})
    ctx.prof_enable(False)
    r["scopes_ms_median_of_profiled_passes"] = {s: float(np.median([p[s] for p in scopes])) for s in SCOPES}
    print(json.dumps(r))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--companies", type=int, default=100_000)
    ap.add_argument("--titles", type=int, default=20_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--slice-libs", default="", help="S=LIB,... what-if builds for the S table (0: whole rows)")
    ap.add_argument("--slice-arm", action="store_true", help="(internal) run the S table's arm in this process and print it")
    ap.add_argument("--commit", default=None, help="the commit the tree was built from, where git cannot tell")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.slice_arm:
        return _slice_arm(args)
    import polyfuzz_amd
    from polyfuzz_amd import _lib, datasets
    from polyfuzz_amd.models import EditDistance
    ctx = polyfuzz_amd.Context.default()
    res = {"commit": args.commit or _commit(), "device": ctx.info()["name"], "repeats": args.repeats, "thresholds": list(THRESHOLDS),
           "blocking_similarity": list(BLOCKING), "candidates": list(CANDIDATES), "pair_slice": _lib.PAIR_SLICE,
           "wall": "time.perf_counter around the matcher's call, result frame included"}
    out = args.out or os.path.join(REPO, "profiles", f"blocked_threshold_{res['commit']}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)

    def write():
        with open(out, "w") as fh:
            json.dump(res, fh, indent=1)

    if args.companies > 0:
        names = datasets.load_company_names()[:args.companies]
        n = len(names)
        d = {"shape": [n, n], "data": "datasets.load_company_names, self-join", "scorer": "levenshtein", "exact": {}}
        ed = EditDistance(scorer="levenshtein", normalize=False)
        f = _lib.DeviceStrings.upload(ctx, names)
        exact = {}
        for t in THRESHOLDS:
            for _ in range(2):
                ed.join(names, min_similarity=t)
            e = {}
            e["k11_join_ms"], e["k11_join_ms_all"] = _median_ms(lambda: ed.join(names, min_similarity=t), args.repeats)
            ed.components(names, t)
            e["k12_components_ms"], e["k12_components_ms_all"] = _median_ms(lambda: ed.components(names, t), args.repeats)
            row_ptr, idx, _, _ = _lib.lev_join(ctx, f, None, "levenshtein", t)
            exact[t] = _csr_keys(row_ptr, idx, n)
            e["hits"] = int(len(idx))
            d["exact"][f"t{t}"] = e
            print(f"[bench_blocked_threshold] exact t {t}: {json.dumps(e)}", file=sys.stderr, flush=True)
        d["arms"] = _arms(ctx, _lib, "levenshtein", names, None, exact, args.repeats, THRESHOLDS)
        res["companies"] = d
        write()
    if args.titles > 0:
        fl, tl = datasets.c3_lists(args.titles)
        n, n_to = len(fl), len(tl)
        d = {"shape": [n, n_to], "data": "datasets.c3_lists (IMDB titles), two lists", "scorer": "jaro_winkler"}
        f, t_dev = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
        t = 0.9
        rows, cols = [], []
        t0 = time.perf_counter()
        for b in range(0, n, 1000):                                   # (the full matrix is n * n_to * 8 bytes: row slices)
            m = _lib.jaro_matrix(ctx, f, t_dev, "jaro_winkler", b, min(n, b + 1000))
            i, j = np.nonzero(m >= t)
            rows.append(i.astype(np.int64) + b)
            cols.append(j.astype(np.int64))
        d["exact_matrix_and_threshold_s"] = time.perf_counter() - t0
        exact = {t: np.concatenate(rows) * n_to + np.concatenate(cols)}
        d["exact"] = {f"t{t}": {"hits": int(len(exact[t]))}}
        d["arms"] = _arms(ctx, _lib, "jaro_winkler", fl, tl, exact, args.repeats, (t,))
        res["titles"] = d
        write()
    if args.slice_libs:
        table = {}
        libs = [("shipped", None)] + [tuple(item.split("=", 1)) for item in args.slice_libs.split(",")]
        for label, lib in libs:
            env = dict(os.environ)
            if lib:
                env["POLYFUZZ_HIP_LIB"] = os.path.abspath(lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--slice-arm", "--companies", str(args.companies or 100_000),
                   "--repeats", str(args.repeats)]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise RuntimeError(f"slice arm {label} failed: {p.stderr[-2000:]}")
            table[label] = json.loads(p.stdout.strip().splitlines()[-1])
            print(f"[bench_blocked_threshold] slice {label}: {json.dumps(table[label])}", file=sys.stderr, flush=True)
        res["slices"] = {"arm": "companies, blocking_similarity 0.6, t 0.9", "pair_slice_of": table}
        write()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
