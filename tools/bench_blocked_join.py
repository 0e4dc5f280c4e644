"""K16, the threshold join over TF-IDF candidates (BlockedEditDistance.join), beside the exact all-pairs join (K11) and beside
BlockedEditDistance.match at the same `candidates` (K10), in one process:

  companies  the 100 000 company names against themselves, "levenshtein", t = 0.9 / 0.8, candidates = 8 / 32 / 128.  Arms, in turn:
             EditDistance("levenshtein").join (K11: every pair), BlockedEditDistance.match, BlockedEditDistance.join;
  titles     BASELINE configuration 3, the 20 000 x 20 000 IMDB titles, "jaro_winkler", t = 0.9 / 0.8, the same candidates; both
             lists resident (re_train=False after a first call).  Jaro has no all-pairs join: the reference pairs are K8's matrix
             (pfz_jaro_matrix_host) thresholded on the host in row slices.

usage: python tools/bench_blocked_join.py [--companies 100000] [--titles 20000] [--repeats 5] [--commit ID] [--out FILE]

Per arm: the wall time of a call (median of `repeats`, after two warming calls).  Per join arm also the split of the call
(BlockedEditDistance.last_timings: the TF-IDF stage, the K16 entry, the frame), the K16 scopes of one profiled pass -- k16_keys_sort
(keys, sort, row pointers), k16_pairs_join (the scoring launches), k16_pairs_join_general, k16_compact (scan and compaction) --, the
three counters (table cells that are a candidate pair, distinct pairs scored, hits) and the PAIR RECALL: the blocked join's hits
that are also the exact join's, over the exact join's -- computed exactly, both are CSR.  (Every blocked hit is an exact hit: the
scores are the same function of the same two strings.)
Prints one JSON object; --out also writes it (default: profiles/blocked_join_<commit>.json).  Run it under a time limit."""
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
CANDIDATES = (8, 32, 128)
SCOPES = ("k16_keys_sort", "k16_pairs_join", "k16_pairs_join_general", "k16_compact")


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


def _keys(row_ptr, idx, n_to):
    return np.repeat(np.arange(len(row_ptr) - 1, dtype=np.int64), np.diff(row_ptr)) * n_to + idx


def blocked_arms(ctx, _lib, scorer, from_list, to_list, exact_keys, repeats):
    """{candidates: {"match": ..., "join_t<t>": ...}} for one data set; exact_keys: {t: sorted int64 keys row * n_to + col of the
    exact join}"""
    from polyfuzz_amd.models import BlockedEditDistance
    n_to = len(from_list if to_list is None else to_list)
    kw = {} if to_list is None else {"re_train": False}
    out = {}
    for c in CANDIDATES:
        m = BlockedEditDistance(scorer=scorer, candidates=c, top_n=1, normalize=False)
        m.match(from_list, to_list)                                      # (fits the TF-IDF side, uploads the to-list)
        m.match(from_list, to_list, **kw)
        r = {}
        r["match_ms"], r["match_ms_all"] = _median_ms(lambda: m.match(from_list, to_list, **kw), repeats)
        r["match_split_ms"] = dict(m.last_timings)
        for t in THRESHOLDS:
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
            _, f_dev, t_dev, cand, *_ = m._block(from_list, to_list, kw.get("re_train", True))
            row_ptr, idx, _ = _lib.pairs_join(ctx, f_dev, None if to_list is None else t_dev, cand, scorer, t)
            got = _keys(row_ptr, idx, n_to)
            assert len(got) == j["counters"]["pairs"]
            common = int(np.isin(got, exact_keys[t], assume_unique=True).sum())
            j["blocked_hits_that_are_exact_hits"] = common
            j["exact_hits"] = int(len(exact_keys[t]))
            j["pair_recall"] = common / max(1, len(exact_keys[t]))
            j["join_over_match_same_candidates"] = j["join_ms"] / r["match_ms"]
            r[f"join_t{t}"] = j
            print(f"[bench_blocked_join] {scorer} candidates {c} t {t}: {json.dumps(j)}", file=sys.stderr, flush=True)
        out[str(c)] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--companies", type=int, default=100_000)
    ap.add_argument("--titles", type=int, default=20_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--commit", default=None, help="the commit the tree was built from, where git cannot tell")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import polyfuzz_amd
    from polyfuzz_amd import _lib, datasets
    from polyfuzz_amd.models import EditDistance
    ctx = polyfuzz_amd.Context.default()
    res = {"commit": args.commit or _commit(), "device": ctx.info()["name"], "repeats": args.repeats, "thresholds": list(THRESHOLDS),
           "candidates": list(CANDIDATES), "wall": "time.perf_counter around the matcher's call, result frame included"}
    out = args.out or os.path.join(REPO, "profiles", f"blocked_join_{res['commit']}.json")
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
            row_ptr, idx, _, _ = _lib.lev_join(ctx, f, None, "levenshtein", t)
            exact[t] = _keys(row_ptr, idx, n)
            e["hits"] = int(len(idx))
            d["exact"][f"t{t}"] = e
        d["blocked"] = blocked_arms(ctx, _lib, "levenshtein", names, None, exact, args.repeats)
        for c in d["blocked"].values():
            for t in THRESHOLDS:
                c[f"join_t{t}"]["k11_join_over_blocked_join"] = d["exact"][f"t{t}"]["k11_join_ms"] / c[f"join_t{t}"]["join_ms"]
        res["companies"] = d
        write()
    if args.titles > 0:
        fl, tl = datasets.c3_lists(args.titles)
        n, n_to = len(fl), len(tl)
        d = {"shape": [n, n_to], "data": "datasets.c3_lists (IMDB titles), two lists", "scorer": "jaro_winkler"}
        f, t_dev = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
        lo = min(THRESHOLDS)
        rows, cols, vals = [], [], []
        t0 = time.perf_counter()
        for b in range(0, n, 1000):                                   # (the full matrix is n * n_to * 8 bytes: row slices)
            m = _lib.jaro_matrix(ctx, f, t_dev, "jaro_winkler", b, min(n, b + 1000))
            i, j = np.nonzero(m >= lo)
            rows.append(i.astype(np.int64) + b)
            cols.append(j.astype(np.int64))
            vals.append(m[i, j])
        d["exact_matrix_and_threshold_s"] = time.perf_counter() - t0
        rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
        exact = {t: (rows * n_to + cols)[vals >= t] for t in THRESHOLDS}
        d["exact"] = {f"t{t}": {"hits": int(len(exact[t]))} for t in THRESHOLDS}
        d["blocked"] = blocked_arms(ctx, _lib, "jaro_winkler", fl, tl, exact, args.repeats)
        res["titles"] = d
        write()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
