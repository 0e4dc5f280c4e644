"""
Config 3's lists under ALL TEN rapidfuzz.fuzz scorers, at full size, from the C oracle:

    oracle.fuzz_extract_one(from_list, to_list, scorer)   (oracle/fuzz_scorers.c / indel.c: process.extractOne's FIRST best choice)

on `polyfuzz_amd.datasets.c3_lists()` -- SURVEY section 8d's 20 000 x 20 000 IMDB titles, the lists `RapidFuzz().match` is benchmarked
on.  rapidfuzz is not installable here, so this is the ORACLE's restatement (`source: "oracle"`; the rapidfuzz pin of DESIGN section 2
stays open): what the fixture buys is that the GPU suite holds K7 to it on EVERY row of the configuration, not on a sample.

Cost on one core, seconds per from-row against the 20 000 to-titles: WRatio 0.37, partial_ratio 0.24, the five whole-string / token
scorers 0.013 - 0.031, the three partial_token_* scorers 0.27 - 0.54.  So: all 20 000 rows for the first seven (about half an hour on
eight cores), every 10th row (0, 10, 20, ...: 2 000 rows) for the three partial_token_* scorers.

Output: tests/golden/c3_fuzz_oracle_<scorer>.npz, one file per scorer (each well below 1 MiB; a scorer whose file exists with the
right lists and stride is skipped, so an interrupted run resumes):  idx int32 / score float64 per fixture row, and beside them
scorer, stride, source and the SHA-256 of the two lists.  tests/test_fuzz_golden_cpu.py recomputes a seeded sample of every file live,
so a change to oracle/fuzz_scorers.c that moves a value turns the suite red until this is rerun.

    python tests/golden/make_golden_c3_fuzz.py [threads] [scorer ...]
"""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

import oracle  # noqa: E402
from tests import helpers  # noqa: E402


def extract_rows(fl, tl, scorer, rows, threads, chunk=16):
    """oracle.fuzz_extract_one for the from-rows `rows` (ascending), in runs of consecutive rows on a thread pool (ctypes releases
    the GIL for the C call)."""
    rows = np.asarray(rows, np.int64)
    runs, start = [], 0                                           # [begin, end) runs of consecutive rows, at most `chunk` long
    for k in range(1, len(rows) + 1):
        if k == len(rows) or rows[k] != rows[k - 1] + 1 or k - start == chunk:
            runs.append((int(rows[start]), int(rows[k - 1]) + 1))
            start = k
    with ThreadPoolExecutor(threads) as pool:
        parts = list(pool.map(lambda r: oracle.fuzz_extract_one(fl, tl, scorer, rows=r), runs))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def main():
    args = sys.argv[1:]
    threads = int(args.pop(0)) if args and args[0].isdigit() else (os.cpu_count() or 1)
    todo = args or [s for s in helpers.C3_FUZZ_SCORERS]
    oracle.build_native()
    fl, tl = helpers.c3_fuzz_lists()
    digest = helpers.lists_sha256(fl, tl)
    for scorer in sorted(todo, key=lambda s: helpers.C3_FUZZ_SCORERS[s]):     # (the cheap files first)
        stride = helpers.C3_FUZZ_SCORERS[scorer]
        path = helpers.c3_fuzz_golden_path(scorer)
        if os.path.exists(path):
            g = np.load(path)
            if str(g["lists_sha256"]) == digest and int(g["stride"]) == stride and str(g["scorer"]) == scorer:
                print(f"{scorer}: {os.path.basename(path)} is there, skipped", flush=True)
                continue
        rows = np.arange(0, len(fl), stride)
        t0 = time.time()
        idx, score = extract_rows(fl, tl, scorer, rows, threads)
        assert len(idx) == len(rows) and idx.dtype == np.int32 and score.dtype == np.float64
        tmp = path[:-4] + ".part.npz"
        np.savez_compressed(tmp, idx=idx, score=score, scorer=np.array(scorer), stride=np.array(stride, np.int32),
                            source=np.array("oracle"), lists_sha256=np.array(digest))
        os.replace(tmp, path)
        print(f"{scorer}: {len(rows)} rows in {time.time() - t0:.0f} s on {threads} threads -> {os.path.basename(path)} "
              f"{os.path.getsize(path)} bytes", flush=True)
        assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
