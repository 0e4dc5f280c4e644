"""
Config 3's lists under a Levenshtein / OSA similarity THRESHOLD, from the oracle (tests/lev_oracle.py: the Wagner-Fischer table):

    every pair with similarity >= FLOOR among the 2 000 seeded from-rows of c3_lev_oracle.npz x all 20 000 to-titles,

the lists EditDistance.join (K11) is measured on.  What the fixture buys: the GPU suite holds K11 -- its length window, its
per-pair cutoff and the walk it abandons -- to the definition at title width, at the floor and at every threshold above it (a
join at t >= FLOOR is this list filtered by `similarity >= t`).  The score is not stored: it is 1.0 - distance / M, float64,
recomputed by the test from the distance and the two lengths.

rapidfuzz is not installable here, so this is the ORACLE's restatement (`source: "oracle"`).  4e7 pairs per scorer: a few minutes on
8 processes for both.  The floor starts at 0.5 and is raised in steps of 0.05 while the file would exceed 1 MiB; the value chosen
is stored.

Output: tests/golden/c3_lev_join_oracle.npz: rows int32[2 000] (the from-rows, as in c3_lev_oracle.npz), floor float64, and per
scorer from_<scorer> int32 (position in `rows`), to_<scorer> int32, distance_<scorer> int32 in row-major order (from, then to);
source and the SHA-256 of the two lists.  tests/test_join_cpu.py recomputes a seeded sample of rows live.

    python tests/golden/make_golden_c3_lev_join.py [processes]
"""
import multiprocessing
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from tests import lev_oracle  # noqa: E402
from make_golden_c3_lev import lists, lists_sha256  # noqa: E402

FLOOR = 0.5
PATH = os.path.join(HERE, "c3_lev_join_oracle.npz")
ROWS_PATH = os.path.join(HERE, "c3_lev_oracle.npz")


def hits(from_rows, to_list, scorer, floor):
    """(from position, to-index, distance) int32 of every pair with similarity >= floor, row-major"""
    d = lev_oracle.matrix(from_rows, to_list, scorer)
    i, j = np.nonzero(lev_oracle.sim_matrix(from_rows, to_list, d) >= floor)
    return i.astype(np.int32), j.astype(np.int32), d[i, j].astype(np.int32)


def _job(args):
    first, rows, scorer = args
    fl, tl = lists()
    i, j, d = hits([fl[r] for r in rows], tl, scorer, FLOOR)
    return i + np.int32(first), j, d


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else min(16, os.cpu_count() or 1)
    fl, tl = lists()
    rows = np.load(ROWS_PATH)["rows"].astype(np.int32)
    la, lb = lev_oracle.lengths([fl[r] for r in rows]), lev_oracle.lengths(tl)
    found = {}
    with multiprocessing.Pool(procs) as pool:
        for scorer in lev_oracle.SCORERS:
            t0 = time.time()
            shards = np.array_split(np.arange(len(rows)), procs * 8)
            parts = pool.map(_job, [(int(s[0]), rows[s], scorer) for s in shards if len(s)], chunksize=1)
            found[scorer] = [np.concatenate([p[k] for p in parts]) for k in range(3)]
            print(f"{scorer}: {len(found[scorer][0])} pairs >= {FLOOR} in {time.time() - t0:.0f} s on {procs} processes", flush=True)
    floor = FLOOR
    tmp = PATH[:-4] + ".part.npz"
    while True:
        out = {"rows": rows, "floor": np.array(floor), "source": np.array("oracle"), "lists_sha256": np.array(lists_sha256(fl, tl))}
        for scorer, (i, j, d) in found.items():
            keep = lev_oracle.similarity(d, la[i], lb[j]) >= floor
            out[f"from_{scorer}"], out[f"to_{scorer}"], out[f"distance_{scorer}"] = i[keep], j[keep], d[keep]
        np.savez_compressed(tmp, **out)
        if os.path.getsize(tmp) < (1 << 20):
            break
        floor = round(floor + 0.05, 2)
    os.replace(tmp, PATH)
    print(f"{os.path.basename(PATH)}: floor {floor}, {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
