"""
Config 3's lists under Levenshtein and OSA similarity, from the oracle (tests/lev_oracle.py: the Wagner-Fischer table, one
from-string against all to-strings per numpy row step; np.argmax's FIRST maximum):

    2 000 seeded from-rows of `polyfuzz_amd.datasets.c3_lists()` against all 20 000 to-titles -- the lists K9 is measured on.

rapidfuzz is not installable here, so this is the ORACLE's restatement (`source: "oracle"`; the rapidfuzz pin stays open).  What the
fixture buys: the GPU suite holds K9 -- its walk from the nearest lengths outwards and the length bound that ends it -- to the
definition at the width its timing is quoted at.  The score is not stored: it is 1.0 - distance / M, float64, recomputed by the test.

4e7 pairs per scorer: a few minutes on 8 processes for both.

Output: tests/golden/c3_lev_oracle.npz (tens of kilobytes): rows int32[2 000] (sorted), seed, and per scorer idx_<scorer> int32,
distance_<scorer> int32, M_<scorer> int32 (max of the two lengths of the winning pair); source and the SHA-256 of the two lists.
tests/test_lev_golden_cpu.py recomputes a seeded sample live.

    python tests/golden/make_golden_c3_lev.py [processes]
"""
import multiprocessing
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from tests import lev_oracle  # noqa: E402

SEED, N_ROWS = 9, 2000
PATH = os.path.join(HERE, "c3_lev_oracle.npz")


def lists():
    from polyfuzz_amd import datasets
    fl, tl = datasets.c3_lists()
    assert len(fl) == len(tl) == 20_000 and fl[0] == "Polly Blue Eyes"
    return fl, tl


def lists_sha256(from_list, to_list):
    import hashlib
    h = hashlib.sha256()
    for lst in (from_list, to_list):
        h.update("\0".join(lst).encode("utf-8", "surrogatepass"))
        h.update(b"\0\0")
    return h.hexdigest()


def best_rows(from_rows, to_list, scorer):
    """(idx, distance, M) of the first maximum of every from-string"""
    d = lev_oracle.matrix(from_rows, to_list, scorer)
    idx, _ = lev_oracle.argmax(lev_oracle.sim_matrix(from_rows, to_list, d))
    la, lb = lev_oracle.lengths(from_rows), lev_oracle.lengths(to_list)
    return idx, d[np.arange(len(from_rows)), idx].astype(np.int32), np.maximum(la, lb[idx]).astype(np.int32)


def _job(args):
    rows, scorer = args
    fl, tl = lists()
    return best_rows([fl[i] for i in rows], tl, scorer)


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else min(16, os.cpu_count() or 1)
    fl, tl = lists()
    rows = np.sort(np.random.default_rng(SEED).choice(len(fl), N_ROWS, replace=False)).astype(np.int32)
    out = {"rows": rows, "seed": np.array(SEED), "source": np.array("oracle"), "lists_sha256": np.array(lists_sha256(fl, tl))}
    with multiprocessing.Pool(procs) as pool:
        for scorer in lev_oracle.SCORERS:
            t0 = time.time()
            shards = np.array_split(rows, procs * 8)
            parts = pool.map(_job, [(s, scorer) for s in shards], chunksize=1)
            for k, name in enumerate(("idx", "distance", "M")):
                out[f"{name}_{scorer}"] = np.concatenate([p[k] for p in parts]).astype(np.int32)
            print(f"{scorer}: {N_ROWS} rows in {time.time() - t0:.0f} s on {procs} processes", flush=True)
    tmp = PATH[:-4] + ".part.npz"
    np.savez_compressed(tmp, **out)
    os.replace(tmp, PATH)
    print(f"{os.path.basename(PATH)}: {os.path.getsize(PATH)} bytes")
    assert os.path.getsize(PATH) < (1 << 20)


if __name__ == "__main__":
    main()
