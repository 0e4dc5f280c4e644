"""
Config 3's lists under Jaro and Jaro-Winkler, at full size, from the C oracle:

    oracle.jaro_argmax(from_list, to_list, scorer)   (oracle/jaro.c: np.argmax's FIRST maximum, np.max)

on `polyfuzz_amd.datasets.c3_lists()` -- the 20 000 x 20 000 IMDB titles K8 is measured on.  jellyfish is not
installable here, so this is the ORACLE's restatement (`source: "oracle"`; the jellyfish pin stays open): what the fixture buys is
that the GPU suite holds K8 to the definition on EVERY row of the size its timing is quoted at.

4e8 pairs per scorer at about a million pairs per second and core: a minute or two on 16 threads for both.

Output: tests/golden/c3_jaro_oracle_<scorer>.npz (each about 0.15 MB): idx int32[20 000], score float64[20 000], and beside them
scorer, source and the SHA-256 of the two lists.  tests/test_jaro_golden_cpu.py recomputes a seeded sample of both files live, so a
change to oracle/jaro.c that moves a value turns the suite red until this is rerun.

    python tests/golden/make_golden_c3_jaro.py [threads]
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

import oracle  # noqa: E402
from tests import helpers  # noqa: E402


def main():
    threads = int(sys.argv[1]) if len(sys.argv) > 1 else min(16, os.cpu_count() or 1)
    oracle.build_native()
    fl, tl = helpers.c3_fuzz_lists()
    digest = helpers.lists_sha256(fl, tl)
    for scorer in helpers.JARO_SCORERS:
        path = helpers.c3_jaro_golden_path(scorer)
        t0 = time.time()
        idx, score = helpers.jaro_oracle_argmax(oracle, fl, tl, scorer, workers=threads)
        assert idx.shape == score.shape == (len(fl),) and idx.dtype == np.int32 and score.dtype == np.float64
        tmp = path[:-4] + ".part.npz"
        np.savez_compressed(tmp, idx=idx, score=score, scorer=np.array(scorer), source=np.array("oracle"), lists_sha256=np.array(digest))
        os.replace(tmp, path)
        print(f"{scorer}: {len(fl)} rows in {time.time() - t0:.0f} s on {threads} threads -> {os.path.basename(path)} "
              f"{os.path.getsize(path)} bytes", flush=True)
        assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
