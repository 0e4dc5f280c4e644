"""
The HEADLINE workload through the REFERENCE itself, in the build container (round 6, VERDICT r5 "next" 1b):

    polyfuzz.models.TFIDF(min_similarity=0, top_n=5, cosine_method="knn").match(names)

on all 100 000 company names -- `/root/reference/polyfuzz/models/_tfidf.py:68-100` ->
`_utils.py:59-70` (`NearestNeighbors(n_neighbors=top_n+1, n_jobs=-1, metric='cosine')`, neighbour column 0 dropped
as "self") -> `_utils.py:104-125` (the frame).  "knn" is the one back-end of the reference that fits 100k x 100k in
this container (the dense "sklearn" branch needs 80 GB; sparse_dot_topn is not installable), and BASELINE.md §3 lists
it as the reference arm of the headline.

The reference is not where the GPU tests run: the OUTPUT is committed (`headline_knn_golden_{0,1,2,3}.npz`, data only) with
this script (python tests/golden/make_golden_headline.py; ~6 min on 8 vCPU).

What is stored, per from-row r and rank k < 5:
* `idx[r, k]`  int32   -- the neighbour index the reference's kneighbors call returned (after ITS column-0 drop),
                          recorded by a spy around `NearestNeighbors.kneighbors` that changes nothing;
* `sim[r, k]`  float32 -- 1 - distance, un-rounded (float64 in the reference; float32 keeps 1e-7);
* `sim3[r, k]` uint16  -- the frame's Similarity column x 1000 (the reference's own 3-dp rounding + `< 0.001 -> 0`);
* `to_none[r, k]` bool -- the frame's To cell is None.
The script asserts the frame IS those arrays (To == names[idx], Similarity == sim3 / 1000) before writing, so the
fixture is the reference's `.match()` output, not an intermediate.

The quirk it carries (`_utils.py:61-65`): column 0 is dropped ASSUMING it is the row itself.  Where a
name has exact duplicates after cleaning (distance 0 ties), column 0 may be a duplicate and the row itself stays in
the list: the test treats a row's own index as one more zero-distance tie.
"""
import json
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)


def _install_stubs():
    """seaborn (plots) and rapidfuzz (other matchers) are absent here; neither is on this path."""
    sys.modules["seaborn"] = types.ModuleType("seaborn")
    rf = types.ModuleType("rapidfuzz")
    rf.fuzz = types.ModuleType("rapidfuzz.fuzz")
    rf.process = types.ModuleType("rapidfuzz.process")
    rf.fuzz.ratio = rf.fuzz.WRatio = None
    rf.process.extractOne = None
    sys.modules.update({"rapidfuzz": rf, "rapidfuzz.fuzz": rf.fuzz, "rapidfuzz.process": rf.process})


def main():
    _install_stubs()
    from polyfuzz.models import TFIDF
    from sklearn.neighbors import NearestNeighbors
    import sklearn

    names = json.load(open(os.path.join(REF, "data", "company_names.json")))
    assert len(names) == 100_000

    seen = {}
    real = NearestNeighbors.kneighbors

    def spy(self, X=None, n_neighbors=None, return_distance=True):
        out = real(self, X, n_neighbors, return_distance)
        seen["dist"], seen["idx"] = out
        return out

    NearestNeighbors.kneighbors = spy
    t0 = time.time()
    df = TFIDF(min_similarity=0, top_n=5, cosine_method="knn").match(names)
    wall = time.time() - t0
    NearestNeighbors.kneighbors = real
    print(f"reference .match(): {wall:.1f} s on {os.cpu_count()} cores")

    idx = np.ascontiguousarray(seen["idx"][:, 1:].astype(np.int32))
    sim64 = 1.0 - seen["dist"][:, 1:]
    sim3 = np.zeros((len(names), 5), np.uint16)
    to_none = np.zeros((len(names), 5), bool)
    assert df["From"].tolist() == names
    for k in range(5):
        tc = "To" if k == 0 else f"To_{k + 1}"
        sc = "Similarity" if k == 0 else f"Similarity_{k + 1}"
        to = df[tc].tolist()
        s = df[sc].to_numpy(np.float64)
        to_none[:, k] = [t is None for t in to]
        sim3[:, k] = np.rint(s * 1000).astype(np.uint16)
        assert np.abs(sim3[:, k] / 1000.0 - s).max() < 1e-12
        # the frame IS the spy's arrays
        exp = np.round(sim64[:, k], 3)
        exp[exp < 0.001] = 0.0
        assert np.array_equal(exp, s), (k, np.flatnonzero(exp != s)[:5])
        for r in np.flatnonzero(~to_none[:, k]):
            assert to[r] == names[idx[r, k]]
        assert np.array_equal(to_none[:, k], exp < 0.001)
    self_kept = int((idx == np.arange(len(names))[:, None]).any(axis=1).sum())
    print(f"rows whose own index survived the column-0 drop: {self_kept}")
    arrays = dict(idx=idx, sim=sim64.astype(np.float32), sim3=sim3, to_none=to_none,
                        meta=np.array(json.dumps({
                            "call": 'TFIDF(min_similarity=0, top_n=5, cosine_method="knn").match(names)',
                            "reference": "MaartenGr/PolyFuzz v0.4.3 (/root/reference), run by tests/golden/make_golden_headline.py",
                            "sklearn": sklearn.__version__, "numpy": np.__version__,
                            "wall_s": round(wall, 1), "cores": os.cpu_count(),
                            "rows_with_self_kept": self_kept})))
    # four consecutive row blocks (tests/helpers.py HEADLINE_GOLDEN_PARTS): each file stays well below 1 MiB
    parts = 4
    rows = -(-len(names) // parts)
    for p in range(parts):
        path = os.path.join(HERE, f"headline_knn_golden_{p}.npz")
        np.savez_compressed(path, **{k: (v[p * rows:(p + 1) * rows] if v.ndim else v) for k, v in arrays.items()})
        print(f"wrote headline_knn_golden_{p}.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
