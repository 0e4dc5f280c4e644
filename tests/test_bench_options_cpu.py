"""bench.py's command line and its --dump-outputs writer, on a box without a GPU: a plain run leaves every record beyond the
line's own timed steps to --full, and the outputs are written as float32 / float64 .npy files of at most 64 MB in all
(a fixed, seeded sample of the rows above that)."""
import os
import sys

import numpy as np
import pandas as pd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


def test_plain_run_leaves_the_other_records_to_full():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    assert a.no_cpu_baseline and a.no_match_wall and a.no_configs
    f = bench.parse(["--full"])
    assert f.full and not f.no_cpu_baseline and not f.no_match_wall and not f.no_configs
    g = bench.parse(["--full", "--no-configs", "--dump-outputs", "out"])
    assert g.no_configs and not g.no_cpu_baseline and g.dump_outputs == "out"


def test_frame_outputs_are_the_frames_columns_as_numbers():
    names = ["a", "b", "a", "c"]
    frame = pd.DataFrame({"From": names, "To": ["a", "c", "b", None], "Similarity": [1.0, 0.5, 0.25, 0.0],
                          "To_2": [None, "a", "a", "b"], "Similarity_2": [0.0, 0.125, 0.2, 0.1]})
    out = bench.frame_outputs(frame, names, 2)
    assert set(out) == {"to_index", "similarity"} and all(a.dtype == np.float64 for a in out.values())
    assert out["to_index"].tolist() == [[0, -1], [3, 0], [1, 0], [-1, 1]]        # the first occurrence of a To string
    assert out["similarity"].tolist() == [[1.0, 0.0], [0.5, 0.125], [0.25, 0.2], [0.0, 0.1]]


def test_topn_outputs_keep_the_score_precision():
    idx = np.array([[3, -1]], np.int32)
    o32 = bench.topn_outputs(idx, np.array([[0.5, 0.0]], np.float32))
    assert o32["index"].dtype == np.float64 and o32["score"].dtype == np.float32 and o32["index"].tolist() == [[3, -1]]
    assert bench.topn_outputs(idx[:, 0], np.array([7, 0], np.int64))["score"].dtype == np.float64


def test_write_outputs_whole_and_sampled(tmp_path, monkeypatch):
    rng = np.random.default_rng(1)
    arrays = {"similarity": rng.random((1000, 5)), "to_index": rng.integers(0, 1000, (1000, 5)).astype(np.float64)}
    bench.write_outputs(str(tmp_path / "whole"), arrays)
    assert sorted(os.listdir(tmp_path / "whole")) == ["similarity.npy", "to_index.npy"]
    for k, a in arrays.items():
        assert np.array_equal(np.load(tmp_path / "whole" / f"{k}.npy"), a)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 20_000)
    for d in ("s1", "s2"):
        bench.write_outputs(str(tmp_path / d), arrays)
    files = sorted(os.listdir(tmp_path / "s1"))
    assert files == ["rows.npy", "similarity.npy", "to_index.npy"]
    assert sum(os.path.getsize(tmp_path / "s1" / f) for f in files) <= 20_000 + 3 * 128      # (+ the .npy headers)
    rows = np.load(tmp_path / "s1" / "rows.npy")
    assert rows.dtype == np.float64 and len(rows) > 100 and np.all(np.diff(rows) > 0)
    for k, a in arrays.items():
        got = np.load(tmp_path / "s1" / f"{k}.npy")
        assert np.array_equal(got, a[rows.astype(np.int64)]) and np.array_equal(got, np.load(tmp_path / "s2" / f"{k}.npy"))
