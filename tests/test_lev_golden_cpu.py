"""tests/golden/c3_lev_oracle.npz (make_golden_c3_lev.py) is what the committed oracle says NOW: the GPU suite holds K9 to this file
on 2 000 rows of the 20 000 x 20 000 titles, so a change to tests/lev_oracle.py that moves a value must turn this module red until
the fixture is regenerated.  No GPU needed."""
import importlib.util
import os

import numpy as np
import pytest

from tests import lev_oracle

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def maker():
    spec = importlib.util.spec_from_file_location("make_golden_c3_lev", os.path.join(HERE, "golden", "make_golden_c3_lev.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_lists_are_the_ones_the_fixture_was_made_on(maker):
    fl, tl = maker.lists()
    assert os.path.getsize(maker.PATH) < (1 << 20)
    g = np.load(maker.PATH)
    assert str(g["lists_sha256"]) == maker.lists_sha256(fl, tl) and str(g["source"]) == "oracle" and int(g["seed"]) == maker.SEED
    rows = g["rows"]
    assert rows.dtype == np.int32 and len(rows) == 2000 and (np.diff(rows) > 0).all() and rows[0] >= 0 and rows[-1] < 20_000
    np.testing.assert_array_equal(rows, np.sort(np.random.default_rng(maker.SEED).choice(len(fl), maker.N_ROWS, replace=False)))
    la = lev_oracle.lengths(fl)[rows]
    for scorer in lev_oracle.SCORERS:
        idx, d, m = (g[f"{k}_{scorer}"] for k in ("idx", "distance", "M"))
        assert idx.dtype == d.dtype == m.dtype == np.int32 and ((idx >= 0) & (idx < 20_000)).all()
        np.testing.assert_array_equal(m, np.maximum(la, lev_oracle.lengths(tl)[idx]))
        assert ((d >= 0) & (d <= m)).all() and (m > 0).all()
    sim = {s: lev_oracle.similarity(g[f"distance_{s}"], g[f"M_{s}"], g[f"M_{s}"]) for s in lev_oracle.SCORERS}
    assert (sim["osa"] >= sim["levenshtein"]).all() and (sim["osa"] > sim["levenshtein"]).any()      # (OSA's d is no larger)


@pytest.mark.parametrize("scorer", lev_oracle.SCORERS)
def test_a_seeded_sample_recomputed_live(maker, scorer):
    """20 seeded fixture rows through the oracle against the whole to-list: index, distance and M"""
    fl, tl = maker.lists()
    g = np.load(maker.PATH)
    pick = np.sort(np.random.default_rng(lev_oracle.SCORERS.index(scorer)).choice(2000, 20, replace=False))
    idx, d, m = maker.best_rows([fl[i] for i in g["rows"][pick]], tl, scorer)
    np.testing.assert_array_equal(idx, g[f"idx_{scorer}"][pick], err_msg=scorer)
    np.testing.assert_array_equal(d, g[f"distance_{scorer}"][pick], err_msg=scorer)
    np.testing.assert_array_equal(m, g[f"M_{scorer}"][pick], err_msg=scorer)
