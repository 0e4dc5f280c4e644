"""tests/golden/c3_jaro_oracle_*.npz (make_golden_c3_jaro.py) is what the committed oracle says NOW: the GPU suite holds K8 to these
files on every row of the 20 000 x 20 000 titles, so a change to oracle/jaro.c that moves a value must turn this module red until the
fixture is regenerated.  No GPU needed."""
import os

import numpy as np
import pytest

from tests import helpers


def test_the_lists_are_the_ones_the_fixture_was_made_on():
    fl, tl = helpers.c3_fuzz_lists()
    digest = helpers.lists_sha256(fl, tl)
    for scorer in helpers.JARO_SCORERS:
        path = helpers.c3_jaro_golden_path(scorer)
        assert os.path.getsize(path) < (1 << 20), path
        assert str(np.load(path)["lists_sha256"]) == digest, scorer
        idx, score = helpers.load_c3_jaro_golden(scorer)
        assert ((idx >= 0) & (idx < 20_000)).all() and ((score > 0) & (score <= 1)).all()
    j, w = (helpers.load_c3_jaro_golden(s)[1] for s in helpers.JARO_SCORERS)
    assert (w >= j).all() and (w > j).any()              # (Winkler's step only adds; a row's best under it is no lower)


@pytest.mark.parametrize("scorer", helpers.JARO_SCORERS)
def test_a_seeded_sample_recomputed_live(oracle_mod, scorer):
    """128 seeded fixture rows through oracle.jaro_argmax against the whole to-list: index and score bit for bit"""
    fl, tl = helpers.c3_fuzz_lists()
    idx, score = helpers.load_c3_jaro_golden(scorer)
    pick = np.sort(np.random.default_rng(helpers.JARO_SCORERS.index(scorer)).choice(len(idx), 128, replace=False))
    sample = [fl[i] for i in pick]
    e_idx, e_score = helpers.jaro_oracle_argmax(oracle_mod, sample, tl, scorer)
    np.testing.assert_array_equal(e_score, score[pick], err_msg=scorer)
    np.testing.assert_array_equal(e_idx, idx[pick], err_msg=scorer)
