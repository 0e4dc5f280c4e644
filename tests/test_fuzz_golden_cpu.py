"""tests/golden/c3_fuzz_oracle_*.npz (make_golden_c3_fuzz.py) is what the committed oracle says NOW: the GPU suite holds K7 to these
files on every row of the 20 000 x 20 000 configuration, so a change to oracle/fuzz_scorers.c / indel.c that moves a value must
turn this module red until the fixture is regenerated.  No GPU needed."""
import concurrent.futures as cf

import numpy as np
import pytest

from tests import helpers

SLOW = ("WRatio", "partial_ratio", "partial_token_ratio", "partial_token_set_ratio", "partial_token_sort_ratio")   # > 0.2 s per row


def test_the_ten_scorers_and_their_row_counts():
    from oracle import native
    assert set(helpers.C3_FUZZ_SCORERS) == set(native.FUZZ_SCORER_IDS) and len(helpers.C3_FUZZ_SCORERS) == 10
    full = [s for s, stride in helpers.C3_FUZZ_SCORERS.items() if stride == 1]
    assert len(full) == 7 and sorted(set(helpers.C3_FUZZ_SCORERS) - set(full)) == [
        "partial_token_ratio", "partial_token_set_ratio", "partial_token_sort_ratio"]
    for scorer, stride in helpers.C3_FUZZ_SCORERS.items():
        rows, idx, score = helpers.load_c3_fuzz_golden(scorer)
        assert len(rows) == (20_000 if stride == 1 else 2_000) and rows[0] == 0 and (np.diff(rows) == stride).all()
        assert ((idx >= 0) & (idx < 20_000)).all() and ((score >= 0) & (score <= 100)).all()


def test_the_lists_are_the_ones_the_fixture_was_made_on():
    import os
    fl, tl = helpers.c3_fuzz_lists()
    digest = helpers.lists_sha256(fl, tl)
    for scorer in helpers.C3_FUZZ_SCORERS:
        path = helpers.c3_fuzz_golden_path(scorer)
        assert os.path.getsize(path) < (1 << 20), path
        assert str(np.load(path)["lists_sha256"]) == digest, scorer


@pytest.mark.parametrize("scorer", sorted(helpers.C3_FUZZ_SCORERS))
def test_a_seeded_sample_recomputed_live(oracle_mod, scorer):
    """16 fixture rows of the scorers above 0.2 s per row, 128 of the cheap ones, through oracle.fuzz_extract_one against the
    whole to-list: index and score bit for bit (about 15 s on eight cores for all ten)."""
    fl, tl = helpers.c3_fuzz_lists()
    rows, idx, score = helpers.load_c3_fuzz_golden(scorer)
    n = 16 if scorer in SLOW else 128
    pick = np.sort(np.random.default_rng(sorted(helpers.C3_FUZZ_SCORERS).index(scorer)).choice(len(rows), n, replace=False))

    def one(k):
        i = int(rows[k])
        return oracle_mod.fuzz_extract_one(fl, tl, scorer, rows=(i, i + 1))
    with cf.ThreadPoolExecutor(8) as ex:
        parts = list(ex.map(one, pick))
    np.testing.assert_array_equal(np.concatenate([p[1] for p in parts]), score[pick], err_msg=scorer)
    np.testing.assert_array_equal(np.concatenate([p[0] for p in parts]), idx[pick], err_msg=scorer)
