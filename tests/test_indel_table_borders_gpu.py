"""K4 at the alphabet sizes where a word class's match table stops fitting LDS.  pfz_indel's dispatch sends a class of from-strings
to the general kernel when (symbols + 1) x its word bytes exceed 60 KiB -- at 480, 960, 1 920, 3 840, 7 680 and 15 360 symbols for
the classes of 128 down to 4 bytes per symbol -- and the quad / octo kernels (16 bytes per symbol) stop at 3 840.  One symbol below
and at every border: matrix, arg-max (host and device entry, with and without a skip list) and top-n == oracle/indel.c bit for
bit, and the profile counters show the rows on the side of the border the rule restated in tests/second_row_cases.py puts them.
The to-lists hold thousands of 16-bit symbols: the general kernels' 16-bit forms and the multi-word classes with 16-bit symbols."""
import numpy as np
import pytest

from tests import lev_oracle
from tests import second_row_cases as sc
from tests.test_edit_topn_gpu import _assert_topn, expected_topn
from tests.test_second_row_gpu import _k4_dev_argmax, _profile

pytestmark = pytest.mark.gpu

K4_COUNTS = ("k4_indel", "k4_indel_general", "k4_general_rows", "k4_quad_launches")


@pytest.mark.parametrize("n_sym", sc.K4_BORDERS)
def test_k4_at_a_table_size_border(ctx, oracle_mod, n_sym):
    from polyfuzz_amd import _lib
    fl, tl, hot = sc.border_lists(n_sym)
    n, n_to = len(fl), len(tl)
    lengths = [len(s) for s in fl]
    assert len(set("".join(tl))) == n_sym and lengths == [m for m in sc.BORDER_FROM_LENGTHS for _ in range(2)]
    e_idx, e_score, mat = oracle_mod.indel_argmax(fl, tl, want_matrix=True)
    assert (mat != 0).mean() > 0.5, (mat != 0).mean()
    general, quad = sc.k4_general_rows(lengths, n_sym), sc.k4_quad_launches(lengths, n_sym)
    assert general >= 2 and (quad == 2) == (n_sym <= 3839)                       # (the two strings of 1 025 characters always)
    f, t = _lib.DeviceStrings.upload(ctx, fl), _lib.DeviceStrings.upload(ctx, tl)
    assert _lib.indel_plan_info(ctx, t)["n_symbols"] == n_sym

    with _profile(ctx, *K4_COUNTS) as box:
        got = _lib.indel_matrix(ctx, f, t)
    assert box == {"k4_indel": 1, "k4_indel_general": 1, "k4_general_rows": general, "k4_quad_launches": 0}, box     # (no quad with a matrix)
    np.testing.assert_array_equal(got, mat)

    skip = e_idx.copy()                      # the row's own best left out, nothing for every fifth row
    skip[::5] = -1
    for what, sk in (("no skip", None), ("one choice", skip)):
        w_idx, w_score = lev_oracle.argmax(mat, sk)
        with _profile(ctx, *K4_COUNTS) as box:
            idx, score = _lib.indel_argmax(ctx, f, t, sk)
            d_idx, d_score = _k4_dev_argmax(ctx, f, t, n, sk)
        assert box == {"k4_indel": 2, "k4_indel_general": 2, "k4_general_rows": 2 * general, "k4_quad_launches": 2 * quad}, (what, box)
        np.testing.assert_array_equal(idx, w_idx, err_msg=what)
        np.testing.assert_array_equal(score, w_score, err_msg=what)
        np.testing.assert_array_equal(d_idx, w_idx, err_msg=f"{what} (device entry)")
        np.testing.assert_array_equal(d_score, w_score, err_msg=f"{what} (device entry)")
    np.testing.assert_array_equal(lev_oracle.argmax(mat)[0], e_idx)
    np.testing.assert_array_equal(lev_oracle.argmax(mat)[1], e_score)

    with _profile(ctx, *K4_COUNTS) as box:
        top = _lib.indel_topn(ctx, f, t, 3, skip)
    assert box == {"k4_indel": 1, "k4_indel_general": 1, "k4_general_rows": general, "k4_quad_launches": 0}, box     # (no quad with ntop)
    _assert_topn(top, expected_topn(mat, 3, skip), n_sym)
