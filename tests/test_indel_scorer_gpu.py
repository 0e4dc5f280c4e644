"""EditDistance(scorer="indel") on the GPU: match, top_n and the join frame against the definition (tests/indel_oracle.py).  The
indices are np.argsort(-sim, kind="stable") of the oracle's float64 scores, the scores are the oracle's float64, and the indices
are also what EditDistance(scorer="ratio") returns on the same lists.  Every comparison is exact."""
import numpy as np
import pandas as pd
import pytest

from tests import indel_oracle
from tests.test_edit_topn_gpu import RATIO_FROM_LENGTHS, _assert_frame, _want_frame, expected_topn
from tests.test_join_gpu import _edited, _rand
from tests.test_levenshtein_gpu import _first_occurrence

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lists():
    """the shapes of tests/test_edit_topn_gpu.py's ratio_lists: from-lengths on both sides of every border of K4's word classes
    against ~200 to-strings, every one twice (the index decides); narrow, and 16-bit symbols"""
    rng = np.random.default_rng(141)
    alpha = "abcdefgh "
    mk = lambda n, a=alpha: "".join(a[i] for i in rng.integers(0, len(a), n))
    fl = [mk(n) for n in RATIO_FROM_LENGTHS] + [mk(int(n)) for n in rng.integers(2, 40, 14)]
    uniq = [mk(int(n)) for n in [0, 1, 3, 17, 32, 64, 100, 130, 300, 600, 1500] + list(rng.integers(1, 40, 89))]
    tl = uniq + uniq[::-1]
    wide = "".join(chr(c) for c in list(range(0x4E00, 0x4E00 + 400)) + list(range(0x41, 0x5B)))
    uniq16 = [mk(int(n), wide) for n in rng.integers(0, 50, 75)] + [mk(n, wide) for n in (33, 70, 130)] + [""]
    fl16 = [mk(n, wide) for n in (0, 1, 16, 17, 32, 33, 64, 65, 128, 129)] + uniq16[:6]
    tl16 = uniq16 + uniq16[::-1]
    assert len(set("".join(tl16))) > 255
    out = {}
    for which, (a, b) in (("narrow", (fl, tl)), ("wide", (fl16, tl16))):
        dup = b[:40] + a[:8] + b[:12] + ["", ""]
        out[which] = (a, b, indel_oracle.sim_matrix(a, b, indel_oracle.lcs_matrix(a, b)), dup,
                      indel_oracle.sim_matrix(dup, dup, indel_oracle.lcs_matrix(dup, dup)))
    return out


@pytest.mark.parametrize("which", ("narrow", "wide"))
def test_match_and_top_n(ctx, lists, which):
    """match (top 1; two lists and the self-match; normalize on and off) and top_n = 1, 5, 64"""
    from polyfuzz_amd.models import EditDistance
    fl, tl, sim, dup, dup_sim = lists[which]
    assert sim.min() == 0.0 and sim.max() == 1.0 and sim[fl.index(""), tl.index("")] == 1.0
    for ntop in (1, 5, 64):
        for normalize in (False, True):
            m = EditDistance(scorer="indel", normalize=normalize)
            m.top_n = ntop
            _assert_frame(m.match(fl, tl), _want_frame(fl, tl, *expected_topn(sim, ntop), normalize))
            k = min(ntop, len(dup) - 1)
            _assert_frame(m.match(dup), _want_frame(dup, dup, *expected_topn(dup_sim, k, _first_occurrence(dup)), normalize))
        r = EditDistance(scorer="ratio", normalize=False)
        r.top_n = ntop
        got, ratio = m.match(fl, tl), r.match(fl, tl)
        for c in got.columns:
            if not c.startswith("Similarity"):
                assert got[c].tolist() == ratio[c].tolist(), c          # K4's order IS this scorer's
        got, ratio = m.match(dup), r.match(dup)
        assert got["To"].tolist() == ratio["To"].tolist()
    plain = EditDistance(scorer="indel", normalize=False).match(fl, tl)
    assert list(plain.columns) == ["From", "To", "Similarity"] and plain["Similarity"].dtype == np.float64
    assert plain["Similarity"].max() == 1.0 and plain["Similarity"].min() >= 0.0          # the 0..1 scale, not 0..100


def test_join_frames_and_single_linkage(ctx):
    """EditDistance(scorer="indel").join: the frame From, To, Similarity == the oracle's pairs in (from-index, to-index) order,
    unrounded and NOT normalised whatever `normalize` says; the self-join form; and the frame goes through single_linkage"""
    from polyfuzz_amd.linkage import single_linkage
    from polyfuzz_amd.models import EditDistance
    rng = np.random.default_rng(115)
    tl = ["acme holdings ltd", "acme holding ltd", "acme holdings ltd.", "globex corp", "globex corporation", "initech", "", "umbrella"] + \
        _rand(rng, "abcdefgh ", 5, 40, 60)
    fl = ["acme holdings ltd", "globex corp.", "initech", "", "zzzz"] + [_edited(rng, s, "abcdefgh ", 2) for s in tl[8:40]]

    def frame(a, b, thr, self_join=False):
        sim = indel_oracle.sim_matrix(a, b, indel_oracle.lcs_matrix(a, b))
        keep = sim >= thr
        if self_join:
            keep &= np.triu(np.ones(keep.shape, bool), 1)
        i, j = np.nonzero(keep)
        return pd.DataFrame({"From": [a[k] for k in i], "To": [b[k] for k in j], "Similarity": sim[i, j]})

    for normalize in (True, False):
        for thr in (0.8, 0.5, 1.0):
            got = EditDistance(scorer="indel", normalize=normalize).join(fl, tl, thr)
            assert list(got.columns) == ["From", "To", "Similarity"] and got["Similarity"].dtype == np.float64
            pd.testing.assert_frame_equal(got, frame(fl, tl, thr), check_exact=True)
    assert "zzzz" not in set(EditDistance(scorer="indel").join(fl, tl, 0.5)["From"])          # no partner: no row
    exact = EditDistance(scorer="indel").join(fl, tl, 1.0)
    assert ("", "") in set(zip(exact["From"], exact["To"])) and (exact["Similarity"] == 1.0).all()      # '' against '': 1.0, a hit at t = 1
    # default threshold, self-join
    got = EditDistance(scorer="indel").join(tl)
    pd.testing.assert_frame_equal(got, frame(tl, tl, 0.8, self_join=True), check_exact=True)
    clusters, mapping, names = single_linkage(got, 0.85)
    acme = {"acme holdings ltd", "acme holding ltd", "acme holdings ltd."}
    assert len({mapping[s] for s in acme}) == 1 and acme <= set(clusters[mapping["acme holdings ltd"]])
