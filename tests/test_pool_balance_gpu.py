"""The caching device allocator balances over every entry point: a call that has returned and whose handles are dropped leaves
exactly the bytes live that were live before it (pfz_pool_stats).  A leaked temporary raises the count call by call; a block
returned twice drives it below the baseline.

Protocol of every case: the call once as warm-up (blocks a context keeps, such as the scan state, are allocated here), every
handle dropped, gc.collect(), live_bytes read; then the same call twice more -- live_bytes must equal the warm-up reading
exactly, and the results of all three calls must be equal bit for bit."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def names():
    from polyfuzz_amd import datasets
    return datasets.load_company_names()[:21000]


@pytest.fixture(scope="module")
def titles():
    from polyfuzz_amd import datasets
    t = datasets.load_movie_titles()
    return t["Netflix"][:300], t["IMDB"][:500]


def _frame_arrays(df):
    return tuple(df[c].to_numpy() for c in df.columns if c != "From")


def _same(a, b):
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        if a.dtype == object:
            return a.tolist() == b.tolist()
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


def _balanced(ctx, case, run):
    """run(): the call under test with every handle a local of its own; returns what the call computed (arrays, or the text of
    the error a refused call raised)"""
    first = run()
    gc.collect()
    live0, _ = ctx.pool_stats()
    print(f"{case}: live after warm-up {live0} B")
    for rep in (1, 2):
        again = run()
        gc.collect()
        live, _ = ctx.pool_stats()
        print(f"{case}: live after repeat {rep} {live} B")
        assert live == live0, f"{case}: {live - live0:+d} bytes live after repeat {rep}"
        assert _same(first, again), f"{case}: repeat {rep} computed something else"


def _tfidf_match(from_list, to_list=None, top_n=3):
    from polyfuzz_amd.models import TFIDF

    def run():
        return _frame_arrays(TFIDF(top_n=top_n, min_similarity=0).match(from_list, to_list))
    return run


@pytest.mark.parametrize("no_lds_hist", [False, True])
def test_tfidf_match(ctx, names, monkeypatch, no_lds_hist):
    """K1 / K2 (document frequencies in LDS histograms, or global atomics), the index build, the row-major K3"""
    if no_lds_hist:
        monkeypatch.setenv("PFZ_NO_LDS_HIST", "1")
    _balanced(ctx, f"tfidf 3000 no_lds_hist={no_lds_hist}", _tfidf_match(names[:3000]))


@pytest.mark.parametrize("fail_alloc", [False, True])
def test_symmetric_self_match(ctx, names, monkeypatch, fail_alloc):
    """three 2048-row blocks, the smallest list the symmetric form takes: the session state is allocated, freed with the index --
    or (PFZ_K3_SYM_FAIL_ALLOC) given back at once, the index marked, the row-major kernel serving it"""
    monkeypatch.setenv("PFZ_K3_SYM", "1")
    if fail_alloc:
        monkeypatch.setenv("PFZ_K3_SYM_FAIL_ALLOC", "1")
    _balanced(ctx, f"symmetric 5000 fail_alloc={fail_alloc}", _tfidf_match(names[:5000]))


def test_deep_top_n(ctx, names):
    """the passes of a top-n beyond the kernel's own depth, and their three temporaries"""
    from polyfuzz_amd.models import TFIDF

    def run():      # (the device result as it is: a frame of 2 200 columns is not what this is about)
        return TFIDF(top_n=1100, min_similarity=0).match_device(names[:1500]).download()
    _balanced(ctx, "deep top-n 1500 x 1100", run)


def test_lockstep(ctx, names, monkeypatch):
    """the lock-step kernel works in the context's scratch: not pooled memory, nothing live after it"""
    monkeypatch.setenv("PFZ_K3_LOCKSTEP", "1")
    _balanced(ctx, "lockstep 1000 x 20000", _tfidf_match(names[:1000], names[1000:21000]))


@pytest.mark.parametrize("side_stream", [False, True])
def test_indel_argmax(ctx, titles, monkeypatch, side_stream):
    """K4: the to-side plan, the row lists of three word classes, the (row, part) records -- on one stream or two"""
    from polyfuzz_amd import _lib
    if side_stream:
        monkeypatch.setenv("PFZ_K4_SIDE_STREAM", "1")
    frm = titles[0] + ["a quiet place in the country, part two!!", "z" * 30 + " the very long title of a film nobody has ever seen, or will " + "y" * 9]
    assert [len(s) for s in frm[-2:]] == [40, 100]

    def run():
        f, t = _lib.DeviceStrings.upload(ctx, frm), _lib.DeviceStrings.upload(ctx, titles[1][:400])
        return _lib.indel_argmax(ctx, f, t)
    _balanced(ctx, f"indel 302 x 400 side_stream={side_stream}", run)


def test_fuzz_extract_one(ctx, titles):
    """K7: forms, plan, the word-class launches and the general kernel (a from-string of 41 tokens)"""
    from polyfuzz_amd import _lib
    frm = titles[0][:200] + ["the " * 40 + "end"]

    def run():
        return _lib.fuzz_extract_one(ctx, frm, titles[1], "WRatio")
    _balanced(ctx, "fuzz 201 x 500", run)


@pytest.mark.parametrize("compute_dtype", [None, "float16"])
def test_dense_panels(ctx, monkeypatch, compute_dtype):
    """K5: six score panels, their block maxima, the two streams; the 16-bit operands' rounding temporary"""
    from polyfuzz_amd import _lib
    monkeypatch.setenv("PFZ_K5_PANEL_ROWS", "128")
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal((700, 96), dtype=np.float32), rng.standard_normal((5000, 96), dtype=np.float32)

    def run():
        return _lib.dense_cossim_topn_host(ctx, a, b, 3, 0.0, compute_dtype=compute_dtype)
    _balanced(ctx, f"dense 700 x 5000 x 96 {compute_dtype}", run)


def test_linkage(ctx, names):
    """K6 on the device-resident result of the 3 000-name match"""
    from polyfuzz_amd import linkage
    from polyfuzz_amd.models import TFIDF
    unique = list(dict.fromkeys(names[:3000]))

    def run():
        res = TFIDF(top_n=3, min_similarity=0).match_device(unique)
        clusters, mapping, name_map = linkage.group_top1(res, unique, 0.75)
        return (sorted(mapping.items()), sorted(name_map.items()))
    _balanced(ctx, "linkage 3000", run)


def test_refused_fit(ctx):
    """strings of punctuation only: the fit raises "empty vocabulary" with its half-built vectoriser and n-gram caches in hand"""
    from polyfuzz_amd.models import TFIDF
    strings = ["!!!", "?? ..", "--- ---", "(*)"] * 50

    def run():
        try:
            TFIDF(clean_string=True, min_similarity=0).match(strings)
        except ValueError as e:
            return str(e)
        return "no error"
    assert "empty vocabulary" in run()
    _balanced(ctx, "refused fit", run)


def test_refused_skip_codes(ctx, titles):
    """a skip array that mixes both forms is refused after the to-side plan has been built"""
    from polyfuzz_amd import _lib
    skip = np.full(300, -1, np.int32)
    skip[3], skip[7] = 5, -4

    def run():
        f, t = _lib.DeviceStrings.upload(ctx, titles[0]), _lib.DeviceStrings.upload(ctx, titles[1][:400])
        try:
            _lib.indel_argmax(ctx, f, t, skip_idx=skip)
        except _lib.PfzError as e:
            return str(e)
        return "no error"
    assert "skip_idx mixes" in run()
    _balanced(ctx, "refused skip codes", run)
