"""K22 on the GPU: pfz_dense_join16 / pfz_dense_components16 (Embeddings.join / .components with search_dtype set).  The plain
16-bit join against pfz_dense_topn on the same 16-bit handles and the rescored join against pfz_dense_rescore_topn over every
column, pairs and float32 score BITS equal; the float64 cosines; a pair that only the margin finds; the components; the
accumulation term of the margin, measured; the candidate buffer's repeat; a call cut into two launches; the pool fill."""
import ctypes
import functools

import numpy as np
import pytest

from tests import dense_join16_cases as C
from tests import dense_join_cases as DJ

pytestmark = pytest.mark.gpu
T = 0.8

# name -> (n_a, n_b or None for a self-join, width).  Why each is there:
#   two lists 300 x 513: two row tiles of 256, the second with 44 rows; three column tiles, the last with ONE row.  Width 64 is one
#     k-chunk (the pipeline re-fetches chunk 0), width 100 is padded to 128.
#   self-join of 600: 3 x 3 tiles, 6 launched; widths 64, 128 and 192 (one, two and three chunks: the loop's first steady state).
CASES = {"300x513x64": (300, 513, 64), "300x513x100": (300, 513, 100), "600x64": (600, None, 64), "600x128": (600, None, 128),
         "600x192": (600, None, 192)}
# planted near-copies (row, column): across the tile edge 255 | 256 both ways, in the last row and the last column, and -- the
# self-join -- inside the diagonal tile (1, 1), whose mirror image (500, 270) lies in the same tile below the diagonal
# (rows 598 and 599 are both copies of row 10, so (598, 599) is a pair too)
PLANTED = {False: ((255, 256), (256, 255), (299, 512), (299, 0), (0, 511)), True: ((255, 256), (10, 599), (10, 598), (270, 500), (3, 4))}


@functools.lru_cache(maxsize=None)
def _lists(name):
    n_a, n_b, d = CASES[name]
    rng = np.random.default_rng(len(name) + d)
    x = DJ.gen(n_a, d, 24, 220 + d)
    y = None if n_b is None else np.ascontiguousarray(DJ.gen(n_b, d, 24, 220 + d)[::-1])      # (the same cluster centres, other rows)
    for i, j in PLANTED[n_b is None]:
        (x if y is None else y)[j] = x[i] + 0.02 * rng.standard_normal(d).astype(np.float32)
    x.setflags(write=False)
    if y is not None:
        y.setflags(write=False)
    return x, y


_cache = {}


def _devs(ctx, name, dtype):
    """(from32, to32 or None, from16, to16 or None), resident"""
    from polyfuzz_amd import _lib
    if ("dev", name, dtype) not in _cache:
        if ("dev32", name) not in _cache:
            x, y = _lists(name)
            _cache["dev32", name] = (_lib.DeviceDense.upload(ctx, x), None if y is None else _lib.DeviceDense.upload(ctx, y))
        f, t = _cache["dev32", name]
        _cache["dev", name, dtype] = (f, t, f.derive16(dtype), None if t is None else t.derive16(dtype))
    return _cache["dev", name, dtype]


def _rescored(ctx, name, dtype):
    """the rescored join of a case at T (computed once): (rows, cols, scores, row_ptr, counts)"""
    from polyfuzz_amd import _lib
    if ("join", name, dtype) not in _cache:
        f, t, f16, t16 = _devs(ctx, name, dtype)
        row_ptr, idx, sim, counts = _lib.dense_join16(ctx, f16, t16, f, t, T, counters=True)
        _cache["join", name, dtype] = DJ.csr_pairs(row_ptr, idx) + (sim, row_ptr, counts)
    return _cache["join", name, dtype]


def _assert_same_pairs(got, want, what):
    (rows, cols, sim), (e_rows, e_cols, e_val) = got, want
    assert len(rows) == len(e_rows), (what, len(rows), len(e_rows))
    np.testing.assert_array_equal(rows, e_rows, err_msg=what)
    np.testing.assert_array_equal(cols, e_cols, err_msg=what)
    np.testing.assert_array_equal(sim.view(np.uint32), e_val.view(np.uint32), err_msg=what)


def _raw_join16(ctx, f16, t16, f, t, thr, cap, n, cand_cap=0):
    """pfz_dense_join16 itself, into buffers pre-filled with -7 and one guard word longer than they need be"""
    row_ptr, idx, sim = np.full(n + 2, -7, np.int64), np.full(cap + 1, -7, np.int32), np.full(cap + 1, -7.0, np.float32)
    total, work = ctypes.c_int64(-7), np.full(3, -7, np.int64)
    h = [None if d is None else d.h for d in (t16, f, t)]
    rc = ctx.lib.pfz_dense_join16(ctx.h, f16.h, h[0], h[1], h[2], float(thr), cap, cand_cap, row_ptr.ctypes.data, idx.ctypes.data,
                                  sim.ctypes.data, ctypes.byref(total), work.ctypes.data)
    return rc, total.value, row_ptr, idx, sim, work


# ---- 1. the plain 16-bit join ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("name", list(CASES))
def test_plain_join_equals_the_16_bit_topn_bit_for_bit(ctx, name, dtype):
    """from_exact=None: pairs and score bits == dense_topn on the same 16-bit handles with ntop = all columns and the bound just
    below t32; capacity 0 returns the exact total and writes nothing, and the repeat fills"""
    from polyfuzz_amd import _lib
    _, _, f16, t16 = _devs(ctx, name, dtype)
    row_ptr, idx, sim, counts = _lib.dense_join16(ctx, f16, t16, None, None, T, counters=True)
    rows, cols = DJ.csr_pairs(row_ptr, idx)
    want = DJ.existing_path(ctx, f16, t16, T)
    assert len(want[0]) > 50 and sim.dtype == np.float32
    _assert_same_pairs((rows, cols, sim), want, f"{name} {dtype}")
    got = set(zip(rows.tolist(), cols.tolist()))
    assert all(p in got for p in PLANTED[t16 is None])
    if t16 is None:
        assert (cols > rows).all()
    tiles = lambda n: -(-n // 256)
    n_b = f16.n if t16 is None else t16.n
    assert counts["tiles"] == (tiles(f16.n) * (tiles(f16.n) + 1) // 2 if t16 is None else tiles(f16.n) * tiles(n_b))
    assert counts["candidates"] == counts["pairs"] == len(rows) and 1 <= counts["hit_corners"] <= 16 * counts["tiles"]
    rc, total, r_ptr, r_idx, r_sim, _ = _raw_join16(ctx, f16, t16, None, None, T, 0, f16.n)
    assert rc == 0 and total == len(rows)
    assert (r_ptr == -7).all() and (r_idx == -7).all() and (r_sim == -7.0).all()
    b_ptr, b_idx, b_sim, b_counts = _lib.dense_join16(ctx, f16, t16, None, None, T, capacity=0)
    assert b_counts == {"pairs": len(rows), "candidates": len(rows)}
    assert b_ptr.tobytes() == row_ptr.tobytes() and b_idx.tobytes() == idx.tobytes() and b_sim.tobytes() == sim.tobytes()


# ---- 2. the rescored join --------------------------------------------------------------------------------------------------------

def _rescore_reference(ctx, f, t, thr):
    """dense_rescore over EVERY column, thresholded at t32 on the host: (rows, cols, scores) by row, then column"""
    from polyfuzz_amd import _lib
    self_join = t is None
    t = f if self_join else t
    assert t.n <= 1024
    cand = _lib.DeviceTopN.from_host(ctx, np.tile(np.arange(t.n, dtype=np.int32), (f.n, 1)), np.zeros((f.n, t.n), np.float32))
    idx, val = _lib.dense_rescore(ctx, f, t, cand, t.n, 0.0).download()
    rows, slot = np.nonzero((idx >= 0) & (val >= _lib.dense_threshold32(thr)))
    cols, vals = idx[rows, slot], val[rows, slot]
    if self_join:
        keep = cols > rows
        rows, cols, vals = rows[keep], cols[keep], vals[keep]
    order = np.lexsort((cols, rows))
    return rows[order], cols[order], vals[order]


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("name", list(CASES))
def test_rescored_join_equals_the_exact_rescoring_and_the_float64_oracle(ctx, oracle_mod, name, dtype):
    """pairs and score bits == dense_rescore over every column, thresholded at t32 on the host; against the float64 cosine the
    same pair set outside a 1e-5 band around t (K14's own rule); the capacity contract on the final hits"""
    from polyfuzz_amd import _lib
    f, t, f16, t16 = _devs(ctx, name, dtype)
    rows, cols, sim, row_ptr, counts = _rescored(ctx, name, dtype)
    assert sim.dtype == np.float32 and row_ptr[0] == 0 and row_ptr[-1] == len(cols) and len(row_ptr) == f.n + 1
    _assert_same_pairs((rows, cols, sim), _rescore_reference(ctx, f, t, T), f"{name} {dtype}")
    same_row = rows[1:] == rows[:-1]
    assert (np.diff(row_ptr) >= 0).all() and (cols[1:][same_row] > cols[:-1][same_row]).all()
    x, y = _lists(name)
    cos = oracle_mod.dense.dense_cossim(x, x if y is None else y)
    if y is None:
        cos[np.tril_indices(len(x))] = -np.inf
    found = np.zeros(cos.shape, bool)
    found[rows, cols] = True
    band = int((np.abs(cos - T) < DJ.BAND).sum())
    print(f"{name} {dtype}: {len(rows)} hits of {counts['candidates']} candidates, oracle {int((cos >= T).sum())} (band {band}), "
          f"max |score - cosine| {np.abs(sim - cos[rows, cols]).max():.3g}")
    assert found[cos >= T + DJ.BAND].all() and not found[cos < T - DJ.BAND].any()
    assert np.abs(sim.astype(np.float64) - cos[rows, cols]).max() <= DJ.BAND
    assert all(found[p] for p in PLANTED[y is None])
    assert counts["pairs"] == len(rows) > 50 and counts["candidates"] >= len(rows)
    # the search compares with ts32 = the largest float32 <= t - eps: the candidates are the plain 16-bit join's hits at that value
    ts32 = _lib.dense_search_threshold32(T, _lib.dense_search_margin(dtype, C.padded(x.shape[1])))
    assert np.float64(ts32) < T - C.rounding_term(dtype, C.padded(x.shape[1]))
    at_ts32 = _lib.dense_join16(ctx, f16, t16, None, None, float(ts32))[3]["pairs"]
    assert counts["candidates"] == at_ts32
    total = len(rows)
    rc, got, r_ptr, r_idx, r_sim, work = _raw_join16(ctx, f16, t16, f, t, T, total - 1, f.n)
    assert rc == 0 and got == total and (r_ptr == -7).all() and (r_idx == -7).all() and (r_sim == -7.0).all()
    assert work.tolist() == [counts["tiles"], counts["hit_corners"], counts["candidates"]]
    rc, got, r_ptr, r_idx, r_sim, _ = _raw_join16(ctx, f16, t16, f, t, T, total, f.n)
    assert rc == 0 and got == total and r_ptr[f.n + 1] == -7 and r_idx[total] == -7 and r_sim[total] == -7.0
    assert r_ptr[:f.n + 1].tobytes() == row_ptr.tobytes() and r_idx[:total].tobytes() == cols.astype(np.int32).tobytes()
    assert r_sim[:total].tobytes() == sim.tobytes()


def test_wrong_handles_are_invalid(ctx):
    from polyfuzz_amd import _lib
    x, _ = _lists("600x64")
    f, _, f16, _ = _devs(ctx, "600x64", "float16")
    other = _lib.DeviceDense.upload(ctx, x[:100])
    raw = _lib.DeviceDense.upload(ctx, x, normalize=False)
    i8 = _lib.DeviceDense.upload_int8(ctx, x)
    for args in ((f, None, f, None), (i8, None, f, None), (f16, None, f16, None), (f16, None, other, None), (f16, None, raw, None),
                 (f16, None, f, other), (f16, None, None, f)):
        rc, *_ = _raw_join16(ctx, args[0], args[1], args[2], args[3], T, 0, 600)
        assert rc == -1, args                                  # PFZ_ERR_INVALID
    # two copies derived from ONE fp32 handle are two lists like any other: the self-join's pairs both ways round, and (i, i)
    g16 = f.derive16("float16")
    rc, total, *_ = _raw_join16(ctx, f16, g16, f, f, T, 0, 600)
    assert rc == 0 and total == 2 * len(_rescored(ctx, "600x64", "float16")[0]) + 600
    with pytest.raises(ValueError, match="fp32"):
        f16.derive16("float16")
    with pytest.raises(ValueError, match="search types"):
        f.derive16("int8")


# ---- 3. the case the margin exists for -------------------------------------------------------------------------------------------

# the rows a pair losing more than 2e-4 is looked for in: bfloat16 loses that on plain Gaussian rows of width 64; float16's worst pair
# there loses 1.5e-4, so its rows are Gaussian with column k scaled by 0.7^k (a few columns carry the cosine: 5.6e-4)
MARGIN_ROWS = {"bfloat16": lambda: C.gaussian_rows(400, 64, 33), "float16": lambda: C.decaying_rows(400, 64, 33)}


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_a_pair_only_the_margin_finds(ctx, dtype):
    """A pair whose float64 cosine exceeds the cosine of its rounded copies by more than 2e-4, t = its float64 cosine - 1e-5: it is
    in the rescored join and absent from the plain 16-bit join at the same t."""
    from polyfuzz_amd import _lib
    x = MARGIN_ROWS[dtype]()
    exact = C.cosines64(x, x)
    r = C.search_copy(x, dtype)
    loss = exact - C.cosines64(r, r)
    loss[np.tril_indices(len(x))] = -np.inf
    loss[exact <= 0.05] = -np.inf                              # (a threshold in [0, 1], and a candidate well inside it)
    i, j = np.unravel_index(np.argmax(loss), loss.shape)
    assert loss[i, j] > 2e-4, loss[i, j]
    t = exact[i, j] - 1e-5
    f = _lib.DeviceDense.upload(ctx, x)
    f16 = f.derive16(dtype)
    rows, cols = DJ.csr_pairs(*_lib.dense_join16(ctx, f16, None, f, None, t)[:2])
    assert (i, j) in set(zip(rows.tolist(), cols.tolist()))
    p_rows, p_cols = DJ.csr_pairs(*_lib.dense_join16(ctx, f16, None, None, None, t)[:2])
    assert (i, j) not in set(zip(p_rows.tolist(), p_cols.tolist()))
    print(f"{dtype} pair ({i}, {j}): cosine {exact[i, j]:.6f}, of the rounded copies {exact[i, j] - loss[i, j]:.6f}; rescored join {len(rows)} pairs, "
          f"plain {len(p_rows)}")


# ---- 4. components and the matcher ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("name", ["600x64", "600x192"])
def test_components_and_the_matcher(ctx, name, dtype):
    from polyfuzz_amd import _lib, linkage
    from polyfuzz_amd.models import Embeddings
    f, _, f16, _ = _devs(ctx, name, dtype)
    rows, cols, sim, row_ptr, counts = _rescored(ctx, name, dtype)
    want = DJ.union_find_labels(f.n, rows, cols)
    label, pairs, components, work = _lib.dense_components16(ctx, f16, f, T, counters=True)
    assert label.dtype == np.int32 and label.tobytes() == want.tobytes()
    assert (pairs, components) == (len(rows), len(np.unique(want))) and 1 < components < f.n
    assert work == {k: counts[k] for k in _lib.DENSE_JOIN16_COUNTERS}
    x, _ = _lists(name)
    names = [f"s{i}" for i in range(len(x))]
    m = Embeddings()
    m.search_dtype = dtype
    frame = m.join(names, min_similarity=T, embeddings_from=x)
    assert list(frame.columns) == ["From", "To", "Similarity"] and m.last_counts == {"pairs": len(rows), "candidates": counts["candidates"]}
    assert frame["From"].tolist() == [names[i] for i in rows] and frame["To"].tolist() == [names[j] for j in cols]
    assert frame["Similarity"].to_numpy().tobytes() == sim.tobytes()
    got = m.components(names, T, embeddings=x)
    assert got.tobytes() == want.tobytes()
    assert m.last_counts == {"pairs": len(rows), "components": components, "candidates": counts["candidates"]}
    assert linkage.connected_components(names, m, T, embeddings=x) == linkage.dicts_from_labels(names, want)


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_two_lists_through_the_matcher(ctx, dtype):
    from polyfuzz_amd.models import Embeddings
    rows, cols, sim, _, _ = _rescored(ctx, "300x513x100", dtype)
    x, y = _lists("300x513x100")
    a, b = [f"a{i}" for i in range(len(x))], [f"b{i}" for i in range(len(y))]
    m = Embeddings()
    m.search_dtype = dtype
    frame = m.join(a, b, T, embeddings_from=x, embeddings_to=y)
    assert frame["From"].tolist() == [a[i] for i in rows] and frame["To"].tolist() == [b[j] for j in cols]
    assert frame["Similarity"].to_numpy().tobytes() == sim.tobytes()


# ---- 5. the accumulation term, measured --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", C.DTYPES)
def test_accumulation_term_holds_at_width_4096(ctx, dtype):
    """max |plain 16-bit score - float64 cosine of the rounded vectors| <= (ld + 8) 2^-23 at width 4096, 256 x 256 rows: the
    second term of the margin is an assumption about the matrix core's fp32 accumulation, and this is where it is held.  The
    16-bit values are made on the host (the emulated search copy) and uploaded as they are, so the float64 cosine is that of
    exactly the values the device multiplies; rows of |Gaussian| values, so that every pair is a hit at t = 0."""
    from polyfuzz_amd import _lib
    d = 4096
    rng = np.random.default_rng(4096)
    ra = C.search_copy(np.abs(rng.standard_normal((256, d))).astype(np.float32), dtype)
    rb = C.search_copy(np.abs(rng.standard_normal((256, d))).astype(np.float32), dtype)
    as_given = (lambda r: r.astype(np.float16)) if dtype == "float16" else (lambda r: (r.view(np.uint32) >> 16).astype(np.uint16))
    f16 = _lib.DeviceDense.upload(ctx, as_given(ra), True, compute_dtype=dtype)
    t16 = _lib.DeviceDense.upload(ctx, as_given(rb), True, compute_dtype=dtype)
    row_ptr, idx, sim, counts = _lib.dense_join16(ctx, f16, t16, None, None, 0.0, capacity=256 * 256)
    assert counts["pairs"] == 256 * 256
    rows, cols = DJ.csr_pairs(row_ptr, idx)
    worst = np.abs(sim.astype(np.float64) - C.cosines64(ra, rb)[rows, cols]).max()
    bound = C.accumulation_term(d)
    print(f"{dtype} width {d}: max |16-bit score - float64 cosine of the rounded vectors| {worst:.3e} = {worst / bound:.4f} of (ld + 8) 2^-23 = {bound:.3e}")
    assert worst <= bound


# ---- 6. the candidate buffer -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("name", ["300x513x64", "600x128"])
def test_a_candidate_buffer_of_one_gives_the_same_bytes_after_a_second_search(ctx, name, dtype):
    """cand_capacity=1 against a buffer with room for every candidate and against the default (the library's choice): the same bytes;
    the search that did not fit ran twice, which its counters show"""
    from polyfuzz_amd import _lib
    f, t, f16, t16 = _devs(ctx, name, dtype)
    rows, cols, sim, row_ptr, _ = _rescored(ctx, name, dtype)                  # (the default buffer)
    tiles = lambda n: -(-n // 256)
    want_tiles = tiles(f.n) * (tiles(f.n) + 1) // 2 if t is None else tiles(f.n) * tiles(t.n)
    once = _lib.dense_join16(ctx, f16, t16, f, t, T, counters=True, cand_capacity=1 << 16)
    twice = _lib.dense_join16(ctx, f16, t16, f, t, T, counters=True, cand_capacity=1)
    for b_ptr, b_idx, b_sim, _ in (once, twice):
        assert b_ptr.tobytes() == row_ptr.tobytes() and b_idx.tobytes() == cols.astype(np.int32).tobytes() and b_sim.tobytes() == sim.tobytes()
    counts, b_counts = once[3], twice[3]
    assert 1 < counts["candidates"] <= 1 << 16 and b_counts["candidates"] == counts["candidates"] and b_counts["pairs"] == counts["pairs"]
    assert counts["tiles"] == want_tiles and b_counts["tiles"] == 2 * want_tiles and b_counts["hit_corners"] == 2 * counts["hit_corners"]
    if t is None:
        label, pairs, components, work = _lib.dense_components16(ctx, f16, f, T, counters=True, cand_capacity=1)
        assert label.tobytes() == DJ.union_find_labels(f.n, rows, cols).tobytes() and pairs == len(rows)
        assert work["tiles"] == 2 * want_tiles and work["candidates"] == counts["candidates"]


# ---- 7. a call cut into two launches -----------------------------------------------------------------------------------------------

BIG_N = 1_048_600            # 4097 row tiles of 256: the upper triangle's blocks are more than 2^23 workgroups of 512
# duplicates (i, j): (5, 100) in the first block, so in the first launch; the other three in the last two block columns, which the
# second launch holds (it starts at block column 511, block row 248) -- one from row tile 0, one deep in the triangle, one in the
# last tile (4096, 4096)
BIG_PLANTED = ((5, 100), (3, 1_048_590), (600_000, 1_048_000), (1_048_580, 1_048_599))


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_a_self_join_of_more_than_2_23_workgroups_is_two_launches(ctx, dtype):
    """1 048 600 Gaussian rows of width 64 (no two reach a cosine of 0.9: the density of a cosine in 64 dimensions falls as
    (1 - c^2)^30.5) with four duplicated rows: the join and the components find exactly those pairs"""
    from polyfuzz_amd import _lib
    if "big" not in _cache:
        x = np.random.default_rng(23).standard_normal((BIG_N, 64), dtype=np.float32)
        for i, j in BIG_PLANTED:
            x[j] = x[i]
        _cache["big"] = _lib.DeviceDense.upload(ctx, x)
    f = _cache["big"]
    f16 = f.derive16(dtype)
    row_ptr, idx, sim, counts = _lib.dense_join16(ctx, f16, None, f, None, 0.9, counters=True)
    rows, cols = DJ.csr_pairs(row_ptr, idx)
    assert sorted(zip(rows.tolist(), cols.tolist())) == sorted(BIG_PLANTED)
    assert (sim >= np.float32(1.0) - np.float32(2e-7)).all()
    tiles = -(-BIG_N // 256)
    assert counts["tiles"] == tiles * (tiles + 1) // 2 and counts["tiles"] > 2 ** 23
    label, pairs, components = _lib.dense_components16(ctx, f16, f, 0.9)
    assert pairs == len(BIG_PLANTED) and components == BIG_N - len(BIG_PLANTED)
    moved = np.nonzero(label != np.arange(BIG_N, dtype=np.int32))[0]
    assert sorted(zip(label[moved].tolist(), moved.tolist())) == sorted(BIG_PLANTED)


# ---- 8. the pool fill ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", C.DTYPES)
def test_results_do_not_depend_on_what_the_allocator_hands_out(ctx, dtype):
    """the rescored join (with and without a repeated search), its capacity repeat and the components under Context.pool_fill's three
    modes: equal bytes, and equal to the run without a fill; back to mode 0 at the end"""
    from polyfuzz_amd import _lib
    from tests import pool_fill_cases as PF
    x, _ = _lists("600x128")
    rows, cols, sim, row_ptr, counts = _rescored(ctx, "600x128", dtype)
    want_label = DJ.union_find_labels(len(x), rows, cols)

    def run():
        f = _lib.DeviceDense.upload(ctx, x)            # its own handles: the copies are made under the fill
        f16 = f.derive16(dtype)
        out = []
        for kw in ({}, {"cand_capacity": 1}, {"capacity": 1}):
            out += list(_lib.dense_join16(ctx, f16, None, f, None, T, **kw)[:3])
        out += list(_lib.dense_join16(ctx, f16, None, None, None, T)[:3])
        label, pairs, components = _lib.dense_components16(ctx, f16, f, T)
        return out + [label, np.array([pairs, components], np.int64)]
    try:
        runs = []
        for _, mode in PF.FILLS:
            ctx.pool_fill(mode)
            runs.append(run())
    finally:
        ctx.pool_fill(0)
    for got in runs:
        for k in range(3):
            for g, w in zip(got[3 * k:3 * k + 3], (row_ptr, cols.astype(np.int32), sim)):
                assert g.tobytes() == w.tobytes(), k
        assert got[12].tobytes() == want_label.tobytes() and got[13].tolist() == [len(rows), len(np.unique(want_label))]
        for g, w in zip(got, runs[0]):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
