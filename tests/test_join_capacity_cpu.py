"""The capacity protocol of the six threshold-join wrappers of polyfuzz_amd._lib (_join_call): a modest first buffer, the exact
total back from the library, ONE repeat with room for it.  No GPU: ctx.lib is a fake that records every ctypes call, reports the
totals the case prescribes and fills the caller's buffers the way the library does -- only when they have room."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from polyfuzz_amd import _lib

N_FROM = 7


class FakeLib:
    """pfz_*_join(..., capacity, out_row_ptr, per-hit arrays ..., out_total, out_counters): every join entry ends like that"""

    def __init__(self, n_hit_arrays, dtypes, totals):
        self.n_hit_arrays, self.dtypes, self.totals = n_hit_arrays, dtypes, list(totals)
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("pfz_"):
            raise AttributeError(name)

        def entry(*args):
            cap, row_ptr, *hits, total, work = args[-(4 + self.n_hit_arrays):]
            reported = self.totals[len(self.calls)]
            self.calls.append(SimpleNamespace(name=name, cap=cap, hit_addresses=[h.value for h in hits], head=args[:-(4 + self.n_hit_arrays)]))
            total._obj.value = reported
            if reported <= cap:                      # (beyond the capacity the library leaves the caller's buffers alone)
                (ctypes.c_int64 * (N_FROM + 1)).from_address(row_ptr.value)[:] = [0] * N_FROM + [reported]
                for h, dt in zip(hits, self.dtypes):
                    if reported:
                        np.ctypeslib.as_array(ctypes.cast(h, ctypes.POINTER(np.ctypeslib.as_ctypes_type(dt))), (reported,))[:] = np.arange(reported)
            if work is not None:
                n_work = {"pfz_dense_join": 2, "pfz_pairs_join_keys": 4}.get(name, 3)
                (ctypes.c_int64 * n_work).from_address(work.value)[:] = range(10, 10 + n_work)
            return 0
        return entry


def _strings():
    return SimpleNamespace(h=object(), n=N_FROM)


# wrapper name -> (the library entry, dtypes of the per-hit arrays, call(ctx, **kw), has a trailing counts dict always)
WRAPPERS = {
    "lev_join": ("pfz_lev_join", (np.int32, np.int32, np.float64),
                 lambda ctx, **kw: _lib.lev_join(ctx, _strings(), _strings(), "levenshtein", 0.5, **kw), False),
    "indel_join": ("pfz_indel_join", (np.int32, np.int32, np.float64),
                   lambda ctx, **kw: _lib.indel_join(ctx, _strings(), None, 0.5, **kw), False),
    "pairs_join": ("pfz_pairs_join", (np.int32, np.float64),
                   lambda ctx, **kw: _lib.pairs_join(ctx, _strings(), None, SimpleNamespace(h=object()), "osa", 0.5, **kw), False),
    "dense_join": ("pfz_dense_join", (np.int32, np.float32),
                   lambda ctx, **kw: _lib.dense_join(ctx, SimpleNamespace(h=object(), n=N_FROM, dtype="float32", normalize=True), None, 0.5,
                                                     **kw), True),
    "sparse_join": ("pfz_cossim_join", (np.int32, np.float32),
                    lambda ctx, **kw: _lib.sparse_join(ctx, SimpleNamespace(h=object()), SimpleNamespace(h=object(), n_rows=N_FROM), 0.5,
                                                       **kw), True),
    "pairs_join_keys": ("pfz_pairs_join_keys", (np.int32, np.float64),
                        lambda ctx, **kw: _lib.pairs_join_keys(ctx, _strings(), _strings(), SimpleNamespace(h=object()), "jaro", 0.5, **kw),
                        False),
}


def _run(wrapper, totals, **kw):
    entry, dtypes, call, _ = WRAPPERS[wrapper]
    lib = FakeLib(len(dtypes), dtypes, totals)
    out = call(SimpleNamespace(lib=lib, h=object()), **kw)
    assert all(c.name == entry for c in lib.calls)
    return lib, out


def _check_result(wrapper, lib, out, total):
    _, dtypes, _, has_counts = WRAPPERS[wrapper]
    row_ptr, hits = out[0], out[1:1 + len(dtypes)]
    assert row_ptr.dtype == np.int64 and row_ptr.shape == (N_FROM + 1,) and row_ptr[-1] == total
    last = lib.calls[-1]
    for a, dt, address in zip(hits, dtypes, last.hit_addresses):
        assert a.dtype == dt and a.shape == (total,)
        np.testing.assert_array_equal(a, np.arange(total).astype(dt))
        assert a.flags.owndata and a.base is None                         # a copy of its own: not a view of the call's buffer
        assert total == 0 or not address <= a.ctypes.data < address + max(last.cap, 1) * a.itemsize
    if has_counts:
        assert out[1 + len(dtypes)] == {"pairs": total} and len(out) == 2 + len(dtypes)
    else:
        assert len(out) == 1 + len(dtypes)


@pytest.mark.parametrize("wrapper", sorted(WRAPPERS))
@pytest.mark.parametrize("capacity,total", ((8, 5), (8, 8), (8, 0), (0, 0), (None, 4095), (None, 4096), (None, 0)),
                         ids=("below", "equal", "none", "zero_capacity_none", "default_below", "default_equal", "default_none"))
def test_one_call_while_the_total_fits(wrapper, capacity, total):
    lib, out = _run(wrapper, [total], capacity=capacity)
    assert [c.cap for c in lib.calls] == [max(4096, 4 * N_FROM) if capacity is None else capacity]
    _check_result(wrapper, lib, out, total)


@pytest.mark.parametrize("wrapper", sorted(WRAPPERS))
@pytest.mark.parametrize("capacity,total", ((8, 9), (0, 3), (None, 4097)), ids=("above", "zero_capacity", "default_above"))
def test_one_repeat_with_room_for_the_exact_total(wrapper, capacity, total):
    lib, out = _run(wrapper, [total, total], capacity=capacity)
    assert [c.cap for c in lib.calls] == [max(4096, 4 * N_FROM) if capacity is None else capacity, total]
    assert lib.calls[0].head == lib.calls[1].head                          # the same operands and threshold both times
    _check_result(wrapper, lib, out, total)


@pytest.mark.parametrize("wrapper", sorted(WRAPPERS))
def test_a_second_total_beyond_its_room_raises(wrapper):
    entry, dtypes, call, _ = WRAPPERS[wrapper]
    lib = FakeLib(len(dtypes), dtypes, [9, 10, 10])
    with pytest.raises(AssertionError):
        call(SimpleNamespace(lib=lib, h=object()), capacity=8)
    assert [c.cap for c in lib.calls] == [8, 9]                            # never a third call


@pytest.mark.parametrize("wrapper", sorted(WRAPPERS))
def test_counters_are_the_last_calls(wrapper):
    _, dtypes, _, has_counts = WRAPPERS[wrapper]
    names = {"lev_join": _lib.LEV_JOIN_COUNTERS, "indel_join": _lib.LEV_JOIN_COUNTERS, "pairs_join": _lib.PAIR_JOIN_COUNTERS,
             "dense_join": _lib.DENSE_JOIN_COUNTERS, "sparse_join": _lib.SPARSE_JOIN_COUNTERS, "pairs_join_keys": _lib.PAIR_KEYS_COUNTERS}[wrapper]
    lib, out = _run(wrapper, [9, 9], capacity=8, counters=True)
    assert len(lib.calls) == 2 and len(out) == 2 + len(dtypes)
    want = dict(zip(names, range(10, 10 + len(names))))
    assert out[-1] == ({"pairs": 9, **want} if has_counts else want)
    assert list(out[-1]) == (["pairs"] if has_counts else []) + list(names)
