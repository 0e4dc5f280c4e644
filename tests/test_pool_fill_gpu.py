"""No result may depend on device memory nobody wrote.  Every temporary and every handle takes its memory from the context's caching
allocator, whose blocks hold whatever their last user left -- very often the same kernel's correct data of the test before, or the
zeros of a fresh block --, so a missing initialisation is invisible to every comparison with an oracle.  pfz_pool_fill makes the
allocator hand out blocks pre-filled with a chosen 64-bit word; each battery of tests/pool_fill_cases.py is run under ZERO, ONE64 and
ONE32 and the runs are compared on their bytes (dtype and shape included; NaN and -0.0 count), and the ZERO run once with the oracle
of the entries' own tests, which keeps three equally wrong runs from passing.  ONE32 makes a 64-bit view read 2^32 + 1 and so runs
only after ONE64 has shown no dependence: an assertion ends the test.  BLIND SPOT: as floats the patterns are zero or denormals, so a
float accumulator that is not cleared is not seen (include/polyfuzz_hip.h).  The positive control shows that the seam is
live: a table pfz_topn_alloc hands out uncleared by design shows exactly the pattern."""
import time

import numpy as np
import pytest

from tests import pool_fill_cases as C

pytestmark = pytest.mark.gpu


def _hold(name, fill_all, run, check, oracle_mod):
    """the battery `run` under the three fills: ZERO against the oracle (`check`), ONE64 and ONE32 against ZERO on the bytes"""
    t0 = time.perf_counter()
    try:
        base = None
        for label, mode in C.FILLS:
            fill_all(mode)
            got = run()
            if base is None:
                base = got
                check(base, oracle_mod)
                print(f"pool fill, {name}: {len(base)} arrays under ZERO equal the oracle; forms that ran: {base.forms}")
                continue
            differ = C.differences(got, base)
            assert not differ, f"{name}: under {label} these results differ from the ZERO run, so they read memory nobody wrote: {differ}"
            assert got.forms == base.forms, (label, got.forms, base.forms)
    finally:
        fill_all(0)
    print(f"pool fill, {name}: three fills in {time.perf_counter() - t0:.1f} s")


@pytest.mark.parametrize("group", list(C.GROUPS))
def test_results_do_not_depend_on_what_the_allocator_hands_out(ctx, oracle_mod, group):
    run, check = C.GROUPS[group]
    _hold(group, ctx.pool_fill, lambda: run(ctx), check, oracle_mod)


def test_sharded_results_do_not_depend_on_what_the_allocator_hands_out(oracle_mod):
    """world 2 on the local transport, 301 x 257: the from-side sharded job and the to-side sharded job with its merge; the fill is
    set on both ranks' contexts"""
    import polyfuzz_amd
    ctxs = [polyfuzz_amd.Context(0), polyfuzz_amd.Context(0)]

    def fill_all(mode):
        for c in ctxs:
            c.pool_fill(mode)
    _hold("sharded", fill_all, lambda: C.run_sharded(ctxs), C.check_sharded, oracle_mod)


def test_positive_control_an_uncleared_table_shows_the_fill(ctx):
    """pfz_topn_alloc returns an uncleared block by design (pfz_topn_clear is separate): downloaded as it is, a 7 x 3 table -- 84
    bytes per half, whole 64-bit words but for the last four bytes -- shows exactly the mode's word in both halves.  So the seam is
    live, and a read of unwritten memory is seen by the comparison of the batteries.  Back under mode 0 nothing is promised about a
    table that was cleared, freed and allocated again: the allocator does not clear, the call only has to work."""
    from polyfuzz_amd import _lib
    try:
        for mode in (C.ONE64, C.ONE32, C.ZERO):
            ctx.pool_fill(mode)
            word = ctx.POOL_FILL_WORDS[mode]
            t = _lib.DeviceTopN.alloc(ctx, 7, 3)
            idx, val = t.download()
            for half in (idx, val):
                raw = half.tobytes()
                assert len(raw) == 84
                assert (np.frombuffer(raw[:80], "<u8") == word).all(), (mode, half)
                assert raw[80:] == int(word).to_bytes(8, "little")[:4], (mode, half)
            if mode == C.ONE32:
                assert (idx == 1).all() and (val.view(np.uint32) == 1).all()
            if mode == C.ONE64:
                assert (idx.reshape(-1)[0::2] == 1).all() and (idx.reshape(-1)[1::2] == 0).all()
            t.clear()
            t.free()
        for bad in (-1, 4, 255):
            with pytest.raises(_lib.PfzError, match="pfz_pool_fill"):
                ctx.pool_fill(bad)
        ctx.pool_fill(0)
        t = _lib.DeviceTopN.alloc(ctx, 7, 3)
        assert t.download()[0].shape == (7, 3)
    finally:
        ctx.pool_fill(0)
