"""K5 with exact rescoring of the int8 / bfloat16 / 1-bit top-n on one panel's worth of BASELINE configuration 5, in one process.

usage: python tools/bench_dense_rescore.py [--rows 4096] [--to 500000] [--dim 768] [--top-n 5] [--repeats 7] [--out FILE]

Seeded unit-norm random-normal vectors, device-resident operands (pipeline.DenseMatchJob), top-5, as tools/bench_dense16.py.
Arms, all in this run: fp32; int8 and bfloat16 plain; int8 and bfloat16 with rescore_multiplier 2, 4 and 8; the sign bits of
the same vectors (DeviceDense.upload_bits, a Hamming search) plain and with rescore_multiplier 4, 16 and 64 -- a 1-bit search
is used with a large oversampling -- which are reported, not gated (the coarse search
keeps top_n x multiplier candidates per row, k5_rescore_topn scores them against the fp32 vectors).  Every arm is warmed up
and then timed over `repeats` steps with device events (pfz_event_*), one pair per step; a further profiled pass
(pfz_prof_*) gives the GEMM's, the row top-n's and the rescoring kernel's own time.  For the rescoring kernel: the bytes it
gathers (rows x candidates x padded width x 4 B, plus the from-rows once) over its time, against the 6.3 TB/s a streaming
kernel reaches on this part's HBM.  Each rescored arm also reports in how many rows its top-n columns equal the fp32 arm's.
Mixed arms, beside the float32-rescoring arm of the same coarse type and multiplier: int8 x 4 against the int8 to-side itself,
binary x 16 against the bits and against an int8 to-side (k5_mixed_rescore: the float32 from-vectors against the quantised
to-rows, 1/4 or 1/32 of the bytes per candidate, no float32 to-side needed); `to_side_bytes` gives the device footprint of each
form of the to-side as the pool counts it (pfz_pool_stats).
The condition: int8 with multiplier 4 is faster than fp32 beyond the spread of the repeats; the expectation (reported, not a
gate): within about 10 % of plain int8.
Prints one JSON object; --out also writes it to a file.  Run it under a time limit (timeout 600 ...)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

HBM = 6.3e12
MULTIPLIERS = (2, 4, 8)
BINARY_MULTIPLIERS = (4, 16, 64)
MIXED = (("int8", 4, "int8"), ("binary", 16, "binary"), ("binary", 16, "int8"))      # coarse type, multiplier, to-side of the rescoring


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--to", type=int, default=500_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--top-n", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    import polyfuzz_amd
    from polyfuzz_amd import _lib, pipeline
    ctx = polyfuzz_amd.Context.default()

    rng = np.random.default_rng(5)
    def unit(n):
        v = rng.standard_normal((n, args.dim), dtype=np.float32)
        v /= np.sqrt((v.astype(np.float64) ** 2).sum(1))[:, None].astype(np.float32)
        return v
    a, b = unit(args.rows), unit(args.to)
    ld = (args.dim + 31) // 32 * 32
    res = {"shape": [args.rows, args.to, args.dim], "top_n": args.top_n, "repeats": args.repeats, "device": ctx.info()["name"],
           "data": "seeded unit-norm random normal", "hbm_bytes_per_s": HBM, "arms": {}}
    res["to_side_bytes"] = {}
    def both(operand):
        up = _lib.DeviceDense.upload_bits if operand == "binary" else (lambda c, v: _lib.DeviceDense.upload_as(c, v, operand))
        h_a = up(ctx, a)
        ctx.sync()
        before = ctx.pool_stats()[0]
        h_b = up(ctx, b)
        ctx.sync()
        res["to_side_bytes"][operand] = ctx.pool_stats()[0] - before
        return h_a, h_b
    exact = dict(zip("ab", both("float32")))       # shared by every rescored arm
    coarse = {"int8": both("int8"), "bf16": both("bfloat16")}
    arms = [("fp32", None, None, None)] + [(k, k, None, None) for k in coarse] + [(f"{k}_x{m}", k, m, None) for k in coarse for m in MULTIPLIERS]
    coarse["binary"] = both("binary")
    arms += [("binary", "binary", None, None)] + [(f"binary_x{m}", "binary", m, None) for m in BINARY_MULTIPLIERS]
    arms += [(f"{k}_x{m}_to_{to}", k, m, to) for k, m, to in MIXED]
    topn = {}
    for arm, kind, mult, to in arms:
        if kind is None:
            job = pipeline.DenseMatchJob(ctx, exact["a"], exact["b"], top_n=args.top_n)
        elif mult is None:
            job = pipeline.DenseMatchJob(ctx, coarse[kind][0], coarse[kind][1], top_n=args.top_n)
        else:
            job = pipeline.DenseMatchJob(ctx, coarse[kind][0], coarse[kind][1], top_n=args.top_n, rescore_from=exact["a"],
                                         rescore_to=exact["b"] if to is None else coarse[to][1], rescore_multiplier=mult)
        for _ in range(2):                        # warm-up: code objects, the pool's panels, clocks
            job.step()
        ctx.sync()
        ms = []
        for _ in range(args.repeats):
            ctx.event_record(0)
            job.step()
            ctx.event_record(1)
            ctx.sync()
            ms.append(ctx.event_elapsed_ms(0, 1))
        ctx.prof_enable(True)
        ctx.prof_reset()
        out = job.step()
        ctx.sync()
        gemm_ms, n_panels = ctx.prof_get("k5_gemm_panel")
        topn_ms, _ = ctx.prof_get("k5_row_topn")
        resc_ms, n_resc = ctx.prof_get("k5_rescore_topn" if to is None else "k5_mixed_rescore")
        ctx.prof_enable(False)
        idx, _ = out.download()
        topn[arm] = idx.copy()
        r = {"ms_per_step_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)),
             "ms_all": [round(x, 3) for x in ms], "gemm_ms": gemm_ms, "row_topn_ms": topn_ms, "panels": n_panels}
        if mult is not None:
            m = job.candidates.ntop
            # a to-row as the kernel reads it: float32 padded to 32 values, int8 to 128 values, bits to 128 bits
            to_row = {None: 4.0 * ld, "int8": (args.dim + 127) // 128 * 128, "binary": (args.dim + 127) // 128 * 16}[to]
            gathered = args.rows * (to_row * m + 4.0 * ld)
            r.update({"candidates_per_row": m, "rescore_ms": resc_ms, "rescore_launches": n_resc, "rescore_bytes_gathered": gathered,
                      "rescore_bytes_per_s": gathered / (resc_ms * 1e-3) if resc_ms > 0 else None,
                      "rescore_fraction_of_6.3TB/s": gathered / (resc_ms * 1e-3) / HBM if resc_ms > 0 else None,
                      "rescore_ms_at_6.3TB/s": gathered / HBM * 1e3})
        if to is not None:
            r["rescored_against"] = to
        res["arms"][arm] = r
        del job, out
    base = res["arms"]["fp32"]
    for arm, kind, mult, to in arms[1:]:
        r = res["arms"][arm]
        r["speedup_over_fp32"] = base["ms_per_step_median"] / r["ms_per_step_median"]
        r["beats_fp32_beyond_spread"] = bool(r["ms_max"] < base["ms_min"])      # its slowest step against the fastest fp32 step
        r["rows_with_the_fp32_columns"] = int((np.sort(topn[arm], axis=1) == np.sort(topn["fp32"], axis=1)).all(axis=1).sum())
        r["rows_equal_to_fp32_in_order"] = int((topn[arm] == topn["fp32"]).all(axis=1).sum())
        if mult is not None:
            plain = res["arms"][kind]
            r["step_over_plain_step"] = r["ms_per_step_median"] / plain["ms_per_step_median"]
            r["overhead_ms"] = r["ms_per_step_median"] - plain["ms_per_step_median"]
            r["overhead_ms_deeper_row_topn"] = r["row_topn_ms"] - plain["row_topn_ms"]
            r["overhead_ms_gemm"] = r["gemm_ms"] - plain["gemm_ms"]
        if to is not None:      # the yardstick of a mixed arm: the float32-rescoring arm of the same coarse type and multiplier
            sibling = res["arms"][f"{kind}_x{mult}"]
            r["step_over_float32_rescoring_step"] = r["ms_per_step_median"] / sibling["ms_per_step_median"]
            r["rescore_ms_over_float32_rescore_ms"] = r["rescore_ms"] / sibling["rescore_ms"] if sibling["rescore_ms"] > 0 else None
            r["rows_equal_to_float32_rescoring_in_order"] = int((topn[arm] == topn[f"{kind}_x{mult}"]).all(axis=1).sum())
    gate = res["arms"]["int8_x4"]
    res["int8_x4_faster_than_fp32"] = gate["beats_fp32_beyond_spread"]
    res["int8_x4_within_10_percent_of_plain_int8"] = bool(gate["step_over_plain_step"] <= 1.10)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if res["int8_x4_faster_than_fp32"] else 1


if __name__ == "__main__":
    sys.exit(main())
