"""K5 with fp32, float16, bfloat16, int8 and 1-bit operands on one panel's worth of BASELINE configuration 5, in one process.

usage: python tools/bench_dense16.py [--rows 4096] [--to 500000] [--dim 768] [--top-n 5] [--repeats 7] [--out FILE]

Seeded unit-norm random-normal vectors, device-resident operands (pipeline.DenseMatchJob), top-5.  Every arm is warmed up
and then timed over `repeats` steps with device events (pfz_event_*), one pair per step; a further profiled pass
(pfz_prof_*) gives the GEMM's and the row top-n's share.  The fp32 arm is the baseline: the fp32 tile program of the same
build, on the same data, in the same run.  Roofline figures per arm: the fraction of the 16-bit MFMA peak (2.5 PF; the
fp32 arm also against its own 157 TF, the int8 arm against the integer cores' 5 POPS = twice the 16-bit rate) and the time
the fp32 score panel alone takes at 6.3 TB/s.  The int8 arm holds the same vectors quantised per row on the device
(DeviceDense.upload_as); its yardstick is the bfloat16 arm of the same run.  The binary arm holds their sign bits, packed
on the device (DeviceDense.upload_bits), and runs the Hamming tile program on the vector ALU: it has no pass/fail time; its
step is recorded against the int8 and bfloat16 arms and against its roofline -- 2 lane-operations (XOR, bit count) per pair
and 32-bit word, at 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz = 78.6e12 lane-operations / s.
Prints one JSON object; --out also writes it to a file.  Run it under a time limit (timeout 600 ...)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

PEAK16, PEAK32, PEAK8, HBM = 2.5e15, 157e12, 5.0e15, 6.3e12
VALU = 256 * 4 * 32 * 2.4e9        # lane-operations per second of the vector ALU


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
    flop = 2.0 * args.rows * args.to * args.dim
    panel_bytes = 4.0 * args.rows * args.to
    res = {"shape": [args.rows, args.to, args.dim], "top_n": args.top_n, "repeats": args.repeats, "device": ctx.info()["name"],
           "data": "seeded unit-norm random normal", "flop": flop, "panel_write_ms_at_6.3TB/s": panel_bytes / HBM * 1e3, "arms": {}}
    top1 = {}
    for arm, operand in (("fp32", "float32"), ("f16", "float16"), ("bf16", "bfloat16"), ("int8", "int8"), ("binary", None)):
        def upload(v):
            return _lib.DeviceDense.upload_bits(ctx, v) if operand is None else _lib.DeviceDense.upload_as(ctx, v, operand)
        job = pipeline.DenseMatchJob(ctx, upload(a), upload(b), top_n=args.top_n)
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
        ctx.prof_enable(False)
        idx, _ = out.download()
        top1[arm] = idx[:, 0].copy()
        med = float(np.median(ms))
        res["arms"][arm] = {
            "ms_per_step_median": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)), "ms_all": [round(x, 3) for x in ms],
            "flop_per_s": flop / (med * 1e-3), "gemm_ms": gemm_ms, "row_topn_ms": topn_ms, "panels": n_panels,
            "gemm_share": gemm_ms / (gemm_ms + topn_ms), "row_topn_share": topn_ms / (gemm_ms + topn_ms),
            "gemm_flop_per_s": flop / (gemm_ms * 1e-3), "gemm_fraction_of_2.5PF": flop / (gemm_ms * 1e-3) / PEAK16,
            "gemm_over_panel_write_time": gemm_ms / (panel_bytes / HBM * 1e3)}
        if arm == "fp32":
            res["arms"][arm]["gemm_fraction_of_fp32_peak_157TF"] = flop / (gemm_ms * 1e-3) / PEAK32
        if arm == "int8":
            res["arms"][arm]["gemm_fraction_of_int8_peak_5POPS"] = flop / (gemm_ms * 1e-3) / PEAK8
        if arm == "binary":
            r = res["arms"][arm]
            for k in [k for k in r if "flop" in k or "2.5PF" in k]:          # no flops here
                del r[k]
            lane_ops = 2.0 * args.rows * args.to * ((args.dim + 31) // 32)
            r.update({"xor_popcount_lane_ops": lane_ops, "panel_lane_ops_per_s": lane_ops / (gemm_ms * 1e-3),
                      "panel_fraction_of_valu_78.6T": lane_ops / (gemm_ms * 1e-3) / VALU, "panel_ms_at_valu_peak": lane_ops / VALU * 1e3,
                      "operand_bytes_to_side": args.to * ((args.dim + 127) // 128 * 16)})
        del job, out
    base = res["arms"]["fp32"]
    for arm in ("f16", "bf16", "int8"):
        r = res["arms"][arm]
        r["speedup_over_fp32"] = base["ms_per_step_median"] / r["ms_per_step_median"]
        # faster by more than the spread of the repeats: the slowest 16-bit step against the fastest fp32 step
        r["beats_fp32_beyond_spread"] = bool(r["ms_max"] < base["ms_min"])
        r["top1_agrees_with_fp32_rows"] = int((top1[arm] == top1["fp32"]).sum())
    i8, bf = res["arms"]["int8"], res["arms"]["bf16"]
    i8["step_over_bf16_step"] = i8["ms_per_step_median"] / bf["ms_per_step_median"]
    i8["gemm_over_bf16_gemm"] = i8["gemm_ms"] / bf["gemm_ms"]
    i8["no_slower_than_bf16"] = bool(i8["ms_per_step_median"] <= bf["ms_per_step_median"])
    b1 = res["arms"]["binary"]
    b1["speedup_over_fp32"] = base["ms_per_step_median"] / b1["ms_per_step_median"]
    b1["step_over_int8_step"] = b1["ms_per_step_median"] / i8["ms_per_step_median"]
    b1["step_over_bf16_step"] = b1["ms_per_step_median"] / bf["ms_per_step_median"]
    b1["panel_over_int8_gemm"] = b1["gemm_ms"] / i8["gemm_ms"]
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if all(res["arms"][k]["beats_fp32_beyond_spread"] for k in ("f16", "bf16", "int8")) and i8["no_slower_than_bf16"] else 1


if __name__ == "__main__":
    sys.exit(main())
