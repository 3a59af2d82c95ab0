"""weighted_shift / powerscale_sensitivity on one MI355X (csrc/dc_sensitivity.hip.h) at 4 rows x 4000 draws:
(a) 45 quantities, the basic model's latent vector, (b) 35 502 quantities, the dynamic model of BASELINE config 4.

    python tools/sensitivity_bench.py [--out DIR] [--reps N] [--ref-quantities N]

Reports per case: the kernel times of `shift_summary`, `psis_rows` and the transpose (summed over the chunks of a
call) from a `rocprofv3 --kernel-trace --stats` run of its own (a child process; profiler off for the wall times);
the wall time of the device call (HipContext.weighted_shift: H2D + kernels + D2H) and of the public
`bpl.powerscale_sensitivity` (medians of N after a warm-up); `mcmc_diagnostics` (4 chains x 1000 draws) on the same
draws in the same run; the time of the numpy restatement (tests/sensitivity_ref.py) on the same input -- on the
first --ref-quantities quantities, SCALED to all of them; the worst |device - restatement| of cjs_sq as a fraction
of the gate 1e-9 ref + 1e-15; and the counted log2 evaluations (4 per interval and row) per second of kernel time.
The draws are independent normal columns; column 0 carries the likelihood (l = -x^2 / 2), column 1 the prior.  No
hardware counters are collected here (they would need a run of their own).  Writes sensitivity_bench.json and
sensitivity_bench.txt under --out (default: profiles/sensitivity)."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "bpl-next_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

S, ROWS, DELTA, CHAINS = 4000, 4, 0.01, 4
CASES = {"basic_45": 45, "dynamic_35502": 35502}
KERNELS = ("shift_summary", "psis_rows", "transpose_f64")


def inputs(Q, seed=5):
    rs = np.random.RandomState(seed)
    v = rs.normal(size=(S, Q))
    return v, -np.abs(v[:, 1]), -0.5 * v[:, 0] ** 2


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * float(np.min(ts)),
            "max_ms": 1e3 * float(np.max(ts)), "reps": reps}


def kernel_times(case, reps):
    d = tempfile.mkdtemp(prefix="shift_rocprof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--child", case, "--reps", str(reps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
        if r.returncode != 0:
            raise RuntimeError(f"the rocprofv3 run exited {r.returncode}: {r.stderr[-2000:]}")
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    for k in KERNELS:
                        if k in row["Name"]:
                            out[k] = {"launches_per_call": int(row["Calls"]) / (reps + 1),
                                      "us_per_call": float(row["TotalDurationNs"]) / 1e3 / (reps + 1)}
        if set(out) != set(KERNELS):
            raise RuntimeError(f"the rocprofv3 stats hold {sorted(out)}, not {KERNELS}")
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sensitivity"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-quantities", type=int, default=200)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    import bpl
    import sensitivity_ref as R
    from bpl._ffi import HipContext

    ctx = HipContext(0)
    if args.child:
        v, lp, ll = inputs(CASES[args.child])
        ratios = R.power_ratios(lp, ll, DELTA)
        for _ in range(args.reps + 1):
            ctx.weighted_shift(v, ratios)
        return

    os.makedirs(args.out, exist_ok=True)
    res, lines = {}, []
    for case, Q in CASES.items():
        v, lp, ll = inputs(Q)
        ratios = R.power_ratios(lp, ll, DELTA)
        wall = {"device_call": timed(lambda: ctx.weighted_shift(v, ratios), args.reps),
                "powerscale_sensitivity": timed(lambda: bpl.powerscale_sensitivity(v, lp, ll, delta=DELTA), args.reps),
                "mcmc_diagnostics": timed(lambda: bpl.mcmc_diagnostics(v, CHAINS), args.reps)}
        nref = min(Q, args.ref_quantities)
        t0 = time.perf_counter()
        ref = R.weighted_shift(v[:, :nref], ratios)
        ref_s = (time.perf_counter() - t0) * Q / nref
        got = ctx.weighted_shift(v, ratios)
        gate = float(np.max(np.abs(got["cjs_sq"][:, :nref] - ref["cjs_sq"]) / (1e-9 * ref["cjs_sq"] + 1e-15)))
        err = {nm: float(np.max(np.abs(got[nm][:, :nref] - ref[nm]) / (1.0 + np.abs(ref[nm])))) for nm in ("mean", "sd")}
        kern = kernel_times(case, args.reps)
        log2s = 4.0 * ROWS * Q * (S - 1)
        rate = log2s / (kern["shift_summary"]["us_per_call"] * 1e-6)
        res[case] = {"quantities": Q, "draws": S, "rows": ROWS, "delta": DELTA, "wall": wall, "kernel": kern,
                     "numpy_restatement_s_scaled": ref_s, "numpy_restatement_quantities_timed": nref,
                     "worst_cjs_sq_error_over_gate": gate, "worst_error_over_1_plus_ref": err,
                     "counted_log2": log2s, "log2_per_second_in_shift_summary": rate}
        lines += [
            f"{case}: {Q} quantities x {S} draws x {ROWS} rows (delta = {DELTA})",
            "  kernels per call: " + ", ".join(f"{k} {kern[k]['us_per_call']:.1f} us ({kern[k]['launches_per_call']:.0f} "
                                               f"launches)" for k in KERNELS),
            f"  device call {wall['device_call']['median_ms']:.3f} ms, bpl.powerscale_sensitivity "
            f"{wall['powerscale_sensitivity']['median_ms']:.3f} ms, bpl.mcmc_diagnostics ({CHAINS} chains) "
            f"{wall['mcmc_diagnostics']['median_ms']:.3f} ms (medians of {args.reps})",
            f"  numpy restatement {ref_s:.2f} s, SCALED from the {nref} quantities timed",
            f"  {log2s:.3g} counted log2 = {rate:.3g} per second of shift_summary",
            f"  worst |device - restatement| of cjs_sq: {gate:.2e} of its gate; mean {err['mean']:.1e}, sd {err['sd']:.1e} "
            "over (1 + |restatement|)"]
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(args.out, "sensitivity_bench.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.join(args.out, "sensitivity_bench.txt"), "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
