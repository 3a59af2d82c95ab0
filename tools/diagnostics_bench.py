"""mcmc_diagnostics on one MI355X (csrc/dc_diagnostics.hip.h) at 4 chains x 1000 draws: (a) 45 quantities, the
basic model's latent vector, (b) 35 502 quantities, the dynamic model of BASELINE config 4.

    python tools/diagnostics_bench.py [--out DIR] [--reps N] [--ref-quantities N]

Reports per case: the kernel times of `diag_rank`, `diag_ess` and the transpose (summed over the chunks of a call)
from a `rocprofv3 --kernel-trace --stats` run of its own (a child process; profiler off for the wall times); the
wall time of the device call (HipContext.mcmc_diagnostics: H2D + kernels + D2H) and of the public
`bpl.mcmc_diagnostics` (medians of N after a warm-up); the time of the numpy restatement (tests/diagnostics_ref.py)
on the same input -- on the first --ref-quantities quantities of case (b), scaled to all of them; and the counted
float64 operations of the autocovariance walk, S x lags computed x 5 per series, as a fraction of the float64
vector rate (78.6 TFLOP/s).  The lags computed are whole blocks of 64 up to each series' truncation point, read from
the restatement's walk on a sample of the quantities.  The draws are AR(1) chains with phi drawn from [0, 0.6], about
what NUTS leaves.  Writes diagnostics_bench.json and diagnostics_bench.txt under --out (default:
profiles/diagnostics)."""
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

C, N = 4, 1000
CASES = {"basic_45": 45, "dynamic_35502": 35502}
KERNELS = ("diag_rank", "diag_ess", "transpose_f64")
F64_VECTOR_RATE = 78.6e12
SERIES = 4   # bulk, mean and the two tail indicators


def draws(Q, seed=5):
    rs = np.random.RandomState(seed)
    phi = rs.uniform(0.0, 0.6, Q)
    x = np.empty((C, N, Q))
    x[:, 0] = rs.normal(size=(C, Q)) / np.sqrt(1.0 - phi * phi)
    for i in range(1, N):
        x[:, i] = phi * x[:, i - 1] + rs.normal(size=(C, Q))
    return np.ascontiguousarray(x.reshape(C * N, Q))


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
    d = tempfile.mkdtemp(prefix="diag_rocprof_")
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
                            n = int(row["Calls"])
                            out[k] = {"launches_per_call": n / (reps + 1),
                                      "us_per_call": float(row["TotalDurationNs"]) / 1e3 / (reps + 1)}
        if set(out) != set(KERNELS):
            raise RuntimeError(f"the rocprofv3 stats hold {sorted(out)}, not {KERNELS}")
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def lag_blocks(x):
    """Blocks of 64 lags the device walks for the four series of one quantity: the restatement's truncation points."""
    import diagnostics_ref as R

    s = R.split_chains(x, C)
    series = [R.z_scale(s), s] + [(s <= np.quantile(s, q)).astype(np.float64) for q in (0.05, 0.95)]
    blocks = 0
    for m in series:
        blocks += R.ess_of(m, with_last_lag=True)[2] // 64 + 1
    return blocks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diagnostics"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-quantities", type=int, default=200)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    import bpl
    from bpl._ffi import HipContext

    ctx = HipContext(0)
    if args.child:
        v = draws(CASES[args.child])
        for _ in range(args.reps + 1):
            ctx.mcmc_diagnostics(v, C)
        return
    import diagnostics_ref as R

    os.makedirs(args.out, exist_ok=True)
    res, lines = {}, []
    for case, Q in CASES.items():
        v = draws(Q)
        wall = {"device_call": timed(lambda: ctx.mcmc_diagnostics(v, C), args.reps),
                "mcmc_diagnostics": timed(lambda: bpl.mcmc_diagnostics(v, C), args.reps)}
        nref = min(Q, args.ref_quantities)
        t0 = time.perf_counter()
        ref = R.diagnose(v[:, :nref], C)
        ref_s = (time.perf_counter() - t0) * Q / nref
        got = ctx.mcmc_diagnostics(v, C)
        err = {nm: float(np.max(np.abs(got[nm][:nref] - ref[nm]) / (1.0 + np.abs(ref[nm])))) for nm in R.STATS}
        blocks = float(np.mean([lag_blocks(v[:, j]) for j in range(min(nref, 50))]))
        kern = kernel_times(case, args.reps)
        S = 2 * C * (N // 2)
        flops = Q * S * 64.0 * blocks * 5.0
        frac = flops / (kern["diag_ess"]["us_per_call"] * 1e-6) / F64_VECTOR_RATE
        res[case] = {"quantities": Q, "chains": C, "draws_per_chain": N, "wall": wall, "kernel": kern,
                     "numpy_restatement_s": ref_s, "numpy_restatement_quantities_timed": nref,
                     "worst_error_over_1_plus_ref": err, "lag_blocks_per_quantity": blocks,
                     "counted_f64_operations": flops, "fraction_of_f64_vector_rate": frac}
        lines += [
            f"{case}: {Q} quantities x {C} chains x {N} draws",
            "  kernels per call: " + ", ".join(f"{k} {kern[k]['us_per_call']:.1f} us ({kern[k]['launches_per_call']:.0f} "
                                               f"launches)" for k in KERNELS),
            f"  device call {wall['device_call']['median_ms']:.3f} ms, bpl.mcmc_diagnostics "
            f"{wall['mcmc_diagnostics']['median_ms']:.3f} ms (medians of {args.reps}); numpy restatement "
            f"{ref_s:.2f} s ({nref} quantities timed)",
            f"  autocovariance walk: {blocks:.2f} blocks of 64 lags per quantity over {SERIES} series, "
            f"{flops:.3g} counted float64 operations = {100 * frac:.2f} % of the float64 vector rate in diag_ess",
            "  worst |device - restatement| / (1 + |restatement|): " + ", ".join(f"{k} {e:.1e}" for k, e in err.items())]
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(args.out, "diagnostics_bench.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.join(args.out, "diagnostics_bench.txt"), "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
