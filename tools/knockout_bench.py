"""The knockout rules of simulate_tournament on one MI355X (csrc/dc_knockout.hip.h): the extra-time rule next to
the redraw rule of the same build, launched in the same run at the same shape, on the World-Cup model of
tools/tournament_bench.py (confederations, one host, S = 1000 posterior draws):

    world_cup_48   12 groups of 4, top two + the 8 best thirds, a 32-team bracket, single legs throughout;
    knockout_64    a 64-team knockout only, five two-legged rounds and a single final (the redraw rule has
                   no legs: it plays the same bracket with single matches).

    python tools/knockout_bench.py [--out DIR] [--reps N]

Reports, per format and at 1e3 / 1e4 / 1e5 simulated tournaments: the kernel time of dc_tournament_et<false>
and dc_tournament<false> from a `rocprofv3 --kernel-trace --stats` run of its own (a child process per
format and size; profiler off for the wall times), the end-to-end wall time of `simulate_tournament` under both
rules (medians of N calls after a warm-up, aggregates only) and the ratios extra time / redraw.  Writes
knockout_bench.json and knockout_bench.txt under --out (default: profiles/knockout)."""
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
sys.path[:0] = [os.path.join(ROOT, "bpl-next_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402

import tournament_bench as TB  # noqa: E402  (the model and the formats' arguments)

SIZES = (1_000, 10_000, 100_000)
FORMATS = {"world_cup_48": None, "knockout_64": (2, 2, 2, 2, 2, 1)}
# the overall-order kernels of the two rules as rocprofv3 names them; neither name is a part of the other
KERNELS = {"extra_time": "dc_tournament_et<false>", "redraw": "dc_tournament<false>"}


def calls(fmt, n):
    """{rule: a call of simulate_tournament with n simulations} on one model (one device context)."""
    m, conf = TB.model()
    kw = TB.arguments(fmt, m, conf)
    rules = {"extra_time": dict(knockout_rule="extra_time", legs=FORMATS[fmt]), "redraw": {}}
    return {rule: (lambda seed, extra=extra: m.simulate_tournament(num_simulations=n, random_state=seed, **kw, **extra))
            for rule, extra in rules.items()}


def wall_times(fmt, n, reps):
    out = {}
    for rule, call in calls(fmt, n).items():
        call(1)   # warm-up: context, upload, code object
        ts = []
        for r in range(reps):
            t0 = time.perf_counter()
            call(2 + r)
            ts.append(time.perf_counter() - t0)
        out[rule] = {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * float(np.min(ts)),
                     "max_ms": 1e3 * float(np.max(ts)), "reps": reps}
    return out


def kernel_times(fmt, n, reps):
    """Both instantiations' mean duration over the calls of a child run under rocprofv3 (its output goes to a
    temporary directory, removed afterwards)."""
    d = tempfile.mkdtemp(prefix=f"knockout_rocprof_{n}_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--child", f"{fmt}:{n}", "--reps", str(reps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise RuntimeError(f"rocprofv3 run for {fmt} {n} exited {r.returncode}: {r.stderr[-2000:]}")
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    for rule, name in KERNELS.items():
                        if name in row["Name"]:
                            out[rule] = {"calls": int(row["Calls"]), "mean_us": float(row["AverageNs"]) / 1e3,
                                         "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
        if set(out) != set(KERNELS):
            raise RuntimeError(f"the rocprofv3 stats of the {fmt} {n} run hold {sorted(out)}, not {sorted(KERNELS)}")
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knockout"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        fmt, n = args.child.split(":")
        wall_times(fmt, int(n), args.reps)
        return
    os.makedirs(args.out, exist_ok=True)
    res = {"setup": f"World-Cup model, {TB.T} teams, {len(TB.CONFS)} confederations, one host, S = {TB.S} draws",
           "formats": {}}
    lines = [res["setup"]]
    for fmt, legs in FORMATS.items():
        lines.append(f"{fmt}: legs {'single' if legs is None else legs} under the extra-time rule")
        res["formats"][fmt] = {"legs": legs, "sizes": {}}
        for n in SIZES:
            wall, kern = wall_times(fmt, n, args.reps), kernel_times(fmt, n, args.reps)
            ratio = {"kernel": kern["extra_time"]["mean_us"] / kern["redraw"]["mean_us"],
                     "wall": wall["extra_time"]["median_ms"] / wall["redraw"]["median_ms"]}
            res["formats"][fmt]["sizes"][str(n)] = {"wall": wall, "kernel": kern, "ratio": ratio}
            lines.append(f"  {n:>7} tournaments: dc_tournament extra time {kern['extra_time']['mean_us']:9.1f} us, redraw "
                         f"{kern['redraw']['mean_us']:9.1f} us: x {ratio['kernel']:.2f}; simulate_tournament end to end "
                         f"{wall['extra_time']['median_ms']:.3f} ms v {wall['redraw']['median_ms']:.3f} ms: "
                         f"x {ratio['wall']:.2f} (medians of {args.reps})")
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(args.out, "knockout_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(args.out, "knockout_bench.txt"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
