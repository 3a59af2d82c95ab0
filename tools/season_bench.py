"""simulate_season on one MI355X: 20 teams, a 380-fixture double round robin, S = 1000 posterior draws,
1e3 / 1e4 / 1e5 simulated seasons.

    python tools/season_bench.py [--out DIR] [--reps N]

Reports, per size: the end-to-end wall time of `simulate_season` (median of N calls after a warm-up;
H2D + kernel + D2H + host post-processing, no optional outputs) and the kernel time of `dc_season`
from a `rocprofv3 --kernel-trace --stats` run of its own (a child process per size, profiler off for
the wall times); and the numpy restatement (tests/season_ref.py) at 1e3 for scale.  Writes
season_bench.json and season_bench.txt under --out (default: profiles/season)."""
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

SIZES = (1_000, 10_000, 100_000)
S, T = 1000, 20


def model():
    from bpl import DixonColesMatchPredictor

    rs = np.random.RandomState(0)
    m = DixonColesMatchPredictor()
    m.teams = np.array([f"t{i:02d}" for i in range(T)])
    m._teams_dict = {t: i for i, t in enumerate(m.teams)}
    m.attack, m.defence = rs.normal(0, 0.3, (S, T)), rs.normal(0, 0.3, (S, T))
    m.home_advantage, m.corr_coef = rs.normal(0.25, 0.05, S), rs.uniform(-0.1, 0.05, S)
    h, a = np.nonzero(~np.eye(T, dtype=bool))
    return m, h.astype(np.uint16), a.astype(np.uint16)


def wall_times(sizes, reps):
    m, h, a = model()
    out = {}
    for n in sizes:
        m.simulate_season(h, a, num_simulations=n, random_state=1)   # warm-up: context, upload, code object
        ts = []
        for r in range(reps):
            t0 = time.perf_counter()
            m.simulate_season(h, a, num_simulations=n, random_state=2 + r)
            ts.append(time.perf_counter() - t0)
        out[n] = {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * float(np.min(ts)),
                  "max_ms": 1e3 * float(np.max(ts)), "reps": reps}
    return out


def kernel_time(n, reps):
    """dc_season's mean duration over the calls of a child run under rocprofv3 (its output goes to a
    temporary directory, removed afterwards)."""
    d = tempfile.mkdtemp(prefix=f"season_rocprof_{n}_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--child", str(n), "--reps", str(reps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise RuntimeError(f"rocprofv3 run for {n} exited {r.returncode}: {r.stderr[-2000:]}")
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    if "dc_season" in row["Name"]:
                        return {"calls": int(row["Calls"]), "mean_us": float(row["AverageNs"]) / 1e3,
                                "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
        raise RuntimeError(f"no dc_season row in the rocprofv3 stats of the {n}-season run")
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "season"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        wall_times([args.child], args.reps)
        return
    os.makedirs(args.out, exist_ok=True)
    res = {"setup": f"{T} teams, {T * (T - 1)} fixtures, S = {S} draws, basic model", "wall": {}, "kernel": {}}
    res["wall"] = {str(k): v for k, v in wall_times(SIZES, args.reps).items()}
    for n in SIZES:
        res["kernel"][str(n)] = kernel_time(n, args.reps)
    import season_ref as R

    m, h, a = model()
    t0 = time.perf_counter()
    R.simulate_season(m.attack, m.defence, m.home_advantage, m.corr_coef, h, a, np.arange(T), np.zeros((T, 3)),
                      (3, 1, 0), SIZES[0], (0, 1))
    res["numpy_restatement_1e3_ms"] = 1e3 * (time.perf_counter() - t0)
    lines = [res["setup"]]
    for n in SIZES:
        k, w = res["kernel"][str(n)], res["wall"][str(n)]
        samples = n * T * (T - 1)
        lines.append(f"{n:>7} seasons: dc_season {k['mean_us']:9.1f} us (min {k['min_us']:.1f}, max {k['max_us']:.1f}, "
                     f"{k['calls']} calls) = {samples / k['mean_us'] / 1e3:.2f} G scorelines/s; simulate_season "
                     f"{w['median_ms']:.3f} ms end to end (median of {w['reps']}, min {w['min_ms']:.3f})")
    lines.append(f"numpy restatement, {SIZES[0]} seasons: {res['numpy_restatement_1e3_ms']:.0f} ms")
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(args.out, "season_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(args.out, "season_bench.txt"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
