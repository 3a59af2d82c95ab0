"""forecast_scores on one MI355X at the World-Cup case of tools/loglik_bench.py (200 teams, 6 confederations,
40 000 fixtures, S = 4000 draws), max_goals = 15, beside the routes a user had before it.

    python tools/scores_bench.py [--out DIR] [--reps N]

Reports: the kernel times of `outcome_tiles` and `outcome_reduce` from a `rocprofv3 --kernel-trace --stats` run
of its own (a child process; profiler off for the wall times); the end-to-end wall time of the device call
(HipContext.outcome_scores: H2D + kernels + D2H, median of N after a warm-up that also builds the team-major
copies) and of the public `forecast_scores(data)`; the existing route to the MEAN forecast alone
(`predict_score_grid` at depth 15 copied to the host and reduced there with `outcome_from_grid`); and the numpy
restatement (tests/scores_ref.py) on the first --ref-fixtures fixtures, its time scaled to all of them (the full
shape is 1.6e8 grids of 256 cells).  Writes scores_bench.json and scores_bench.txt under --out (default:
profiles/scores)."""
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

from loglik_bench import S, case  # noqa: E402

G = 15
KERNELS = ("outcome_tiles", "outcome_reduce")


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * float(np.min(ts)),
            "max_ms": 1e3 * float(np.max(ts)), "reps": reps}


def kernel_times(reps):
    d = tempfile.mkdtemp(prefix="scores_rocprof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
        if r.returncode != 0:
            raise RuntimeError(f"the rocprofv3 run exited {r.returncode}: {r.stderr[-2000:]}")
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    for k in KERNELS:
                        if k in row["Name"]:
                            out[k] = {"calls": int(row["Calls"]), "mean_us": float(row["AverageNs"]) / 1e3,
                                      "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
        if set(out) != set(KERNELS):
            raise RuntimeError(f"the rocprofv3 stats hold {sorted(out)}, not {KERNELS}")
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scores"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ref-fixtures", type=int, default=400)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    m, data = case("world_cup")
    n = len(data["home_goals"])
    (_, device, kw), = m._loglik_groups(data)[0]
    dev = device()
    if args.child:
        for _ in range(args.reps + 1):
            dev.outcome_scores(**kw, max_goals=G)
        return
    from bpl.base import outcome_from_grid

    os.makedirs(args.out, exist_ok=True)
    wall = {"device_call": timed(lambda: dev.outcome_scores(**kw, max_goals=G), args.reps),
            "forecast_scores": timed(lambda: m.forecast_scores(data, max_goals=G), args.reps)}

    def grid_route():
        grid = dev.predict_score_grid(kw["home_idx"], kw["away_idx"], G, neutral=kw["neutral"], conf=kw["conf"])
        return outcome_from_grid(grid)

    wall["grid_route_mean_forecast_only"] = timed(grid_route, max(3, args.reps // 3))
    kern = kernel_times(args.reps)
    got = m.forecast_scores(data, max_goals=G)
    g = grid_route()
    grid_diff = float(np.max(np.abs(got["outcome_proba"] - np.stack([g["home_win"], g["draw"], g["away_win"]], axis=1))))

    import scores_ref as SR

    k = args.ref_fixtures
    sub = {key: v[:k] for key, v in data.items()}
    t0 = time.perf_counter()
    ref = SR.scores(m, sub, G)
    ref_s = time.perf_counter() - t0
    diff = float(np.max(np.abs(ref["outcome_proba"] - got["outcome_proba"][:k])))

    pairs = n * S
    t = kern["outcome_tiles"]
    res = {"draws": S, "fixtures": n, "max_goals": G, "wall": wall, "kernel": kern,
           "numpy": {"fixtures": k, "seconds": ref_s, "scaled_to_all_fixtures_s": ref_s * n / k,
                     "max_abs_diff_outcome_proba": diff},
           "grid_route_max_abs_diff_outcome_proba": grid_diff,
           "scores": {key: got[key] for key in ("rps", "brier", "log_score", "rps_se", "brier_se", "log_score_se")},
           "rps_draws_quantiles_5_50_95": [float(q) for q in np.quantile(got["rps_draws"], [0.05, 0.5, 0.95])]}
    lines = [
        f"world_cup: {len(m.teams)} teams, {n} fixtures, S = {S} draws, max_goals = {G}",
        f"  outcome_tiles kernel {t['mean_us']:.1f} us (min {t['min_us']:.1f}, max {t['max_us']:.1f}, {t['calls']} calls)"
        f" = {pairs / t['mean_us'] / 1e3:.1f} G draw-fixtures/s; outcome_reduce {kern['outcome_reduce']['mean_us']:.1f} us",
        f"  device call {wall['device_call']['median_ms']:.3f} ms end to end, forecast_scores(data) "
        f"{wall['forecast_scores']['median_ms']:.3f} ms (medians of {args.reps})",
        f"  existing route (predict_score_grid at depth {G} to the host + outcome_from_grid; the mean forecast only, "
        f"float32 grid) {wall['grid_route_mean_forecast_only']['median_ms']:.3f} ms; max |difference| of outcome_proba "
        f"{grid_diff:.2e}",
        f"  numpy restatement on the first {k} fixtures {ref_s:.2f} s, scaled to {n}: {ref_s * n / k:.0f} s "
        f"(not run at the full shape); max |difference| of outcome_proba {diff:.2e}",
        f"  rps {got['rps']:.5f} +- {got['rps_se']:.5f}; rps of the draws: 5 % {res['rps_draws_quantiles_5_50_95'][0]:.5f}, "
        f"median {res['rps_draws_quantiles_5_50_95'][1]:.5f}, 95 % {res['rps_draws_quantiles_5_50_95'][2]:.5f}"]
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(args.out, "scores_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(args.out, "scores_bench.txt"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
