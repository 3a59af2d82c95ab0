"""loo_scores on one MI355X at the World-Cup case of tools/loglik_bench.py (200 teams, 6 confederations, S = 4000
draws), max_goals = 15, at two sizes: its first 380 fixtures and all 40 000, beside the two kernels it combines.

    python tools/loo_scores_bench.py [--out DIR] [--reps N]

Reports per size: the kernel times of `loo_forecast`, `loglik_summary` and `outcome_tiles` from one
`rocprofv3 --kernel-trace --stats` run of its own (a child process that makes the three device calls in turn;
profiler off for the wall times); the end-to-end wall time of the device call (HipContext.loo_scores: H2D +
kernel + D2H, median of N after a warm-up that also builds the team-major copies) and of the public
`loo_scores(data)`; and, once, the numpy restatement (tests/loo_scores_ref.py) on the first --ref-fixtures
fixtures, its time scaled to the others (it holds every draw's full grid), with the largest differences to the
device.  Writes loo_scores_bench.json and loo_scores_bench.txt under --out (default: profiles/loo_scores)."""
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
SIZES = (380, 40_000)
KERNELS = ("loo_forecast", "loglik_summary", "outcome_tiles")


def sized(n):
    m, data = case("world_cup")
    return m, {key: v[:n] for key, v in data.items()}


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * float(np.min(ts)),
            "max_ms": 1e3 * float(np.max(ts)), "reps": reps}


def kernel_times(n, reps):
    d = tempfile.mkdtemp(prefix=f"loo_scores_rocprof_{n}_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--child", str(n), "--reps", str(reps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
        if r.returncode != 0:
            raise RuntimeError(f"the rocprofv3 run for {n} fixtures exited {r.returncode}: {r.stderr[-2000:]}")
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


def numpy_yardstick(m, data, got, k):
    import loo_scores_ref as OR

    sub = {key: v[:k] for key, v in data.items()}
    t0 = time.perf_counter()
    ref = OR.scores(m, sub, G)
    seconds = time.perf_counter() - t0
    fin = np.isfinite(ref["elpd_loo"])
    pit = np.concatenate([got["pit_home"][:k], got["pit_away"][:k]], axis=1)
    return {"fixtures": k, "seconds": seconds,
            "max_abs_diff_outcome_proba": float(np.max(np.abs(ref["proba"] - got["outcome_proba"][:k]))),
            "max_abs_diff_pit": float(np.max(np.abs(ref["pit"] - pit))),
            "max_abs_diff_elpd_loo_i": float(np.max(np.abs(ref["elpd_loo"][fin] - got["elpd_loo_i"][:k][fin]))),
            "minus_inf_fixtures": int((~fin).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loo_scores"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ref-fixtures", type=int, default=100)
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        m, data = sized(args.child)
        (_, device, kw), = m._loglik_groups(data)[0]
        dev = device()
        for _ in range(args.reps + 1):
            dev.loo_scores(**kw, max_goals=G)
            dev.loglik_summary(**kw)
            dev.outcome_scores(**kw, max_goals=G)
        return
    os.makedirs(args.out, exist_ok=True)
    res, lines = {"draws": S, "max_goals": G, "r_eff": 1.0, "sizes": {}}, []
    for n in SIZES:
        m, data = sized(n)
        (_, device, kw), = m._loglik_groups(data)[0]
        dev = device()
        wall = {"device_call": timed(lambda: dev.loo_scores(**kw, max_goals=G), args.reps),
                "loo_scores": timed(lambda: m.loo_scores(data, max_goals=G), args.reps),
                "loglik_summary_call": timed(lambda: dev.loglik_summary(**kw), args.reps),
                "outcome_scores_call": timed(lambda: dev.outcome_scores(**kw, max_goals=G), args.reps)}
        kern = kernel_times(n, args.reps)
        got = m.loo_scores(data, max_goals=G)
        entry = {"fixtures": n, "wall": wall, "kernel": kern,
                 "scores": {key: got[key] for key in ("rps", "brier", "log_score")}, "in_sample": got["in_sample"],
                 "elpd_loo": got["elpd_loo"], "unreliable_fixtures": int((~got["reliable"]).sum())}
        t = kern["loo_forecast"]
        parts = kern["loglik_summary"]["mean_us"] + kern["outcome_tiles"]["mean_us"]
        lines += [
            f"world_cup: {len(m.teams)} teams, {n} fixtures, S = {S} draws, max_goals = {G}, r_eff = 1",
            f"  loo_forecast kernel {t['mean_us']:.1f} us (min {t['min_us']:.1f}, max {t['max_us']:.1f}, {t['calls']} calls)"
            f" = {n * S / t['mean_us'] / 1e3:.2f} G draw-fixtures/s; in the same run loglik_summary "
            f"{kern['loglik_summary']['mean_us']:.1f} us and outcome_tiles {kern['outcome_tiles']['mean_us']:.1f} us "
            f"(together {parts:.1f} us, {t['mean_us'] / parts:.2f}x)",
            f"  device call {wall['device_call']['median_ms']:.3f} ms end to end, loo_scores(data) "
            f"{wall['loo_scores']['median_ms']:.3f} ms; the loglik_summary call {wall['loglik_summary_call']['median_ms']:.3f} ms, "
            f"the outcome_scores call {wall['outcome_scores_call']['median_ms']:.3f} ms (medians of {args.reps})",
            f"  rps {got['rps']:.5f} leave-one-out against {got['in_sample']['rps']:.5f} in sample; log score "
            f"{got['log_score']:.5f} against {got['in_sample']['log_score']:.5f}; {entry['unreliable_fixtures']} fixtures "
            f"with pareto_k > 0.7"]
        if n == SIZES[0]:
            ref = entry["numpy"] = numpy_yardstick(m, data, got, min(args.ref_fixtures, n))
            lines.append(
                f"  numpy restatement on the first {ref['fixtures']} fixtures {ref['seconds']:.2f} s, scaled to {SIZES[1]}: "
                f"{ref['seconds'] * SIZES[1] / ref['fixtures']:.0f} s (not run at that shape); max |difference| of "
                f"outcome_proba {ref['max_abs_diff_outcome_proba']:.2e}, of the transform {ref['max_abs_diff_pit']:.2e}, of "
                f"elpd_loo_i {ref['max_abs_diff_elpd_loo_i']:.2e} ({ref['minus_inf_fixtures']} fixtures with a clipped tau)")
        res["sizes"][str(n)] = entry
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(args.out, "loo_scores_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(args.out, "loo_scores_bench.txt"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
