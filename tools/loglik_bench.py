"""PSIS-LOO on one MI355X: the `loglik_summary` kernel (csrc/dc_loglik.hip.h) for two cases, with the float64
numpy restatement (tests/loglik_ref.py) on the same inputs as the CPU yardstick.

    league      Dixon-Coles, 20 teams, the 380 fixtures of a double round robin, S = 4000 draws
    world_cup   World-Cup model, 200 teams, 6 confederations, 40 000 fixtures (half neutral), S = 4000 draws

    python tools/loglik_bench.py [--out DIR] [--reps N]

Reports per case: the kernel time of `loglik_summary` from a `rocprofv3 --kernel-trace --stats` run of its own
(a child process, profiler off for the wall times), the end-to-end wall time of the device call
(HipContext.loglik_summary: H2D + kernel + D2H, median of N after a warm-up that also builds the team-major
copies) and of the public `loo(data)` (host checks and name lookups included), and the numpy restatement's
time for the ll matrix plus PSIS, with the largest difference of elpd_loo_i between the two.  Writes
loglik_bench.json and loglik_bench.txt under --out (default: profiles/loglik)."""
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

S = 4000
CASES = ("league", "world_cup")


def case(name):
    """(model, data) of a case, from fixed seeds."""
    rs = np.random.RandomState(0)
    if name == "league":
        from bpl import DixonColesMatchPredictor

        T = 20
        m = DixonColesMatchPredictor()
        m.teams = np.array([f"t{i:02d}" for i in range(T)])
        m._teams_dict = {t: i for i, t in enumerate(m.teams)}
        m.attack, m.defence = rs.normal(0, 0.3, (S, T)), rs.normal(0, 0.3, (S, T))
        m.home_advantage, m.corr_coef = rs.normal(0.25, 0.05, S), rs.uniform(-0.1, 0.05, S)
        h, a = np.nonzero(~np.eye(T, dtype=bool))
        n = h.size
        data = {"home_team": list(m.teams[h]), "away_team": list(m.teams[a])}
    else:
        from bpl import NeutralDixonColesMatchPredictorWC

        T, C, n = 200, 6, 40_000
        m = NeutralDixonColesMatchPredictorWC()
        m.teams = np.array([f"t{i:03d}" for i in range(T)])
        m._teams_dict = {t: i for i, t in enumerate(m.teams)}
        m.attack, m.defence = rs.normal(0, 0.4, (S, T)), rs.normal(0, 0.4, (S, T))
        for nm in ("home_attack", "away_attack", "home_defence", "away_defence"):
            setattr(m, nm, rs.normal(0, 0.1, (S, T)))
        m.corr_coef = rs.uniform(-0.1, 0.05, S)
        m.conferences = np.array(["AFC", "CAF", "CONCACAF", "CONMEBOL", "OFC", "UEFA"])
        m._conferences_dict = {c: i for i, c in enumerate(m.conferences)}
        m.confederation_strength = rs.normal(0, 0.3, (S, C))
        h = rs.randint(0, T, n)
        a = (h + 1 + rs.randint(0, T - 1, n)) % T
        conf = m.conferences[np.arange(T) % C]
        data = {"home_team": list(m.teams[h]), "away_team": list(m.teams[a]), "neutral_venue": rs.randint(0, 2, n),
                "home_conf": list(conf[h]), "away_conf": list(conf[a])}
    data["home_goals"], data["away_goals"] = rs.poisson(1.5, n), rs.poisson(1.1, n)
    return m, data


def wall_times(name, reps):
    m, data = case(name)
    groups, _ = m._loglik_groups(data)
    (_, device, kw), = groups
    dev = device()
    dev.loglik_summary(**kw)   # warm-up: context, upload, team-major copies, code object
    out = {}
    for label, fn in (("device_call", lambda: dev.loglik_summary(**kw)), ("loo", lambda: m.loo(data))):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        out[label] = {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * float(np.min(ts)),
                      "max_ms": 1e3 * float(np.max(ts)), "reps": reps}
    return out


def kernel_time(name, reps):
    """loglik_summary's mean duration over the calls of a child run under rocprofv3 (output in a
    temporary directory, removed afterwards)."""
    d = tempfile.mkdtemp(prefix=f"loglik_rocprof_{name}_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(reps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
        if r.returncode != 0:
            raise RuntimeError(f"rocprofv3 run for {name} exited {r.returncode}: {r.stderr[-2000:]}")
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    for k in ("loglik_summary", "transpose_f64"):
                        if k in row["Name"]:
                            out[k] = {"calls": int(row["Calls"]), "mean_us": float(row["AverageNs"]) / 1e3,
                                      "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
        if "loglik_summary" not in out:
            raise RuntimeError(f"no loglik_summary row in the rocprofv3 stats of the {name} run")
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def numpy_yardstick(name, gpu_elpd):
    import loglik_ref as R

    m, data = case(name)
    t0 = time.perf_counter()
    ll = R.ll_matrix(m, data)
    t1 = time.perf_counter()
    ref = R.summary(ll, 1.0)
    t2 = time.perf_counter()
    fin = np.isfinite(ref["elpd_loo"])
    return {"ll_matrix_s": t1 - t0, "psis_s": t2 - t1, "total_s": t2 - t0,
            "max_abs_diff_elpd_loo_i": float(np.max(np.abs(ref["elpd_loo"][fin] - gpu_elpd[fin]))),
            "minus_inf_fixtures": int((~fin).sum()),
            "minus_inf_agree": bool(np.array_equal(ref["elpd_loo"][~fin], gpu_elpd[~fin]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loglik"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        m, data = case(args.child)
        (_, device, kw), = m._loglik_groups(data)[0]
        dev = device()
        for _ in range(args.reps + 1):
            dev.loglik_summary(**kw)
        return
    os.makedirs(args.out, exist_ok=True)
    res, lines = {"draws": S, "r_eff": 1.0, "cases": {}}, []
    for name in CASES:
        m, data = case(name)
        n = len(data["home_goals"])
        wall = wall_times(name, args.reps)
        kern = kernel_time(name, args.reps)
        gpu = m.loo(data)
        ref = numpy_yardstick(name, gpu["elpd_loo_i"])
        k = kern["loglik_summary"]
        res["cases"][name] = {"fixtures": n, "teams": len(m.teams), "wall": wall, "kernel": kern, "numpy": ref,
                              "elpd_loo": gpu["elpd_loo"], "max_pareto_k": float(np.max(gpu["pareto_k"]))}
        lines.append(f"{name}: {len(m.teams)} teams, {n} fixtures, S = {S} draws, PSIS on (r_eff = 1)")
        lines.append(f"  loglik_summary kernel {k['mean_us']:.1f} us (min {k['min_us']:.1f}, max {k['max_us']:.1f}, "
                     f"{k['calls']} calls) = {n * S / k['mean_us'] / 1e3:.2f} G draw-fixtures/s")
        lines.append(f"  device call {wall['device_call']['median_ms']:.3f} ms end to end, loo(data) "
                     f"{wall['loo']['median_ms']:.3f} ms (medians of {args.reps})")
        lines.append(f"  numpy restatement: ll matrix {ref['ll_matrix_s']:.3f} s + PSIS {ref['psis_s']:.3f} s = "
                     f"{ref['total_s']:.3f} s; {ref['total_s'] * 1e3 / wall['device_call']['median_ms']:.0f}x the "
                     f"device call; max |elpd_loo_i difference| {ref['max_abs_diff_elpd_loo_i']:.2e} over the finite ones, "
                     f"{ref['minus_inf_fixtures']} fixtures with a clipped tau (elpd_loo_i = -inf) "
                     f"{'in both' if ref['minus_inf_agree'] else 'NOT MATCHING'}")
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(args.out, "loglik_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(args.out, "loglik_bench.txt"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
