"""simulate_tournament on one MI355X: the 48-team World Cup format (12 groups of 4, top two + the 8 best
thirds, a 32-team bracket), the Euro format (6 groups of 4, top two + the 4 best thirds) and a 64-team
knockout only, on the World-Cup model (confederations, one host) with S = 1000 posterior draws, at
1e3 / 1e4 / 1e5 simulated tournaments.

    python tools/tournament_bench.py [--out DIR] [--reps N]

Reports, per format and size: the end-to-end wall time of `simulate_tournament` (median of N calls after
a warm-up; H2D + kernel + D2H + host post-processing, no per-simulation stages) and the kernel time of
`dc_tournament` from a `rocprofv3 --kernel-trace --stats` run of its own (a child process per format and
size, profiler off for the wall times); and the numpy restatement (tests/tournament_ref.py) at 1e3 for
scale.  Writes tournament_bench.json and tournament_bench.txt under --out (default: profiles/tournament)."""
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

import tournament_ref as R  # noqa: E402

SIZES = (1_000, 10_000, 100_000)
FORMATS = ("world_cup_48", "euro_24", "knockout_64")
S, T = 1000, 64
CONFS = np.array(["AFC", "CAF", "CONCACAF", "CONMEBOL", "OFC", "UEFA"])


def model():
    from bpl import NeutralDixonColesMatchPredictorWC

    rs = np.random.RandomState(0)
    m = NeutralDixonColesMatchPredictorWC()
    m.teams = np.array([f"t{i:02d}" for i in range(T)])
    m._teams_dict = {t: i for i, t in enumerate(m.teams)}
    m.attack, m.defence = rs.normal(0, 0.4, (S, T)), rs.normal(0, 0.4, (S, T))
    for nm in ("home_attack", "away_attack", "home_defence", "away_defence"):
        setattr(m, nm, rs.normal(0, 0.1, (S, T)))
    m.corr_coef = rs.uniform(-0.1, 0.05, S)
    m.conferences = CONFS
    m._conferences_dict = {c: i for i, c in enumerate(CONFS)}
    m.confederation_strength = rs.normal(0, 0.3, (S, len(CONFS)))
    conf = {t: CONFS[i % len(CONFS)] for i, t in enumerate(m.teams)}
    return m, conf


def arguments(fmt, m, conf):
    kw = getattr(R, fmt)(list(m.teams))
    return dict(kw, hosts=[m.teams[0]], team_conf=conf)


def wall_times(fmt, sizes, reps):
    m, conf = model()
    kw = arguments(fmt, m, conf)
    out = {}
    for n in sizes:
        m.simulate_tournament(num_simulations=n, random_state=1, **kw)   # warm-up: context, upload, code object
        ts = []
        for r in range(reps):
            t0 = time.perf_counter()
            m.simulate_tournament(num_simulations=n, random_state=2 + r, **kw)
            ts.append(time.perf_counter() - t0)
        out[n] = {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * float(np.min(ts)),
                  "max_ms": 1e3 * float(np.max(ts)), "reps": reps}
    return out


def kernel_time(fmt, n, reps):
    """dc_tournament's mean duration over the calls of a child run under rocprofv3 (its output goes to a
    temporary directory, removed afterwards)."""
    d = tempfile.mkdtemp(prefix=f"tournament_rocprof_{n}_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--child", f"{fmt}:{n}", "--reps", str(reps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise RuntimeError(f"rocprofv3 run for {fmt} {n} exited {r.returncode}: {r.stderr[-2000:]}")
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    if "dc_tournament" in row["Name"]:
                        return {"calls": int(row["Calls"]), "mean_us": float(row["AverageNs"]) / 1e3,
                                "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
        raise RuntimeError(f"no dc_tournament row in the rocprofv3 stats of the {fmt} {n} run")
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tournament"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        fmt, n = args.child.split(":")
        wall_times(fmt, [int(n)], args.reps)
        return
    os.makedirs(args.out, exist_ok=True)
    res = {"setup": f"World-Cup model, {T} teams, {len(CONFS)} confederations, one host, S = {S} draws",
           "formats": {}}
    lines = [res["setup"]]
    m, conf = model()
    for fmt in FORMATS:
        wall = wall_times(fmt, SIZES, args.reps)
        kern = {n: kernel_time(fmt, n, args.reps) for n in SIZES}
        kw = arguments(fmt, m, conf)
        inp = m._tournament_inputs(kw["knockout"], kw.get("groups"), kw.get("advance", 2), kw.get("best_of_rest", 0),
                                   None, None, kw["hosts"], (3, 1, 0), SIZES[0], conf)
        t0 = time.perf_counter()
        R.simulate_tournament(R.model_tables(m), inp, (0, 1))
        ref_ms = 1e3 * (time.perf_counter() - t0)
        res["formats"][fmt] = {"group_fixtures": int(inp["fix_p"].size), "bracket": 1 << inp["rounds"],
                               "wall": {str(k): v for k, v in wall.items()},
                               "kernel": {str(k): v for k, v in kern.items()}, "numpy_restatement_1e3_ms": ref_ms}
        lines.append(f"{fmt}: {inp['fix_p'].size} group fixtures, a {1 << inp['rounds']}-team bracket")
        for n in SIZES:
            k, w = kern[n], wall[n]
            lines.append(f"  {n:>7} tournaments: dc_tournament {k['mean_us']:9.1f} us (min {k['min_us']:.1f}, max "
                         f"{k['max_us']:.1f}, {k['calls']} calls) = {n / k['mean_us']:.2f} M tournaments/s; "
                         f"simulate_tournament {w['median_ms']:.3f} ms end to end (median of {w['reps']}, "
                         f"min {w['min_ms']:.3f})")
        lines.append(f"  numpy restatement, {SIZES[0]} tournaments: {ref_ms:.0f} ms")
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(args.out, "tournament_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(args.out, "tournament_bench.txt"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
