"""tournament_paths on one MI355X (csrc/dc_paths.hip.h) at the World Cup case: N = 100 000 simulations of 48 teams
(12 groups of 4, 72 group fixtures, a 32-team bracket) over 1000 posterior draws.

    python tools/paths_bench.py [--out DIR] [--reps N] [--sims N]

Reports: the kernel times of the recording stage `dc_paths_sim`, of the counting kernels `dc_leverage_count` and
`dc_paths_count` (summed over the chunks of a call) and of `dc_tournament` at the same shape, from a `rocprofv3
--kernel-trace --stats` run of its own (a child process; profiler off for the wall times); the end-to-end wall time
of the device call (HipContext.tournament_paths: H2D + kernels + D2H) and of the public `tournament_paths` (medians
of N after a warm-up); and the only other route to the tables: `tournament_paths(return_records=True)` plus the numpy
cross-tabulation of tests/paths_ref.py, whose tables must equal the device's.  The figures of merit are the two
ratios recording stage / dc_tournament and counting / recording stage, taken in the same run.  Writes
paths_bench.json and paths_bench.txt under --out (default: profiles/paths)."""
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

S, T, SEED = 1000, 64, 31337
KERNELS = ("dc_paths_sim", "dc_leverage_count", "dc_paths_count", "dc_tournament")
TABLES = ("stage_count", "advance_count", "meet_count", "position_stage_count", "outcome_count", "target_count",
          "joint_count")


def world_cup():
    """(model with a hand-built posterior, simulate_tournament kwargs): the shape of tools/tournament_bench.py."""
    import tournament_ref as R
    from bpl import NeutralDixonColesMatchPredictor

    rs = np.random.RandomState(9)
    m = NeutralDixonColesMatchPredictor()
    m.teams = np.array([f"t{i:02d}" for i in range(T)])
    m._teams_dict = {t: i for i, t in enumerate(m.teams)}
    m.attack, m.defence = rs.normal(0, 0.3, (S, T)), rs.normal(0, 0.3, (S, T))
    for nm in ("home_attack", "away_attack", "home_defence", "away_defence"):
        setattr(m, nm, rs.normal(0, 0.1, (S, T)))
    m.corr_coef = rs.uniform(-0.05, 0.05, S)
    return m, R.world_cup_48(list(m.teams))


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * float(np.min(ts)),
            "max_ms": 1e3 * float(np.max(ts)), "reps": reps}


def calls(n_sims):
    """(model, kwargs, the device call, simulate_tournament's device call without per-simulation outputs)."""
    m, kw = world_cup()
    _, call = m._tournament_call(kw["knockout"], kw["groups"], kw["advance"], kw["best_of_rest"], None, None, None,
                                 (3, 1, 0), n_sims, SEED, None, "overall", None, "redraw", None, 1 / 3, None, False)
    dev = m._device()
    return (m, kw, lambda: dev.tournament_paths(*call["args"], **call["kwargs"]),
            lambda: dev.simulate_tournament(*call["args"], **call["kwargs"]))


def kernel_times(n_sims, reps):
    """Per device call: the summed duration of each kernel's launches (the stages run once per chunk)."""
    d = tempfile.mkdtemp(prefix="paths_rocprof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--child", "--sims", str(n_sims), "--reps", str(reps)]
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
                            out[k] = {"launches": n, "launches_per_call": n / (reps + 1),
                                      "us_per_call": float(row["TotalDurationNs"]) / 1e3 / (reps + 1)}
        if set(out) != set(KERNELS):
            raise RuntimeError(f"the rocprofv3 stats hold {sorted(out)}, not {KERNELS}")
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paths"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--ref-reps", type=int, default=1)
    ap.add_argument("--sims", type=int, default=100_000)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    N = args.sims
    m, kw, device_call, tournament_call = calls(N)
    if args.child:
        for _ in range(args.reps + 1):
            device_call()
            tournament_call()
        return
    import paths_ref as P
    from bpl import paths

    os.makedirs(args.out, exist_ok=True)
    run = dict(num_simulations=N, random_state=SEED, **kw)
    wall = {"device_call": timed(device_call, args.reps),
            "tournament_paths": timed(lambda: m.tournament_paths(**run), args.reps),
            "simulate_tournament_aggregates_only": timed(tournament_call, args.reps)}
    inp = m._tournament_inputs(kw["knockout"], kw["groups"], kw["advance"], kw["best_of_rest"], None, None, None,
                               (3, 1, 0), N, None)
    route = {"records_s": [], "numpy_s": []}
    for _ in range(args.ref_reps + 1):          # (the first pass is the warm-up)
        t0 = time.perf_counter()
        rec = m.tournament_paths(return_records=True, **run)
        t1 = time.perf_counter()
        ref = P.counts(rec, inp)
        t2 = time.perf_counter()
        route["records_s"].append(t1 - t0)
        route["numpy_s"].append(t2 - t1)
    route = {k: float(np.median(v[1:])) for k, v in route.items()}
    route["total_s"] = route["records_s"] + route["numpy_s"]
    got = m.tournament_paths(**run)
    same = all(np.array_equal(got[k], ref[k]) for k in TABLES)
    kern = kernel_times(N, args.reps)
    counting = kern["dc_leverage_count"]["us_per_call"] + kern["dc_paths_count"]["us_per_call"]
    sim_ratio = kern["dc_paths_sim"]["us_per_call"] / kern["dc_tournament"]["us_per_call"]
    count_ratio = counting / kern["dc_paths_sim"]["us_per_call"]
    ratio = route["total_s"] * 1e3 / wall["tournament_paths"]["median_ms"]
    final = paths.most_likely_final(got)
    res = {"simulations": N, "draws": S, "teams": 48, "fixtures": int(inp["fix_p"].size), "rounds": int(inp["rounds"]),
           "wall": wall, "kernel": kern, "sim_over_tournament_kernel_time": sim_ratio,
           "count_over_sim_kernel_time": count_ratio, "records_route": route,
           "records_route_over_tournament_paths": ratio, "tables_equal_the_numpy_route": bool(same)}
    lines = [
        f"World Cup: {N} simulations x 48 teams x {inp['fix_p'].size} group fixtures x {inp['rounds']} rounds, "
        f"{S} draws",
        f"  dc_paths_sim {kern['dc_paths_sim']['us_per_call']:.1f} us per call "
        f"({kern['dc_paths_sim']['launches_per_call']:.0f} launches), dc_tournament at the same shape (aggregates "
        f"only) {kern['dc_tournament']['us_per_call']:.1f} us: recording / dc_tournament = {sim_ratio:.2f}",
        f"  dc_leverage_count {kern['dc_leverage_count']['us_per_call']:.1f} us + dc_paths_count "
        f"{kern['dc_paths_count']['us_per_call']:.1f} us per call: counting / recording = {count_ratio:.2f}",
        f"  device call {wall['device_call']['median_ms']:.3f} ms end to end, tournament_paths(...) "
        f"{wall['tournament_paths']['median_ms']:.3f} ms, simulate_tournament device call (aggregates only) "
        f"{wall['simulate_tournament_aggregates_only']['median_ms']:.3f} ms (medians of {args.reps})",
        f"  from the records: tournament_paths(return_records=True) {route['records_s']:.3f} s + numpy "
        f"cross-tabulation {route['numpy_s']:.3f} s = {route['total_s']:.3f} s: {ratio:.1f} x tournament_paths; "
        f"tables equal: {same}",
        f"  most likely final: {final[0]} v {final[1]}, {final[2]:.4f}"]
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(args.out, "paths_bench.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.join(args.out, "paths_bench.txt"), "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
