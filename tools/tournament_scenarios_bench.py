"""tournament_scenarios on one MI355X (csrc/dc_tscen.hip.h) at the World Cup case: N = 100 000 simulations of 48 teams
(12 groups of 4, 72 group fixtures, a 32-team bracket) over 1000 posterior draws, default rule, two sets of keys:
the 2 final fixtures of one group with cap 3 (49 scenarios) and 8 keys with cap 1 (6561 scenarios).

    python tools/tournament_scenarios_bench.py [--out DIR] [--reps N] [--runs N] [--sims N]

Reports, per case: the kernel time of the recording stage `dc_tscen_sim` beside `dc_paths_sim` and `dc_tournament`
at the same shape and of the counting kernel `dc_scenario_count` (summed over the chunks of a call), from `rocprofv3
--kernel-trace --stats` runs of their own (child processes, all four kernels timed in the same run; profiler off for
the wall times); the end-to-end wall time of the device call (HipContext.tournament_scenarios: H2D + kernels + D2H)
and of the public `tournament_scenarios` (medians of --reps after a warm-up); and the only other route to the tables:
`tournament_scenarios(return_records=True)` plus the numpy cross-tabulation of tests/tournament_scenarios_ref.py, whose
tables must equal the device's.  Everything is measured --runs times (default 3): the figures are the medians over the
runs, with the smallest and largest run beside them.  The figure of merit is dc_tscen_sim / dc_paths_sim.  Writes
tournament_scenarios_bench.json and tournament_scenarios_bench.txt under --out (default:
profiles/tournament_scenarios)."""
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

from paths_bench import S, SEED, timed, world_cup  # noqa: E402

KERNELS = ("dc_tscen_sim", "dc_scenario_count", "dc_paths_sim", "dc_tournament")
# positions in the default round robin: group g's fixtures are 6 g .. 6 g + 5, (0,1) (0,2) (0,3) (1,2) (1,3) (2,3);
# its final matchday is (0,3) and (1,2)
CASES = {"final_two": ([2, 3], [3, 3]),
         "eight_keys": ([6 * g + f for g in range(4) for f in (2, 3)], [1] * 8)}


def calls(n_sims, case):
    """(model, kwargs, checked inputs, the device call, tournament_paths' and simulate_tournament's device calls)."""
    m, kw = world_cup()
    inp, call = m._tournament_call(kw["knockout"], kw["groups"], kw["advance"], kw["best_of_rest"], None, None, None,
                                   (3, 1, 0), n_sims, SEED, None, "overall", None, "redraw", None, 1 / 3, None, False)
    keys, caps = CASES[case]
    dev = m._device()
    return (m, kw, inp,
            lambda: dev.tournament_scenarios(*call["args"], key_fixture=keys, key_cap=caps, **call["kwargs"]),
            lambda: dev.tournament_paths(*call["args"], **call["kwargs"]),
            lambda: dev.simulate_tournament(*call["args"], **call["kwargs"]))


def kernel_times(n_sims, reps, case):
    """Per device call: the summed duration of each kernel's launches (the stages run once per chunk)."""
    d = tempfile.mkdtemp(prefix="tscen_rocprof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--child", case, "--sims", str(n_sims), "--reps", str(reps)]
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
                            n = int(row["Calls"])
                            out[k] = {"launches_per_call": n / (reps + 1),
                                      "us_per_call": float(row["TotalDurationNs"]) / 1e3 / (reps + 1)}
        if set(out) != set(KERNELS):
            raise RuntimeError(f"the rocprofv3 stats hold {sorted(out)}, not {KERNELS}")
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def spread(values):
    v = [float(x) for x in values]
    return {"median": float(np.median(v)), "min": min(v), "max": max(v), "runs": v}


def fmt(s, unit="", digits=1):
    return f"{s['median']:.{digits}f}{unit} ({s['min']:.{digits}f} .. {s['max']:.{digits}f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tournament_scenarios"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sims", type=int, default=100_000)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    N = args.sims
    if args.child:
        _, _, _, device_call, paths_call, tournament_call = calls(N, args.child)
        for _ in range(args.reps + 1):
            device_call()
            paths_call()
            tournament_call()
        return
    import tournament_scenarios_ref as TS

    os.makedirs(args.out, exist_ok=True)
    res = {"simulations": N, "draws": S, "teams": 48, "runs": args.runs, "reps": args.reps, "cases": {}}
    lines = []
    for case, (keys, caps) in CASES.items():
        m, kw, inp, device_call, paths_call, tournament_call = calls(N, case)
        run = dict(fixtures=keys, margin_cap=caps, num_simulations=N, random_state=SEED, **kw)
        wall = {k: [] for k in ("device_call", "tournament_scenarios", "tournament_paths_device_call",
                                "simulate_tournament_device_call", "records_s", "numpy_s")}
        kern = []
        same = True
        for _ in range(args.runs):
            wall["device_call"].append(timed(device_call, args.reps)["median_ms"])
            wall["tournament_scenarios"].append(timed(lambda: m.tournament_scenarios(**run), args.reps)["median_ms"])
            wall["tournament_paths_device_call"].append(timed(paths_call, args.reps)["median_ms"])
            wall["simulate_tournament_device_call"].append(timed(tournament_call, args.reps)["median_ms"])
            m.tournament_scenarios(return_records=True, **run)          # (the warm-up of the route below)
            t0 = time.perf_counter()
            rec = m.tournament_scenarios(return_records=True, **run)
            t1 = time.perf_counter()
            ref = TS.counts(rec, inp, keys, caps)
            t2 = time.perf_counter()
            wall["records_s"].append(t1 - t0)
            wall["numpy_s"].append(t2 - t1)
            got = m.tournament_scenarios(**run)
            same = same and all(np.array_equal(got[k], ref[k]) for k in ("scenario_count", "joint_count"))
            kern.append(kernel_times(N, args.reps, case))
        wall = {k: spread(v) for k, v in wall.items()}
        kernel = {k: spread([r[k]["us_per_call"] for r in kern]) for k in KERNELS}
        launches = {k: kern[0][k]["launches_per_call"] for k in KERNELS}
        over_paths = spread([r["dc_tscen_sim"]["us_per_call"] / r["dc_paths_sim"]["us_per_call"] for r in kern])
        over_tournament = spread([r["dc_tscen_sim"]["us_per_call"] / r["dc_tournament"]["us_per_call"] for r in kern])
        count_share = spread([r["dc_scenario_count"]["us_per_call"] / r["dc_tscen_sim"]["us_per_call"] for r in kern])
        route = spread([a + b for a, b in zip(wall["records_s"]["runs"], wall["numpy_s"]["runs"])])
        ratio = route["median"] * 1e3 / wall["tournament_scenarios"]["median"]
        occurred = int((got["scenario_count"] > 0).sum())
        res["cases"][case] = {
            "fixtures": keys, "margin_cap": caps, "scenarios": int(got["scenario_count"].size), "occurred": occurred,
            "kernel_us_per_call": kernel, "launches_per_call": launches,
            "tscen_sim_over_paths_sim": over_paths, "tscen_sim_over_tournament": over_tournament,
            "count_over_tscen_sim": count_share, "wall_ms": {k: v for k, v in wall.items() if not k.endswith("_s")},
            "records_route_s": {"records": wall["records_s"], "numpy": wall["numpy_s"], "total": route},
            "records_route_over_tournament_scenarios": ratio, "tables_equal_the_numpy_route": bool(same)}
        lines += [
            f"{case}: {len(keys)} key fixtures {keys} with caps {caps}, {got['scenario_count'].size} scenarios, "
            f"{occurred} of them occurred",
            f"  dc_tscen_sim {fmt(kernel['dc_tscen_sim'], ' us')} per call ({launches['dc_tscen_sim']:.0f} launches); "
            f"same run: dc_paths_sim {fmt(kernel['dc_paths_sim'], ' us')}, dc_tournament (aggregates only) "
            f"{fmt(kernel['dc_tournament'], ' us')}",
            f"  dc_tscen_sim / dc_paths_sim = {fmt(over_paths, '', 3)}; dc_tscen_sim / dc_tournament = "
            f"{fmt(over_tournament, '', 3)}",
            f"  dc_scenario_count {fmt(kernel['dc_scenario_count'], ' us')} per call "
            f"({launches['dc_scenario_count']:.0f} launches) = {fmt(count_share, '', 3)} of stage 1",
            f"  device call {fmt(wall['device_call'], ' ms', 3)} end to end, tournament_scenarios(...) "
            f"{fmt(wall['tournament_scenarios'], ' ms', 3)}; tournament_paths device call "
            f"{fmt(wall['tournament_paths_device_call'], ' ms', 3)}, simulate_tournament device call "
            f"{fmt(wall['simulate_tournament_device_call'], ' ms', 3)}",
            f"  from the records: tournament_scenarios(return_records=True) {fmt(wall['records_s'], ' s', 3)} + numpy "
            f"cross-tabulation {fmt(wall['numpy_s'], ' s', 3)} = {fmt(route, ' s', 3)}: {ratio:.1f} x "
            f"tournament_scenarios; tables equal: {same}"]
    head = (f"World Cup: {N} simulations x 48 teams x 72 group fixtures x 5 rounds, {S} draws; medians over {args.runs} "
            f"runs (smallest .. largest run), each run {args.reps} calls after a warm-up")
    text = "\n".join([head] + lines)
    print(text)
    with open(os.path.join(args.out, "tournament_scenarios_bench.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.join(args.out, "tournament_scenarios_bench.txt"), "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
