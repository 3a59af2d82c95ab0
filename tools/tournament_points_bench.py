"""tournament_points on one MI355X (csrc/dc_group_points.hip.h) at the World Cup case: N = 100 000 simulations of 48
teams (12 groups of 4, 72 group fixtures, the 8 best thirds, a 32-team bracket) over 1000 posterior draws, default
knockout rule (or --knockout-rule extra_time: single legs, dc_knockout.hip.h's ladder), in both tie-break modes
("overall" and "head_to_head").

    python tools/tournament_points_bench.py [--out DIR] [--reps N] [--runs N] [--sims N] [--knockout-rule RULE]

Reports, per mode: the kernel time of the recording stage `dc_gpts_sim` and of the counting kernel `dc_gpts_count`
(summed over the chunks of a call) beside `dc_tscen_sim`, `dc_paths_sim` and `dc_tournament` at the same shape, from
`rocprofv3 --kernel-trace --stats` runs of their own (child processes, all five kernels timed in the same run; profiler
off for the wall times); the end-to-end wall time of the device call (HipContext.tournament_points: H2D + kernels + D2H)
and of the public `tournament_points` (medians of --reps after a warm-up); and the only other route to the points
tables: `tournament_paths(return_records=True)` plus the numpy cross-tabulation of tests/tournament_points_ref.py, which
gives five of the eight tables (no goal difference, no ranking of the rest) and must equal the device's.  Everything is
measured --runs times (default 3): the figures are the medians over the runs, with the smallest and largest run beside
them.  Writes tournament_points_bench.json and tournament_points_bench.txt under --out (default:
profiles/tournament_points)."""
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

KERNELS = ("dc_gpts_sim", "dc_gpts_count", "dc_tscen_sim", "dc_paths_sim", "dc_tournament")
MODES = ("overall", "head_to_head")
TABLES = ("team_points_count", "team_target_count", "team_place_count", "place_points_count", "place_gap_count")
GD_CAP = 3


def calls(n_sims, tiebreak, rule="redraw"):
    """(model, kwargs, checked inputs, the device call, and tournament_scenarios', tournament_paths' and
    simulate_tournament's device calls at the same shape)."""
    from bpl.base import points_axis

    m, kw = world_cup()
    inp, call = m._tournament_call(kw["knockout"], kw["groups"], kw["advance"], kw["best_of_rest"], None, None, None,
                                   (3, 1, 0), n_sims, SEED, None, tiebreak, None, rule, None, 1 / 3, None, False)
    pmin, bins = points_axis(inp["table"][:, 0], inp["fix_p"], inp["fix_q"], inp["points"])
    dev = m._device()
    return (m, kw, inp,
            lambda: dev.tournament_points(*call["args"], points_min=pmin, n_bins=bins, gd_cap=GD_CAP, **call["kwargs"]),
            lambda: dev.tournament_scenarios(*call["args"], key_fixture=[2, 3], key_cap=[3, 3], **call["kwargs"]),
            lambda: dev.tournament_paths(*call["args"], **call["kwargs"]),
            lambda: dev.simulate_tournament(*call["args"], **call["kwargs"]))


def kernel_times(n_sims, reps, tiebreak, rule="redraw"):
    """Per device call: the summed duration of each kernel's launches (the stages run once per chunk)."""
    d = tempfile.mkdtemp(prefix="gpts_rocprof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--child", tiebreak, "--sims", str(n_sims), "--reps", str(reps),
           "--knockout-rule", rule]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tournament_points"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sims", type=int, default=100_000)
    ap.add_argument("--knockout-rule", default="redraw", choices=("redraw", "extra_time"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    N, rule = args.sims, args.knockout_rule
    if args.child:
        _, _, _, *device_calls = calls(N, args.child, rule)
        for _ in range(args.reps + 1):
            for fn in device_calls:
                fn()
        return
    import tournament_points_ref as G
    from bpl import group_points

    os.makedirs(args.out, exist_ok=True)
    res = {"simulations": N, "draws": S, "teams": 48, "gd_cap": GD_CAP, "knockout_rule": rule, "runs": args.runs,
           "reps": args.reps, "modes": {}}
    lines = []
    for tiebreak in MODES:
        m, kw, inp, device_call, scen_call, paths_call, tournament_call = calls(N, tiebreak, rule)
        run = dict(num_simulations=N, random_state=SEED, tiebreak=tiebreak, knockout_rule=rule, **kw)
        wall = {k: [] for k in ("device_call", "tournament_points", "tournament_scenarios_device_call",
                                "tournament_paths_device_call", "simulate_tournament_device_call", "records_s", "numpy_s")}
        kern = []
        same = True
        for _ in range(args.runs):
            wall["device_call"].append(timed(device_call, args.reps)["median_ms"])
            wall["tournament_points"].append(timed(lambda: m.tournament_points(gd_cap=GD_CAP, **run), args.reps)["median_ms"])
            wall["tournament_scenarios_device_call"].append(timed(scen_call, args.reps)["median_ms"])
            wall["tournament_paths_device_call"].append(timed(paths_call, args.reps)["median_ms"])
            wall["simulate_tournament_device_call"].append(timed(tournament_call, args.reps)["median_ms"])
            m.tournament_paths(return_records=True, **run)              # (the warm-up of the route below)
            t0 = time.perf_counter()
            rec = m.tournament_paths(return_records=True, **run)
            t1 = time.perf_counter()
            got = m.tournament_points(gd_cap=GD_CAP, **run)
            t2 = time.perf_counter()
            ref = G.counts(G.records_from_paths(rec, inp), inp, int(got["points"][0]), got["points"].size)
            t3 = time.perf_counter()
            wall["records_s"].append(t1 - t0)
            wall["numpy_s"].append(t3 - t2)
            same = same and all(np.array_equal(got[k], ref[k]) for k in TABLES)
            kern.append(kernel_times(N, args.reps, tiebreak, rule))
        wall = {k: spread(v) for k, v in wall.items()}
        kernel = {k: spread([r[k]["us_per_call"] for r in kern]) for k in KERNELS}
        launches = {k: kern[0][k]["launches_per_call"] for k in KERNELS}
        over = {k: spread([r["dc_gpts_sim"]["us_per_call"] / r[k]["us_per_call"] for r in kern])
                for k in ("dc_tscen_sim", "dc_paths_sim", "dc_tournament")}
        count_share = spread([r["dc_gpts_count"]["us_per_call"] / r["dc_gpts_sim"]["us_per_call"] for r in kern])
        route = spread([a + b for a, b in zip(wall["records_s"]["runs"], wall["numpy_s"]["runs"])])
        ratio = route["median"] * 1e3 / wall["tournament_points"]["median"]
        cut = list(group_points.cut_line(got))
        res["modes"][tiebreak] = {
            "points_bins": int(got["points"].size), "kernel_us_per_call": kernel, "launches_per_call": launches,
            "gpts_sim_over": over, "count_over_gpts_sim": count_share,
            "wall_ms": {k: v for k, v in wall.items() if not k.endswith("_s")},
            "records_route_s": {"records": wall["records_s"], "numpy": wall["numpy_s"], "total": route},
            "records_route_over_tournament_points": ratio, "tables_equal_the_numpy_route": bool(same), "cut_line": cut}
        lines += [
            f"{tiebreak}: {got['points'].size} points bins, {2 * GD_CAP + 1} goal-difference bins; most likely last "
            f"qualifying third: {cut[0]} points, goal difference {cut[1]:+d} ({cut[2]:.3f})",
            f"  dc_gpts_sim {fmt(kernel['dc_gpts_sim'], ' us')} per call ({launches['dc_gpts_sim']:.0f} launches); same "
            f"run: dc_tscen_sim {fmt(kernel['dc_tscen_sim'], ' us')}, dc_paths_sim {fmt(kernel['dc_paths_sim'], ' us')}, "
            f"dc_tournament (aggregates only) {fmt(kernel['dc_tournament'], ' us')}",
            f"  dc_gpts_sim / dc_tscen_sim = {fmt(over['dc_tscen_sim'], '', 3)}; / dc_paths_sim = "
            f"{fmt(over['dc_paths_sim'], '', 3)}; / dc_tournament = {fmt(over['dc_tournament'], '', 3)}",
            f"  dc_gpts_count {fmt(kernel['dc_gpts_count'], ' us')} per call ({launches['dc_gpts_count']:.0f} launches) "
            f"= {fmt(count_share, '', 3)} of stage 1",
            f"  device call {fmt(wall['device_call'], ' ms', 3)} end to end, tournament_points(...) "
            f"{fmt(wall['tournament_points'], ' ms', 3)}; device calls of tournament_scenarios "
            f"{fmt(wall['tournament_scenarios_device_call'], ' ms', 3)}, tournament_paths "
            f"{fmt(wall['tournament_paths_device_call'], ' ms', 3)}, simulate_tournament "
            f"{fmt(wall['simulate_tournament_device_call'], ' ms', 3)}",
            f"  from the records: tournament_paths(return_records=True) {fmt(wall['records_s'], ' s', 3)} + numpy "
            f"cross-tabulation {fmt(wall['numpy_s'], ' s', 3)} = {fmt(route, ' s', 3)} for five of the eight tables: "
            f"{ratio:.1f} x tournament_points; tables equal: {same}"]
    head = (f"World Cup: {N} simulations x 48 teams x 72 group fixtures x 5 rounds ({rule}), {S} draws; medians over "
            f"{args.runs} runs (smallest .. largest run), each run {args.reps} calls after a warm-up")
    text = "\n".join([head] + lines)
    print(text)
    with open(os.path.join(args.out, "tournament_points_bench.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.join(args.out, "tournament_points_bench.txt"), "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
