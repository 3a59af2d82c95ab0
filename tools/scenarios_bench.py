"""match_scenarios on one MI355X (csrc/dc_scenario.hip.h) at the league case: N = 100 000 simulations of a
380-fixture double round robin of 20 teams over 1000 posterior draws, the default targets, in two cases:

    last_matchday   8 of the last matchday's 10 fixtures (those of the eight strongest home sides) as keys with
                    cap 1: M = 3^8 = 6561 scenarios
    three_by_three  3 of them with cap 3: M = 7^3 = 343 scenarios

    python tools/scenarios_bench.py [--out DIR] [--reps N] [--sims N]

Reports per case: the kernel times of the two stages, `dc_scenario_sim` and `dc_scenario_count` (summed over the
chunks of a call), beside `dc_season`, `dc_leverage_sim` and `dc_points_sim` at the same shape, all from one
`rocprofv3 --kernel-trace --stats` run per case (a child process; profiler off for the wall times) -- stage 1 as a
multiple of `dc_season`, next to `dc_points_sim`'s multiple in the same run; the end-to-end wall time of the device
call (HipContext.season_scenarios: H2D + kernels + D2H) and of the public `match_scenarios` (medians of N after a
warm-up); and the only route without it: `simulate_season(return_tables=True, return_scores=True)` plus the numpy
cross-tabulation of tests/scenarios_ref.py, whose tables must equal the device's.  Writes scenarios_bench.json and
scenarios_bench.txt under --out (default: profiles/scenarios)."""
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

S, T, SEED = 1000, 20, 31337
KERNELS = ("dc_scenario_sim", "dc_scenario_count", "dc_season", "dc_leverage_sim", "dc_points_sim")
TABLES = ("scenario_count", "joint_count")
CASES = ("last_matchday", "three_by_three")


def league():
    """(model with a hand-built posterior, home, away): a double round robin by the circle method, matchday by
    matchday, so that the last 10 fixtures are the last matchday."""
    from bpl import DixonColesMatchPredictor

    rs = np.random.RandomState(9)
    m = DixonColesMatchPredictor()
    m.teams = np.array([f"t{i:02d}" for i in range(T)])
    m._teams_dict = {t: i for i, t in enumerate(m.teams)}
    m.attack, m.defence = rs.normal(0, 0.3, (S, T)), rs.normal(0, 0.3, (S, T))
    m.home_advantage, m.corr_coef = rs.normal(0.25, 0.05, S), rs.uniform(-0.1, 0.1, S)
    ring, first = list(range(1, T)), []
    for r in range(T - 1):
        row = [0] + ring[r:] + ring[:r]
        pairs = [(row[i], row[T - 1 - i]) for i in range(T // 2)]
        first += [(q, p) if r % 2 else (p, q) for p, q in pairs]
    h, a = zip(*(first + [(q, p) for p, q in first]))
    return m, np.array(h, dtype=np.uint16), np.array(a, dtype=np.uint16)


def keys_of(case, m, h):
    """The key fixtures (positions in the list) and their cap."""
    strength = (m.attack + m.defence).mean(axis=0)
    last = np.arange(h.size - T // 2, h.size)
    by_home = last[np.argsort(-strength[h[last]], kind="stable")]
    return ([int(f) for f in by_home[:8]], 1) if case == "last_matchday" else ([int(f) for f in by_home[:3]], 3)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * float(np.min(ts)),
            "max_ms": 1e3 * float(np.max(ts)), "reps": reps}


def calls(n_sims, case):
    """(model, fixtures, keys, cap, the device call, and the season, leverage and points device calls beside it)."""
    from bpl._ffi import prng_key
    from bpl.base import leverage_targets, points_axis

    m, h, a = league()
    keys, cap = keys_of(case, m, h)
    hh, aa, table_idx, table, points, n = m._season_inputs(h, a, n_sims, None, None, (3, 1, 0))
    _, masks = leverage_targets(None, table_idx.size)
    points_min, n_bins = points_axis(table[:, 0], hh, aa, points)      # (slots are the model indices here)
    dev = m._device()
    key = prng_key(SEED)
    head = (hh, aa, table_idx, table, points, n, key)
    return (m, h, a, keys, cap,
            lambda: dev.season_scenarios(*head, masks, keys, [cap] * len(keys)),
            lambda: dev.simulate_season(*head),
            lambda: dev.match_leverage(*head, masks),
            lambda: dev.season_points(*head, masks, points_min, n_bins))


def kernel_times(n_sims, reps, case):
    """Per device call: the summed duration of each kernel's launches (the stages run once per chunk)."""
    d = tempfile.mkdtemp(prefix="scenarios_rocprof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--child", case, "--sims", str(n_sims), "--reps", str(reps)]
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


def measure(case, N, reps, ref_reps):
    import leverage_ref as L
    import scenarios_ref as R
    from bpl.base import LEVERAGE_TARGETS

    m, h, a, keys, cap, device_call, season_call, _, _ = calls(N, case)
    public = lambda: m.match_scenarios(h, a, keys, num_simulations=N, random_state=SEED, margin_cap=cap)   # noqa: E731
    wall = {"device_call": timed(device_call, reps), "match_scenarios": timed(public, reps),
            "simulate_season_aggregates_only": timed(season_call, reps)}
    inside = L.target_masks(LEVERAGE_TARGETS, T)
    route = {"simulate_season_s": [], "numpy_s": []}
    for _ in range(ref_reps + 1):          # (the first pass is the warm-up)
        t0 = time.perf_counter()
        season = m.simulate_season(h, a, num_simulations=N, random_state=SEED, return_tables=True, return_scores=True)
        t1 = time.perf_counter()
        ref = R.counts(season["position"], season["home_goals"], season["away_goals"], inside, keys, [cap] * len(keys))
        t2 = time.perf_counter()
        route["simulate_season_s"].append(t1 - t0)
        route["numpy_s"].append(t2 - t1)
    route = {k: float(np.median(v[1:])) for k, v in route.items()}
    route["total_s"] = route["simulate_season_s"] + route["numpy_s"]
    got = public()
    same = all(np.array_equal(got[k], r) for k, r in zip(TABLES, ref))
    kern = kernel_times(N, reps, case)
    ratio = route["total_s"] * 1e3 / wall["match_scenarios"]["median_ms"]
    season_us = kern["dc_season"]["us_per_call"]
    res = {"key_fixtures": keys, "margin_cap": cap, "scenarios": int(got["scenario_count"].size),
           "scenarios_that_occurred": int((got["scenario_count"] > 0).sum()), "wall": wall, "kernel": kern,
           "sim_over_season_kernel_time": kern["dc_scenario_sim"]["us_per_call"] / season_us,
           "points_sim_over_season_kernel_time": kern["dc_points_sim"]["us_per_call"] / season_us,
           "leverage_sim_over_season_kernel_time": kern["dc_leverage_sim"]["us_per_call"] / season_us,
           "count_over_sim_kernel_time": kern["dc_scenario_count"]["us_per_call"] / kern["dc_scenario_sim"]["us_per_call"],
           "parent_route": route, "parent_route_over_match_scenarios": ratio, "tables_equal_the_numpy_route": bool(same)}
    sim, cnt = kern["dc_scenario_sim"]["us_per_call"], kern["dc_scenario_count"]["us_per_call"]
    lines = [
        f"{case}: {len(keys)} key fixtures {keys} with cap {cap}, {res['scenarios']} scenarios, "
        f"{res['scenarios_that_occurred']} of them occurred",
        f"  dc_scenario_sim {sim:.1f} us per call ({kern['dc_scenario_sim']['launches_per_call']:.0f} launches) = "
        f"{sim / season_us:.2f} x dc_season ({season_us:.1f} us, aggregates only, same run); beside it dc_points_sim "
        f"{kern['dc_points_sim']['us_per_call']:.1f} us = {res['points_sim_over_season_kernel_time']:.2f} x and "
        f"dc_leverage_sim {kern['dc_leverage_sim']['us_per_call']:.1f} us = "
        f"{res['leverage_sim_over_season_kernel_time']:.2f} x; dc_scenario_count {cnt:.1f} us per call "
        f"({kern['dc_scenario_count']['launches_per_call']:.0f} launches) = {cnt / sim:.2f} of stage 1",
        f"  device call {wall['device_call']['median_ms']:.3f} ms end to end, match_scenarios(...) "
        f"{wall['match_scenarios']['median_ms']:.3f} ms, simulate_season device call (aggregates only) "
        f"{wall['simulate_season_aggregates_only']['median_ms']:.3f} ms (medians of {reps})",
        f"  without it: simulate_season(return_tables, return_scores) {route['simulate_season_s']:.3f} s + numpy "
        f"cross-tabulation {route['numpy_s']:.3f} s = {route['total_s']:.3f} s: {ratio:.0f} x match_scenarios; "
        f"tables equal: {same}"]
    return res, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scenarios"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--ref-reps", type=int, default=1)
    ap.add_argument("--sims", type=int, default=100_000)
    ap.add_argument("--child", choices=CASES, help=argparse.SUPPRESS)
    args = ap.parse_args()
    N = args.sims
    if args.child:
        runs = calls(N, args.child)[5:]
        for _ in range(args.reps + 1):
            for call in runs:
                call()
        return
    os.makedirs(args.out, exist_ok=True)
    res = {"simulations": N, "draws": S, "fixtures": T * (T - 1), "teams": T, "cases": {}}
    text = [f"league: {N} simulations x {T * (T - 1)} fixtures x {T} teams x 3 targets, {S} draws"]
    for case in CASES:
        res["cases"][case], lines = measure(case, N, args.reps, args.ref_reps)
        text += lines
    text = "\n".join(text)
    print(text)
    with open(os.path.join(args.out, "scenarios_bench.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.join(args.out, "scenarios_bench.txt"), "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
