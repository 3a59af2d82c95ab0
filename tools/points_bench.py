"""points_needed on one MI355X (csrc/dc_points.hip.h) at the league case: N = 100 000 simulations of a
380-fixture double round robin of 20 teams over 1000 posterior draws, the default targets.

    python tools/points_bench.py [--out DIR] [--reps N] [--sims N]

Reports: the kernel times of the two stages, `dc_points_sim` and `dc_points_count` (summed over the chunks of a
call), and of `dc_season` at the same shape, from a `rocprofv3 --kernel-trace --stats` run of its own (a child
process; profiler off for the wall times) -- stage 1 as a multiple of `dc_season`, stage 2 as a share of stage 1;
the end-to-end wall time of the device call (HipContext.season_points: H2D + kernels + D2H) and of the public
`points_needed` (medians of N after a warm-up); and the only route without it:
`simulate_season(return_tables=True)` plus the numpy cross-tabulation of tests/points_ref.py, whose tables must
equal the device's.  Writes points_bench.json and points_bench.txt under --out (default: profiles/points)."""
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
KERNELS = ("dc_points_sim", "dc_points_count", "dc_season")
TABLES = ("team_points_count", "team_target_count", "position_points_count", "gap_count")


def league():
    """(model with a hand-built posterior, home, away): the shape of tools/leverage_bench.py."""
    from bpl import DixonColesMatchPredictor

    rs = np.random.RandomState(9)
    m = DixonColesMatchPredictor()
    m.teams = np.array([f"t{i:02d}" for i in range(T)])
    m._teams_dict = {t: i for i, t in enumerate(m.teams)}
    m.attack, m.defence = rs.normal(0, 0.3, (S, T)), rs.normal(0, 0.3, (S, T))
    m.home_advantage, m.corr_coef = rs.normal(0.25, 0.05, S), rs.uniform(-0.1, 0.1, S)
    h, a = np.nonzero(~np.eye(T, dtype=bool))
    return m, h.astype(np.uint16), a.astype(np.uint16)


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
    """(model, fixtures, the axis, the device call, the season kernel's call without per-simulation outputs)."""
    from bpl._ffi import prng_key
    from bpl.base import leverage_targets, points_axis

    m, h, a = league()
    hh, aa, table_idx, table, points, n = m._season_inputs(h, a, n_sims, None, None, (3, 1, 0))
    _, masks = leverage_targets(None, table_idx.size)
    points_min, n_bins = points_axis(table[:, 0], hh, aa, points)      # (slots are the model indices here)
    dev = m._device()
    key = prng_key(SEED)
    return (m, h, a, (points_min, n_bins),
            lambda: dev.season_points(hh, aa, table_idx, table, points, n, key, masks, points_min, n_bins),
            lambda: dev.simulate_season(hh, aa, table_idx, table, points, n, key))


def kernel_times(n_sims, reps):
    """Per device call: the summed duration of each kernel's launches (the stages run once per chunk)."""
    d = tempfile.mkdtemp(prefix="points_rocprof_")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--ref-reps", type=int, default=1)
    ap.add_argument("--sims", type=int, default=100_000)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    N = args.sims
    m, h, a, (points_min, n_bins), device_call, season_call = calls(N)
    if args.child:
        for _ in range(args.reps + 1):
            device_call()
            season_call()
        return
    import leverage_ref as L
    import points_ref as R
    from bpl.base import LEVERAGE_TARGETS

    os.makedirs(args.out, exist_ok=True)
    wall = {"device_call": timed(device_call, args.reps),
            "points_needed": timed(lambda: m.points_needed(h, a, num_simulations=N, random_state=SEED), args.reps),
            "simulate_season_aggregates_only": timed(season_call, args.reps)}
    inside = L.target_masks(LEVERAGE_TARGETS, T)
    route = {"simulate_season_s": [], "numpy_s": []}
    for _ in range(args.ref_reps + 1):          # (the first pass is the warm-up)
        t0 = time.perf_counter()
        season = m.simulate_season(h, a, num_simulations=N, random_state=SEED, return_tables=True)
        t1 = time.perf_counter()
        ref = R.counts(season["points"], season["position"], inside, points_min, n_bins)
        t2 = time.perf_counter()
        route["simulate_season_s"].append(t1 - t0)
        route["numpy_s"].append(t2 - t1)
    route = {k: float(np.median(v[1:])) for k, v in route.items()}
    route["total_s"] = route["simulate_season_s"] + route["numpy_s"]
    got = m.points_needed(h, a, num_simulations=N, random_state=SEED)
    same = all(np.array_equal(got[k], r) for k, r in zip(TABLES, ref))
    kern = kernel_times(N, args.reps)
    ratio = route["total_s"] * 1e3 / wall["points_needed"]["median_ms"]
    res = {"simulations": N, "draws": S, "fixtures": int(h.size), "teams": T, "targets": list(LEVERAGE_TARGETS),
           "points_min": points_min, "bins": n_bins, "occupied_bins": int((got["team_points_count"].sum(0) > 0).sum()),
           "wall": wall, "kernel": kern,
           "sim_over_season_kernel_time": kern["dc_points_sim"]["us_per_call"] / kern["dc_season"]["us_per_call"],
           "count_over_sim_kernel_time": kern["dc_points_count"]["us_per_call"] / kern["dc_points_sim"]["us_per_call"],
           "parent_route": route, "parent_route_over_points_needed": ratio, "tables_equal_the_numpy_route": bool(same)}
    lines = [
        f"league: {N} simulations x {h.size} fixtures x {T} teams x {len(LEVERAGE_TARGETS)} targets, {S} draws; "
        f"{n_bins} bins from {points_min} points, {res['occupied_bins']} of them occupied"]
    sim, cnt, season = (kern[k]["us_per_call"] for k in KERNELS)
    lines += [
        f"  dc_points_sim {sim:.1f} us per call ({kern['dc_points_sim']['launches_per_call']:.0f} launches) = "
        f"{sim / season:.2f} x dc_season ({season:.1f} us, aggregates only, same run); dc_points_count {cnt:.1f} us "
        f"per call ({kern['dc_points_count']['launches_per_call']:.0f} launches) = {cnt / sim:.2f} of stage 1"]
    lines += [
        f"  device call {wall['device_call']['median_ms']:.3f} ms end to end, points_needed(...) "
        f"{wall['points_needed']['median_ms']:.3f} ms, simulate_season device call (aggregates only) "
        f"{wall['simulate_season_aggregates_only']['median_ms']:.3f} ms (medians of {args.reps})",
        f"  without it: simulate_season(return_tables) {route['simulate_season_s']:.3f} s + numpy cross-tabulation "
        f"{route['numpy_s']:.3f} s = {route['total_s']:.3f} s: {ratio:.0f} x points_needed; tables equal: {same}",
        f"  the champion ends on {got['position_points_mean'][0]:.1f} points on average "
        f"({', '.join(f'{q} at {lv:g}' for lv, q in zip(got['levels'], got['position_points_quantile'][:, 0]))}); "
        f"position 17 (the last safe one) on {got['position_points_mean'][16]:.1f}; title level on points in "
        f"{got['level_proba'][0]:.4f} of the simulations, the drop in {got['level_proba'][16]:.4f}"]
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(args.out, "points_bench.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.join(args.out, "points_bench.txt"), "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
