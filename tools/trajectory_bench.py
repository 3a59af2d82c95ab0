"""season_trajectory on one MI355X (csrc/dc_trajectory.hip.h) at the league case: N = 100 000 simulations of a
380-fixture double round robin of 20 teams in 38 matchdays of 10, over 1000 posterior draws, the default targets.

    python tools/trajectory_bench.py [--out DIR] [--reps N] [--sims N] [--ref-sims N]

Reports: the kernel times of the three stages, `dc_trajectory_sim`, `dc_trajectory_count` and `dc_trajectory_paths`
(summed over the chunks of a call), and of `dc_season` and `dc_points_sim` at the same shape, from a
`rocprofv3 --kernel-trace --stats` run of its own (a child process; profiler off for the wall times) -- stage 1 as a
multiple of `dc_season`; the end-to-end wall time of the device call (HipContext.season_trajectory: H2D + kernels +
D2H) and of the public `season_trajectory` (medians of N after a warm-up); and the only route without it:
`simulate_season(return_tables=True, return_scores=True)` plus the numpy re-ranking of tests/trajectory_ref.py, run at
--ref-sims simulations (small enough to finish) and SCALED linearly to N, labelled as such; its tables must equal the
device's at --ref-sims.  Writes trajectory_bench.json and trajectory_bench.txt under --out (default:
profiles/trajectory)."""
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

S, T, ROUNDS, SEED = 1000, 20, 38, 31337
KERNELS = ("dc_trajectory_sim", "dc_trajectory_count", "dc_trajectory_paths", "dc_points_sim", "dc_season")
TABLES = ("position_count", "target_count", "target_final_count", "points_sum", "points_sq_sum",
          "rounds_inside_count", "secured_count", "lead_changes_count")


def league():
    """(model with a hand-built posterior, home, away, matchday): the shape of tools/points_bench.py, the fixtures
    dealt into 38 matchdays of 10 in shuffled order."""
    from bpl import DixonColesMatchPredictor

    rs = np.random.RandomState(9)
    m = DixonColesMatchPredictor()
    m.teams = np.array([f"t{i:02d}" for i in range(T)])
    m._teams_dict = {t: i for i, t in enumerate(m.teams)}
    m.attack, m.defence = rs.normal(0, 0.3, (S, T)), rs.normal(0, 0.3, (S, T))
    m.home_advantage, m.corr_coef = rs.normal(0.25, 0.05, S), rs.uniform(-0.1, 0.1, S)
    h, a = np.nonzero(~np.eye(T, dtype=bool))
    md = rs.permutation(h.size) // (h.size // ROUNDS)
    return m, h.astype(np.uint16), a.astype(np.uint16), md


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
    """(model, fixtures, labels, the device call, the points and season kernels' calls at the same shape)."""
    from bpl._ffi import prng_key
    from bpl.base import leverage_targets, points_axis, trajectory_axis, trajectory_rounds

    m, h, a, md = league()
    hh, aa, table_idx, table, points, n = m._season_inputs(h, a, n_sims, None, None, (3, 1, 0))
    _, masks = leverage_targets(None, table_idx.size)
    low, bins = trajectory_axis(table[:, 0], hh, aa, points)          # (slots are the model indices here)
    points_min, n_bins = points_axis(table[:, 0], hh, aa, points)
    _, fix_id, round_end = trajectory_rounds(md, h.size)
    dev = m._device()
    key = prng_key(SEED)
    return (m, h, a, md,
            lambda: dev.season_trajectory(hh, aa, table_idx, table, points, n, key, masks, low, bins, fix_id, round_end),
            lambda: dev.season_points(hh, aa, table_idx, table, points, n, key, masks, points_min, n_bins),
            lambda: dev.simulate_season(hh, aa, table_idx, table, points, n, key))


def kernel_times(n_sims, reps):
    """Per device call: the summed duration of each kernel's launches (the stages run once per chunk)."""
    d = tempfile.mkdtemp(prefix="trajectory_rocprof_")
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


def host_route(m, h, a, md, n_ref):
    """(seconds of simulate_season with scorelines, seconds of the numpy re-ranking and counting, tables equal)."""
    import leverage_ref as L
    import trajectory_ref as R
    from bpl._ffi import prng_key
    from bpl.base import LEVERAGE_TARGETS

    inside = L.target_masks(LEVERAGE_TARGETS, T)
    m.simulate_season(h, a, num_simulations=n_ref, random_state=SEED, return_tables=True, return_scores=True)   # warm-up
    t0 = time.perf_counter()
    season = m.simulate_season(h, a, num_simulations=n_ref, random_state=SEED, return_tables=True, return_scores=True)
    t1 = time.perf_counter()
    _, pos, pts = R.paths(h, a, md, season["home_goals"], season["away_goals"], np.zeros((T, 3), dtype=np.int64),
                          (3, 1, 0), prng_key(SEED))                 # (slots are the model indices here)
    ref = R.counts(pos, pts, inside)
    t2 = time.perf_counter()
    got = m.season_trajectory(h, a, md, num_simulations=n_ref, random_state=SEED)
    return t1 - t0, t2 - t1, all(np.array_equal(got[k], ref[k]) for k in TABLES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trajectory"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sims", type=int, default=100_000)
    ap.add_argument("--ref-sims", type=int, default=5_000)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    N = args.sims
    m, h, a, md, device_call, points_call, season_call = calls(N)
    if args.child:
        for _ in range(args.reps + 1):
            device_call()
            points_call()
            season_call()
        return
    os.makedirs(args.out, exist_ok=True)
    wall = {"device_call": timed(device_call, args.reps),
            "season_trajectory": timed(lambda: m.season_trajectory(h, a, md, num_simulations=N, random_state=SEED),
                                       args.reps),
            "points_device_call": timed(points_call, args.reps),
            "simulate_season_aggregates_only": timed(season_call, args.reps)}
    sim_s, numpy_s, same = host_route(m, h, a, md, args.ref_sims)
    scale = N / args.ref_sims
    route = {"ref_sims": args.ref_sims, "simulate_season_s": sim_s, "numpy_s": numpy_s,
             "scaled_to_sims": N, "scaled_total_s": (sim_s + numpy_s) * scale}
    got = m.season_trajectory(h, a, md, num_simulations=N, random_state=SEED)
    kern = kernel_times(N, args.reps)
    ratio = route["scaled_total_s"] * 1e3 / wall["season_trajectory"]["median_ms"]
    sim, cnt, pth, pts, season = (kern[k]["us_per_call"] for k in KERNELS)
    res = {"simulations": N, "draws": S, "fixtures": int(h.size), "teams": T, "matchdays": ROUNDS,
           "record_bytes_per_simulation": 3 * T * ROUNDS + ROUNDS, "wall": wall, "kernel": kern,
           "sim_over_season_kernel_time": sim / season, "sim_over_points_sim_kernel_time": sim / pts,
           "counting_over_sim_kernel_time": (cnt + pth) / sim, "host_route": route,
           "scaled_host_route_over_season_trajectory": ratio, "tables_equal_the_numpy_route": bool(same)}
    top = int(np.argmax(got["position_proba"][-1][:, 0]))
    half = ROUNDS // 2 - 1
    lines = [
        f"league: {N} simulations x {h.size} fixtures in {ROUNDS} matchdays x {T} teams x 3 targets, {S} draws; "
        f"{res['record_bytes_per_simulation']} B of record per simulation",
        f"  dc_trajectory_sim {sim:.1f} us per call ({kern['dc_trajectory_sim']['launches_per_call']:.0f} launches) = "
        f"{sim / season:.2f} x dc_season ({season:.1f} us, aggregates only, same run) = {sim / pts:.2f} x dc_points_sim "
        f"({pts:.1f} us); dc_trajectory_count {cnt:.1f} us, dc_trajectory_paths {pth:.1f} us per call: together "
        f"{(cnt + pth) / sim:.2f} of stage 1",
        f"  device call {wall['device_call']['median_ms']:.3f} ms end to end, season_trajectory(...) "
        f"{wall['season_trajectory']['median_ms']:.3f} ms; season_points device call "
        f"{wall['points_device_call']['median_ms']:.3f} ms, simulate_season device call (aggregates only) "
        f"{wall['simulate_season_aggregates_only']['median_ms']:.3f} ms (medians of {args.reps})",
        f"  without it, at {args.ref_sims} simulations: simulate_season(return_scores) {sim_s:.3f} s + numpy re-ranking "
        f"and counting {numpy_s:.3f} s; SCALED x{scale:g} to {N}: {route['scaled_total_s']:.1f} s = {ratio:.0f} x "
        f"season_trajectory; tables equal at {args.ref_sims}: {same}",
        f"  {got['teams'][top]} is top after matchday {half + 1} of {ROUNDS} in {got['target_proba'][half, top, 0]:.3f} of "
        f"the simulations and then champion in {got['final_given_inside'][half, top, 0]:.3f} of those "
        f"({got['final_given_outside'][half, top, 0]:.3f} otherwise); the lead changes hands "
        f"{got['expected_lead_changes']:.2f} times a season; the eventual bottom three spend "
        f"{got['expected_rounds_inside'][:, 2].max():.1f} matchdays there at most on average"]
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(args.out, "trajectory_bench.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.join(args.out, "trajectory_bench.txt"), "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
