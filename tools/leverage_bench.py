"""match_leverage on one MI355X (csrc/dc_leverage.hip.h) at the league case: N = 100 000 simulations of a
380-fixture double round robin of 20 teams over 1000 posterior draws, the default targets.

    python tools/leverage_bench.py [--out DIR] [--reps N] [--sims N]

Reports: the kernel times of the two stages, `dc_leverage_sim` and `dc_leverage_count` (summed over the chunks
of a call), and of `dc_season` at the same shape, from a `rocprofv3 --kernel-trace --stats` run of its own (a
child process; profiler off for the wall times); the end-to-end wall time of the device call
(HipContext.match_leverage: H2D + kernels + D2H) and of the public `match_leverage` (medians of N after a
warm-up); and the only route without it: `simulate_season(return_tables=True, return_scores=True)` plus the
numpy cross-tabulation of tests/leverage_ref.py (timed --ref-reps times: it takes seconds), whose tables must
equal the device's.  Writes leverage_bench.json and leverage_bench.txt under --out (default: profiles/leverage)."""
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
KERNELS = ("dc_leverage_sim", "dc_leverage_count", "dc_season")


def league():
    """(model with a hand-built posterior, home, away): the shape of tests/test_gpu_season.py's large run."""
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
    """(model, fixtures, the device call, the season kernel's call without per-simulation outputs)."""
    from bpl._ffi import prng_key
    from bpl.base import leverage_targets

    m, h, a = league()
    hh, aa, table_idx, table, points, n = m._season_inputs(h, a, n_sims, None, None, (3, 1, 0))
    _, masks = leverage_targets(None, table_idx.size)
    dev = m._device()
    key = prng_key(SEED)
    return (m, h, a, lambda: dev.match_leverage(hh, aa, table_idx, table, points, n, key, masks),
            lambda: dev.simulate_season(hh, aa, table_idx, table, points, n, key))


def kernel_times(n_sims, reps):
    """Per device call: the summed duration of each kernel's launches (the stages run once per chunk)."""
    d = tempfile.mkdtemp(prefix="leverage_rocprof_")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "leverage"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--ref-reps", type=int, default=1)
    ap.add_argument("--sims", type=int, default=100_000)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    N = args.sims
    m, h, a, device_call, season_call = calls(N)
    if args.child:
        for _ in range(args.reps + 1):
            device_call()
            season_call()
        return
    import leverage_ref as L
    from bpl.base import LEVERAGE_TARGETS

    os.makedirs(args.out, exist_ok=True)
    wall = {"device_call": timed(device_call, args.reps),
            "match_leverage": timed(lambda: m.match_leverage(h, a, num_simulations=N, random_state=SEED), args.reps),
            "simulate_season_aggregates_only": timed(season_call, args.reps)}
    inside = L.target_masks(LEVERAGE_TARGETS, T)
    route = {"simulate_season_s": [], "numpy_s": []}
    for _ in range(args.ref_reps + 1):          # (the first pass is the warm-up)
        t0 = time.perf_counter()
        season = m.simulate_season(h, a, num_simulations=N, random_state=SEED, return_tables=True, return_scores=True)
        t1 = time.perf_counter()
        ref = L.counts(season["position"], season["home_goals"], season["away_goals"], inside)
        t2 = time.perf_counter()
        route["simulate_season_s"].append(t1 - t0)
        route["numpy_s"].append(t2 - t1)
    route = {k: float(np.median(v[1:])) for k, v in route.items()}
    route["total_s"] = route["simulate_season_s"] + route["numpy_s"]
    got = m.match_leverage(h, a, num_simulations=N, random_state=SEED)
    same = all(np.array_equal(got[k], r) for k, r in zip(("outcome_count", "target_count", "joint_count"), ref))
    kern = kernel_times(N, args.reps)
    ratio = route["total_s"] * 1e3 / wall["match_leverage"]["median_ms"]
    stage = kern["dc_leverage_count"]["us_per_call"] / kern["dc_leverage_sim"]["us_per_call"]
    f, t, k = np.unravel_index(np.argmax(got["leverage"]), got["leverage"].shape)
    res = {"simulations": N, "draws": S, "fixtures": int(h.size), "teams": T, "targets": list(LEVERAGE_TARGETS),
           "wall": wall, "kernel": kern, "count_over_sim_kernel_time": stage, "parent_route": route,
           "parent_route_over_match_leverage": ratio, "tables_equal_the_numpy_route": bool(same)}
    lines = [
        f"league: {N} simulations x {h.size} fixtures x {T} teams x {len(LEVERAGE_TARGETS)} targets, {S} draws",
        f"  dc_leverage_sim {kern['dc_leverage_sim']['us_per_call']:.1f} us per call "
        f"({kern['dc_leverage_sim']['launches_per_call']:.0f} launches), dc_leverage_count "
        f"{kern['dc_leverage_count']['us_per_call']:.1f} us per call "
        f"({kern['dc_leverage_count']['launches_per_call']:.0f} launches): counting / simulation = {stage:.2f}",
        f"  dc_season at the same shape (aggregates only) {kern['dc_season']['us_per_call']:.1f} us per call",
        f"  device call {wall['device_call']['median_ms']:.3f} ms end to end, match_leverage(...) "
        f"{wall['match_leverage']['median_ms']:.3f} ms, simulate_season device call (aggregates only) "
        f"{wall['simulate_season_aggregates_only']['median_ms']:.3f} ms (medians of {args.reps})",
        f"  without it: simulate_season(return_tables, return_scores) {route['simulate_season_s']:.3f} s + numpy "
        f"cross-tabulation {route['numpy_s']:.3f} s = {route['total_s']:.3f} s: {ratio:.0f} x match_leverage; "
        f"tables equal: {same}",
        f"  largest leverage: fixture {f} ({m.teams[h[f]]} v {m.teams[a[f]]}) on {m.teams[t]}'s "
        f"{list(LEVERAGE_TARGETS)[k]} odds, {got['leverage'][f, t, k]:.4f}"]
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(args.out, "leverage_bench.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.join(args.out, "leverage_bench.txt"), "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
