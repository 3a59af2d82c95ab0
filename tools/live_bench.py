"""simulate_season with matches in progress on one MI355X (csrc/dc_live.hip.h) next to the kick-off simulator at the
same size:

    live    N simulations of 370 fixtures still to kick off + 10 matches in play (a 20-team double round robin with
            one round in progress) over 1000 posterior draws, the draws re-weighted by the ten states and resampled:
            live_loglik, live_weights and dc_season_live<false>;
    plain   N simulations of the same 380 fixtures from kick-off: dc_season<false>.

    python tools/live_bench.py [--out DIR] [--reps N] [--sims N]

Reports the kernel times, each mode from a `rocprofv3 --kernel-trace --stats` run of its own (a child process;
profiler off for the wall times), the wall time of the device call and of the public method end to end (medians of N
after a warm-up), the ratio dc_season_live / dc_season, and the numpy restatement's time at 1000 simulations.  Writes
live_bench.json and live_bench.txt under --out (default: profiles/live)."""
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
KERNELS = {"live": ("live_loglik", "live_weights", "dc_season_live<false>"), "plain": ("dc_season<false>",)}
# the round in progress: (home goals, away goals, elapsed) of team 2m v team 2m + 1
STATES = ((0, 0, 0.0), (1, 0, 0.2), (0, 1, 0.35), (1, 1, 0.5), (2, 0, 0.5), (0, 0, 0.6), (2, 1, 0.7), (0, 2, 0.8),
          (3, 1, 0.9), (1, 1, 0.97))


def league():
    from bpl import DixonColesMatchPredictor

    rs = np.random.RandomState(9)
    m = DixonColesMatchPredictor()
    m.teams = np.array([f"t{i:02d}" for i in range(T)])
    m._teams_dict = {t: i for i, t in enumerate(m.teams)}
    m.attack, m.defence = rs.normal(0, 0.3, (S, T)), rs.normal(0, 0.3, (S, T))
    m.home_advantage, m.corr_coef = rs.normal(0.25, 0.05, S), rs.uniform(-0.1, 0.1, S)
    h, a = np.nonzero(~np.eye(T, dtype=bool))
    live = (h % 2 == 0) & (a == h + 1)
    ip = {"home_team": h[live].astype(np.uint16), "away_team": a[live].astype(np.uint16),
          "home_goals": [s[0] for s in STATES], "away_goals": [s[1] for s in STATES], "elapsed": [s[2] for s in STATES]}
    return m, h.astype(np.uint16), a.astype(np.uint16), live, ip


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
    """{mode: (the device call, the public method)}, aggregates only."""
    from bpl._ffi import prng_key

    key = prng_key(SEED)
    m, h, a, live, ip = league()
    hh, aa, table_idx, table, points, n = m._season_inputs(h, a, n_sims, None, None, (3, 1, 0))
    ipr = m._in_play_inputs(ip)
    dev = m._device()
    return {
        "live": (lambda: dev.simulate_season_live(hh[~live], aa[~live], table_idx, table, points, n, key, in_play=ipr),
                 lambda: m.simulate_season(h[~live], a[~live], num_simulations=n_sims, random_state=SEED, in_play=ip)),
        "plain": (lambda: dev.simulate_season(hh, aa, table_idx, table, points, n, key),
                  lambda: m.simulate_season(h, a, num_simulations=n_sims, random_state=SEED)),
    }


def restatement_seconds(n_sims=1000):
    import live_ref as LR
    from bpl._ffi import prng_key

    m, h, a, live, ip = league()
    hh, aa, table_idx, table, points, n = m._season_inputs(h, a, n_sims, None, None, (3, 1, 0))
    t0 = time.perf_counter()
    LR.simulate_season_live(m.attack, m.defence, m.home_advantage, m.corr_coef, hh[~live], aa[~live],
                            m._in_play_inputs(ip), table_idx, table, points, n, prng_key(SEED))
    return time.perf_counter() - t0


def kernel_times(mode, n_sims, reps):
    """Per device call of `mode`: the summed duration of each of its kernels' launches."""
    d = tempfile.mkdtemp(prefix="live_rocprof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--child", mode, "--sims", str(n_sims), "--reps", str(reps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise RuntimeError(f"the rocprofv3 run exited {r.returncode}: {r.stderr[-2000:]}")
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    k = next((k for k in KERNELS[mode] if k in row["Name"]), None)
                    if k:
                        out[k] = {"launches": int(row["Calls"]),
                                  "us_per_call": float(row["TotalDurationNs"]) / 1e3 / (reps + 1)}
        if set(out) != set(KERNELS[mode]):
            raise RuntimeError(f"the rocprofv3 stats hold {sorted(out)}, not {sorted(KERNELS[mode])}")
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "live"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sims", type=int, default=100_000)
    ap.add_argument("--child", choices=tuple(KERNELS), help=argparse.SUPPRESS)
    args = ap.parse_args()
    N = args.sims
    todo = calls(N)
    if args.child:
        for _ in range(args.reps + 1):
            todo[args.child][0]()
        return
    os.makedirs(args.out, exist_ok=True)
    wall = {mode: {"device_call": timed(pair[0], args.reps), "end_to_end": timed(pair[1], args.reps)}
            for mode, pair in todo.items()}
    kern = {}
    for mode in KERNELS:
        kern.update(kernel_times(mode, N, args.reps))
    ratio = kern["dc_season_live<false>"]["us_per_call"] / kern["dc_season<false>"]["us_per_call"]
    ref_s = restatement_seconds()
    res = {"simulations": N, "draws": S, "teams": T, "fixtures": T * (T - 1) - len(STATES), "in_play": len(STATES),
           "wall": wall, "kernel": kern, "kernel_ratio": ratio, "restatement_seconds_at_1000_simulations": ref_s}
    lines = [f"{N} simulations, {S} draws, {T} teams: {T * (T - 1) - len(STATES)} fixtures + {len(STATES)} in play "
             f"v {T * (T - 1)} fixtures from kick-off"]
    lines.append(f"  dc_season_live<false> {kern['dc_season_live<false>']['us_per_call']:.1f} us per call, "
                 f"dc_season<false> {kern['dc_season<false>']['us_per_call']:.1f} us: x {ratio:.2f}")
    lines.append(f"  live_loglik {kern['live_loglik']['us_per_call']:.1f} us, live_weights "
                 f"{kern['live_weights']['us_per_call']:.1f} us per call")
    for mode in KERNELS:
        w = wall[mode]
        lines.append(f"  {mode}: device call {w['device_call']['median_ms']:.3f} ms, public method end to end "
                     f"{w['end_to_end']['median_ms']:.3f} ms (medians of {args.reps})")
    lines.append(f"  the numpy restatement at 1000 simulations: {ref_s:.2f} s")
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(args.out, "live_bench.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.join(args.out, "live_bench.txt"), "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
