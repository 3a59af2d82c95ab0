"""Posterior predictive checks on one MI355X: the `dc_ppc` kernel (csrc/dc_ppc.hip.h) for the two cases of
tools/loglik_bench.py, R = 4000 replications of every fixture, with the numpy restatement (tests/ppc_ref.py) as
the CPU yardstick.

    league      Dixon-Coles, 20 teams, the 380 fixtures of a double round robin, S = 4000 draws
    world_cup   World-Cup model, 200 teams, 6 confederations, 40 000 fixtures (half neutral), S = 4000 draws

    python tools/ppc_bench.py [--out DIR] [--reps N]

Reports per case: the kernel time of `dc_ppc` from a `rocprofv3 --kernel-trace --stats` run of its own (a child
process, profiler off for the wall times), the end-to-end wall time of the device call (HipContext.ppc: H2D +
kernel + D2H, median of N after a warm-up) and of the public `posterior_predictive_check(data)` (host checks,
name lookups and statistics included), and the numpy restatement's time.  The restatement draws the
replications one at a time, so it is timed on the first R_REF replications and scaled to R; those
replications are compared with the device's, scoreline by scoreline.  Writes ppc_bench.json and ppc_bench.txt
under --out (default: profiles/ppc)."""
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

R = 4000
R_REF = {"league": 4000, "world_cup": 100}
SEED = 7
MAX_GOALS = 6
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


def device_args(m, data, reps):
    """(device, positional args, keyword args) of the one HipContext.ppc call posterior_predictive_check makes."""
    from bpl._ffi import prng_key as _prng_key

    (_, device, kw), = m._loglik_groups(data)[0]
    idx = np.union1d(kw["home_idx"], kw["away_idx"])
    hs, as_ = np.searchsorted(idx, kw["home_idx"]), np.searchsorted(idx, kw["away_idx"])
    args = (kw["home_idx"], kw["away_idx"], hs, as_, idx.size, MAX_GOALS, reps, _prng_key(SEED))
    return device, args, {nm: kw[nm] for nm in ("neutral", "conf") if nm in kw}


def wall_times(name, reps):
    m, data = case(name)
    device, args, kw = device_args(m, data, R)
    dev = device()
    dev.ppc(*args, **kw)   # warm-up: context, upload, code object
    out = {}
    for label, fn in (("device_call", lambda: dev.ppc(*args, **kw)),
                      ("ppc", lambda: m.posterior_predictive_check(data, num_replications=R, random_state=SEED,
                                                                   max_goals=MAX_GOALS))):
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
    """dc_ppc's mean duration over the calls of a child run under rocprofv3 (output in a temporary
    directory, removed afterwards)."""
    d = tempfile.mkdtemp(prefix=f"ppc_rocprof_{name}_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(reps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
        if r.returncode != 0:
            raise RuntimeError(f"rocprofv3 run for {name} exited {r.returncode}: {r.stderr[-2000:]}")
        out = None
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    if "dc_ppc" in row["Name"]:
                        out = {"calls": int(row["Calls"]), "mean_us": float(row["AverageNs"]) / 1e3,
                               "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
        if out is None:
            raise RuntimeError(f"no dc_ppc row in the rocprofv3 stats of the {name} run")
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def numpy_yardstick(name):
    """The restatement on the first R_REF replications, timed, and compared with the device's."""
    import ppc_ref as PR
    from bpl._ffi import prng_key as _prng_key

    m, data = case(name)
    r_ref = R_REF[name]
    t0 = time.perf_counter()
    x, y, flagged = PR.replicate(m, data, r_ref, _prng_key(SEED))
    t1 = time.perf_counter()
    got = m.posterior_predictive_check(data, num_replications=r_ref, random_state=SEED, max_goals=MAX_GOALS,
                                       return_replications=True)["replications"]
    ok = ~flagged
    same = bool(np.array_equal(got["home_goals"][ok], x[ok]) and np.array_equal(got["away_goals"][ok], y[ok]))
    return {"replications": r_ref, "seconds": t1 - t0, "seconds_scaled_to_R": (t1 - t0) * R / r_ref,
            "flagged_replications": int(flagged.sum()), "unflagged_scorelines_equal": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppc"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        m, data = case(args.child)
        device, a, kw = device_args(m, data, R)
        dev = device()
        for _ in range(args.reps + 1):
            dev.ppc(*a, **kw)
        return
    os.makedirs(args.out, exist_ok=True)
    res, lines = {"draws": S, "replications": R, "max_goals": MAX_GOALS, "cases": {}}, []
    for name in CASES:
        m, data = case(name)
        n = len(data["home_goals"])
        wall = wall_times(name, args.reps)
        k = kernel_time(name, args.reps)
        ref = numpy_yardstick(name)
        res["cases"][name] = {"fixtures": n, "teams": len(m.teams), "wall": wall, "kernel": k, "numpy": ref}
        lines.append(f"{name}: {len(m.teams)} teams, {n} fixtures, S = {S} draws, R = {R} replications, "
                     f"max_goals = {MAX_GOALS}")
        lines.append(f"  dc_ppc kernel {k['mean_us']:.1f} us (min {k['min_us']:.1f}, max {k['max_us']:.1f}, "
                     f"{k['calls']} calls) = {n * R / k['mean_us'] / 1e3:.2f} G scorelines/s")
        lines.append(f"  device call {wall['device_call']['median_ms']:.3f} ms end to end, "
                     f"posterior_predictive_check(data) {wall['ppc']['median_ms']:.3f} ms (medians of {args.reps})")
        lines.append(f"  numpy restatement: {ref['seconds']:.3f} s for {ref['replications']} replications, "
                     f"{ref['seconds_scaled_to_R']:.2f} s scaled to R = {R}; "
                     f"{ref['seconds_scaled_to_R'] * 1e3 / wall['device_call']['median_ms']:.0f}x the device call; "
                     f"scorelines {'equal' if ref['unflagged_scorelines_equal'] else 'NOT EQUAL'} outside "
                     f"{ref['flagged_replications']} flagged replications")
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(args.out, "ppc_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(args.out, "ppc_bench.txt"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
