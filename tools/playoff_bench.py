"""simulate_season with play-offs on one MI355X (csrc/dc_playoff.hip.h) next to the same build's simulate_season
without them, launched in the same run at the same shape: the Championship's format on a hand-built Dixon-Coles
posterior (S = 1000 draws) -- 24 teams, the whole double round robin of 552 fixtures still to play, then 3rd to 6th
in the bracket [5, 2, 4, 3] with legs (2, 1) and venues ("seed", "neutral").

    python tools/playoff_bench.py [--out DIR] [--reps N]

Reports, at 1e3 / 1e4 / 1e5 simulated seasons: the kernel time of dc_playoff<false> and dc_season<false> from a
`rocprofv3 --kernel-trace --stats` run of its own (a child process per size; profiler off for the wall times), the
end-to-end wall time of `simulate_season` with and without `playoffs` (medians of N calls after a warm-up,
aggregates only) and the ratios with / without.  Writes playoff_bench.json and playoff_bench.txt under --out
(default: profiles/playoff)."""
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
sys.path[:0] = [os.path.join(ROOT, "bpl-next_amd")]

import numpy as np  # noqa: E402

from bpl import DixonColesMatchPredictor  # noqa: E402

SIZES = (1_000, 10_000, 100_000)
T, S = 24, 1000
PLAYOFFS = {"bracket": [5, 2, 4, 3], "legs": (2, 1), "venue": ("seed", "neutral")}
# the overall-order kernels as rocprofv3 names them; neither name is a part of the other
KERNELS = {"playoffs": "dc_playoff<false>", "league_only": "dc_season<false>"}


def model():
    rs = np.random.RandomState(0)
    m = DixonColesMatchPredictor()
    m.teams = np.array([f"t{i:02d}" for i in range(T)])
    m._teams_dict = {t: i for i, t in enumerate(m.teams)}
    m.attack, m.defence = rs.normal(0, 0.3, (S, T)), rs.normal(0, 0.3, (S, T))
    m.home_advantage, m.corr_coef = rs.normal(0.25, 0.05, S), rs.uniform(-0.1, 0.1, S)
    return m


def calls(n):
    """{variant: a call of simulate_season with n simulations} on one model (one device context)."""
    m = model()
    h, a = np.nonzero(~np.eye(T, dtype=bool))
    variants = {"playoffs": {"playoffs": PLAYOFFS}, "league_only": {}}
    return {name: (lambda seed, extra=extra: m.simulate_season(h, a, num_simulations=n, random_state=seed, **extra))
            for name, extra in variants.items()}, int(h.size)


def wall_times(n, reps):
    out = {}
    for name, call in calls(n)[0].items():
        call(1)   # warm-up: context, upload, code object
        ts = []
        for r in range(reps):
            t0 = time.perf_counter()
            call(2 + r)
            ts.append(time.perf_counter() - t0)
        out[name] = {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * float(np.min(ts)),
                     "max_ms": 1e3 * float(np.max(ts)), "reps": reps}
    return out


def kernel_times(n, reps):
    """Both kernels' mean duration over the calls of a child run under rocprofv3 (its output goes to a temporary
    directory, removed afterwards)."""
    d = tempfile.mkdtemp(prefix=f"playoff_rocprof_{n}_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--child", str(n), "--reps", str(reps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise RuntimeError(f"rocprofv3 run for {n} exited {r.returncode}: {r.stderr[-2000:]}")
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    for name, kernel in KERNELS.items():
                        if kernel in row["Name"]:
                            out[name] = {"calls": int(row["Calls"]), "mean_us": float(row["AverageNs"]) / 1e3,
                                         "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
        if set(out) != set(KERNELS):
            raise RuntimeError(f"the rocprofv3 stats of the {n} run hold {sorted(out)}, not {sorted(KERNELS)}")
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "playoff"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        wall_times(int(args.child), args.reps)
        return
    os.makedirs(args.out, exist_ok=True)
    fixtures = T * (T - 1)
    res = {"setup": f"Dixon-Coles model, {T} teams, {fixtures} fixtures, S = {S} draws; bracket {PLAYOFFS['bracket']}, "
                    f"legs {PLAYOFFS['legs']}, venue {PLAYOFFS['venue']}", "sizes": {}}
    lines = [res["setup"]]
    for n in SIZES:
        wall, kern = wall_times(n, args.reps), kernel_times(n, args.reps)
        ratio = {"kernel": kern["playoffs"]["mean_us"] / kern["league_only"]["mean_us"],
                 "wall": wall["playoffs"]["median_ms"] / wall["league_only"]["median_ms"]}
        res["sizes"][str(n)] = {"wall": wall, "kernel": kern, "ratio": ratio}
        lines.append(f"  {n:>7} seasons: dc_playoff {kern['playoffs']['mean_us']:9.1f} us, dc_season "
                     f"{kern['league_only']['mean_us']:9.1f} us: x {ratio['kernel']:.2f}; simulate_season end to end "
                     f"{wall['playoffs']['median_ms']:.3f} ms v {wall['league_only']['median_ms']:.3f} ms: "
                     f"x {ratio['wall']:.2f} (medians of {args.reps})")
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(args.out, "playoff_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(args.out, "playoff_bench.txt"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
