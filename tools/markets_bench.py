"""predict_markets on one MI355X (csrc/dc_market.hip.h) at the two cases of tools/loglik_bench.py, max_goals = 15:

    league      380 fixtures x 4000 draws x 12 markets (the usual board: outcomes, over / under 2.5, both teams
                to score, clean sheets, a handicap, expected goals)
    world_cup   40 000 fixtures x 4000 draws x 3 markets (home win, over 2.5, both teams to score)

    python tools/markets_bench.py [--out DIR] [--reps N]

Reports per case: the kernel times of `market_values` and `market_summary` (summed over the chunks of a call) from
a `rocprofv3 --kernel-trace --stats` run of its own (a child process; profiler off for the wall times); the
float64 operation count (G+1)^2 (1 + K) S n of the values kernel's design and the share of the float64 vector
rate (78.6 TFLOP/s = 39.3e12 fma lanes per second; a multiplication issues like an fma) that count over the
`market_values` time comes to; the end-to-end wall time of the device call (HipContext.market_summary: H2D +
kernels + D2H, median of N after a warm-up that also builds the team-major copies) and of the public
`predict_markets(data, markets)`; and the numpy restatement (tests/markets_ref.py) on the first --ref-fixtures
fixtures, its time scaled to all of them, with the largest difference of the means and quantiles.  Writes
markets_bench.json and markets_bench.txt under --out (default: profiles/markets)."""
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

from loglik_bench import CASES, S, case  # noqa: E402

G = 15
QS = (0.05, 0.5, 0.95)
KERNELS = ("market_values", "market_summary")
FMA_LANES_PER_S = 39.3e12   # float64 vector rate of one MI355X (78.6 TFLOP/s)


def markets_of(name):
    from bpl import markets as MK

    if name == "world_cup":
        return {"home_win": MK.home_win(), "over_2.5": MK.total_over(2.5), "btts": MK.btts()}
    return {"home_win": MK.home_win(), "draw": MK.draw(), "away_win": MK.away_win(), "over_2.5": MK.total_over(2.5),
            "under_2.5": MK.total_under(2.5), "btts": MK.btts(), "clean_sheet_home": MK.clean_sheet("home"),
            "clean_sheet_away": MK.clean_sheet("away"), "handicap_home_-1": MK.handicap(-1),
            "goals_home": MK.goals("home"), "goals_away": MK.goals("away"), "total_goals": MK.total_goals()}


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * float(np.min(ts)),
            "max_ms": 1e3 * float(np.max(ts)), "reps": reps}


def device_call(name):
    """(model, data, markets, the device call of the case as a function)."""
    import markets_ref as MR

    m, data = case(name)
    mk = markets_of(name)
    W = MR.weights_of(mk, G)
    (_, device, kw), = m._fixture_groups(data, with_goals=False)[0]
    dev = device()
    return m, data, mk, lambda: dev.market_summary(**kw, max_goals=G, weights=W, quantiles=QS)


def kernel_times(name, reps):
    """Per device call: the summed duration of each kernel's launches (one per chunk of fixtures)."""
    d = tempfile.mkdtemp(prefix="markets_rocprof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(reps)]
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
                            calls = int(row["Calls"])
                            out[k] = {"launches": calls, "launches_per_call": calls / (reps + 1),
                                      "us_per_call": float(row["TotalDurationNs"]) / 1e3 / (reps + 1)}
        if set(out) != set(KERNELS):
            raise RuntimeError(f"the rocprofv3 stats hold {sorted(out)}, not {KERNELS}")
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "markets"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-fixtures", type=int, default=100)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        call = device_call(args.child)[3]
        for _ in range(args.reps + 1):
            call()
        return
    import markets_ref as MR

    os.makedirs(args.out, exist_ok=True)
    res, lines = {}, []
    for name in CASES:
        m, data, mk, call = device_call(name)
        data = {k: v for k, v in data.items() if not k.endswith("_goals")}
        n, K = len(data["home_team"]), len(mk)
        wall = {"device_call": timed(call, args.reps),
                "predict_markets": timed(lambda: m.predict_markets(data, mk, max_goals=G, quantiles=QS), args.reps)}
        kern = kernel_times(name, args.reps)
        got = m.predict_markets(data, mk, max_goals=G, quantiles=QS)
        k = min(args.ref_fixtures, n)
        sub = {key: v[:k] for key, v in data.items()}
        t0 = time.perf_counter()
        ref = MR.predict_markets(m, sub, mk, G, QS)
        ref_s = time.perf_counter() - t0
        diff = max(float(np.abs(ref[key] - got[key][..., :k]).max()) for key in ("mean", "sd", "quantile"))
        ops = (G + 1) ** 2 * (1 + K) * S * n
        t_values = kern["market_values"]["us_per_call"] * 1e-6
        share = ops / FMA_LANES_PER_S / t_values
        res[name] = {"draws": S, "fixtures": n, "markets": list(mk), "max_goals": G, "quantiles": list(QS), "wall": wall,
                     "kernel": kern, "float64_operations": ops, "float64_valu_share_of_market_values": share,
                     "numpy": {"fixtures": k, "seconds": ref_s, "scaled_to_all_fixtures_s": ref_s * n / k,
                               "max_abs_diff": diff}}
        i = list(mk).index("home_win")
        lines += [
            f"{name}: {n} fixtures x {S} draws x {K} markets, max_goals = {G}, quantiles {QS}",
            f"  market_values {kern['market_values']['us_per_call']:.1f} us per call "
            f"({kern['market_values']['launches_per_call']:.0f} launches), market_summary "
            f"{kern['market_summary']['us_per_call']:.1f} us per call",
            f"  float64 operations (G+1)^2 (1+K) S n = {ops:.3e}: {ops / t_values / 1e12:.2f} T operations/s in "
            f"market_values = {100 * share:.1f} % of the float64 vector rate ({FMA_LANES_PER_S / 1e12:.1f}e12 fma lanes/s)",
            f"  device call {wall['device_call']['median_ms']:.3f} ms end to end, predict_markets(data, markets) "
            f"{wall['predict_markets']['median_ms']:.3f} ms (medians of {args.reps})",
            f"  numpy restatement on the first {k} fixtures {ref_s:.2f} s, scaled to {n}: {ref_s * n / k:.0f} s; "
            f"max |difference| of mean, sd and quantiles {diff:.2e}",
            f"  fixture 0, home_win: mean {got['mean'][i, 0]:.4f}, sd {got['sd'][i, 0]:.4f}, 5 % / median / 95 % "
            + " / ".join(f"{v:.4f}" for v in got["quantile"][i, :, 0])]
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(args.out, "markets_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(args.out, "markets_bench.txt"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
