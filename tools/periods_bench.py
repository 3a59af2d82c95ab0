"""predict_periods on one MI355X (csrc/dc_period.hip.h) at the league case of tools/loglik_bench.py:

    380 fixtures x 4000 draws x 9 markets (the half-time/full-time table), max_goals = 15, split = 0.45

    python tools/periods_bench.py [--out DIR] [--reps N]

Reports: the kernel times of `period_values` and `market_summary` from a `rocprofv3 --kernel-trace --stats` run of
its own (a child process; profiler off for the wall times), and in the same way `market_values` and
`market_summary` of `predict_markets` with 9 markets at the same shape; the float64 operation count
T^2 (1 + K) S n, T = (G+1)(G+2)/2, of the values kernel's design, the instructions a launch issues
(T^2 (1 + 8) + 2 per step of the first-period away count, per draw, fixture and pass of 8) and the share of the
float64 vector rate (78.6 TFLOP/s = 39.3e12 fma lanes per second; a multiplication issues like an fma) each comes to
over the `period_values` time; the end-to-end wall times of the device calls and of the public methods (medians of N
after a warm-up); the only route there was before -- `predict_in_play(return_draws=True)` over all (G+1)^2 states of
a fixture, exp(evidence) x value recombined in numpy -- on the first --route-fixtures fixtures, its time SCALED to
all of them; and the numpy restatement (tests/periods_ref.py) on the first --ref-fixtures fixtures, scaled likewise,
with the largest difference of the means, sds and quantiles.  Writes periods_bench.json and periods_bench.txt under
--out (default: profiles/periods)."""
import argparse
import csv
import glob
import itertools
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

from loglik_bench import S, case  # noqa: E402
from markets_bench import FMA_LANES_PER_S, timed  # noqa: E402

G = 15
QS = (0.05, 0.5, 0.95)
SPLIT = 0.45
PICKS = ("home", "draw", "away")
KERNELS = {"periods": ("period_values", "market_summary"), "markets": ("market_values", "market_summary")}
BLOCK, KPASS = 8, 8   # csrc/dc_period.hip.h PERIOD_DB, PERIOD_KPASS


def period_markets():
    from bpl import periods as PD

    return {f"{first}/{final}": PD.ht_ft(first, final) for first, final in itertools.product(PICKS, repeat=2)}


def full_time_markets():
    from bpl import markets as MK

    return {"home_win": MK.home_win(), "draw": MK.draw(), "away_win": MK.away_win(), "over_2.5": MK.total_over(2.5),
            "under_2.5": MK.total_under(2.5), "btts": MK.btts(), "clean_sheet_home": MK.clean_sheet("home"),
            "goals_home": MK.goals("home"), "total_goals": MK.total_goals()}


def league():
    m, data = case("league")
    return m, {k: v for k, v in data.items() if not k.endswith("_goals")}


def device_call(which):
    """The device call of predict_periods ("periods") or of predict_markets ("markets") as a function."""
    import markets_ref as MR
    import periods_ref as PR

    m, data = league()
    (_, device, kw), = m._fixture_groups(data, with_goals=False)[0]
    dev = device()
    if which == "periods":
        W = PR.weights_of(period_markets(), G)
        split = np.full(len(data["home_team"]), SPLIT)
        return lambda: dev.period_summary(**kw, split=split, max_goals=G, weights=W, quantiles=QS)
    W = MR.weights_of(full_time_markets(), G)
    return lambda: dev.market_summary(**kw, max_goals=G, weights=W, quantiles=QS)


def kernel_times(which, reps):
    """Per device call: the summed duration of each kernel's launches."""
    d = tempfile.mkdtemp(prefix="periods_rocprof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--child", which, "--reps", str(reps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
        if r.returncode != 0:
            raise RuntimeError(f"the rocprofv3 run exited {r.returncode}: {r.stderr[-2000:]}")
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    for k in KERNELS[which]:
                        if k in row["Name"]:
                            calls = int(row["Calls"])
                            out[k] = {"launches": calls, "launches_per_call": calls / (reps + 1),
                                      "us_per_call": float(row["TotalDurationNs"]) / 1e3 / (reps + 1)}
        if set(out) != set(KERNELS[which]):
            raise RuntimeError(f"the rocprofv3 stats hold {sorted(out)}, not {KERNELS[which]}")
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def in_play_route(m, data, fixtures):
    """The half-time/full-time table of the first `fixtures` fixtures by the route there was before: every state
    (a, b) at the split as a match in progress, exp(evidence) x the final-outcome values, summed per half-time
    outcome in numpy and summarised there.  Returns (seconds, mean [9, fixtures])."""
    import markets_ref as MR
    from bpl import markets as MK

    final = {"home": MK.home_win(), "draw": MK.draw(), "away": MK.away_win()}
    a, b = (v.ravel() for v in np.meshgrid(np.arange(G + 1), np.arange(G + 1), indexing="ij"))
    first = np.stack([a > b, a == b, a < b]).astype(np.float64)   # [3, states]
    mean = np.empty((9, fixtures))
    t0 = time.perf_counter()
    for i in range(fixtures):
        live = {k: [v[i]] * a.size for k, v in data.items()}
        live.update(home_goals=a, away_goals=b, elapsed=np.full(a.size, SPLIT))
        r = m.predict_in_play(live, final, max_goals=G, quantiles=(), reweight=False, return_draws=True)
        joint = np.exp(r["draw_log_evidence"])[:, None, :] * r["draws"]   # [S, final, states]
        v = np.einsum("hc,sfc->shf", first, joint).reshape(S, 9, 1)
        mean[:, i] = MR.summarise(v, QS)["mean"][:, 0]
    return time.perf_counter() - t0, mean


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "periods"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-fixtures", type=int, default=2)
    ap.add_argument("--route-fixtures", type=int, default=4)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        call = device_call(args.child)
        for _ in range(args.reps + 1):
            call()
        return
    import periods_ref as PR

    os.makedirs(args.out, exist_ok=True)
    m, data = league()
    n = len(data["home_team"])
    pm, fm = period_markets(), full_time_markets()
    K = len(pm)
    wall = {"period_summary": timed(device_call("periods"), args.reps),
            "predict_periods": timed(lambda: m.predict_periods(data, pm, split=SPLIT, max_goals=G, quantiles=QS),
                                     args.reps),
            "market_summary": timed(device_call("markets"), args.reps),
            "predict_markets": timed(lambda: m.predict_markets(data, fm, max_goals=G, quantiles=QS), args.reps)}
    kern = {which: kernel_times(which, args.reps) for which in KERNELS}
    got = m.predict_periods(data, pm, split=SPLIT, max_goals=G, quantiles=QS)
    route_s, route_mean = in_play_route(m, data, args.route_fixtures)
    route_diff = float(np.abs(route_mean - got["mean"][:, :args.route_fixtures]).max())
    k = min(args.ref_fixtures, n)
    sub = {key: v[:k] for key, v in data.items()}
    t0 = time.perf_counter()
    ref = PR.predict_periods(m, sub, pm, SPLIT, G, QS)
    ref_s = time.perf_counter() - t0
    diff = max(float(np.abs(ref[key] - got[key][..., :k]).max()) for key in ("mean", "sd", "quantile"))
    T = (G + 1) * (G + 2) // 2
    passes = -(-K // KPASS)
    steps = T * sum(G - d0 + 1 for d0 in range(0, G + 1, BLOCK))   # steps of the first-period away count
    ops = T * T * (1 + K) * S * n
    issued = (T * T * (1 + KPASS) + 2 * steps) * passes * S * n
    t_values = kern["periods"]["period_values"]["us_per_call"] * 1e-6
    res = {"draws": S, "fixtures": n, "markets": list(pm), "max_goals": G, "split": SPLIT, "quantiles": list(QS),
           "wall": wall, "kernel": kern, "cells_per_draw_fixture_pass": T * T, "float64_operations": ops,
           "float64_instructions_issued": issued,
           "float64_valu_share_of_period_values": {"counted": ops / FMA_LANES_PER_S / t_values,
                                                   "issued": issued / FMA_LANES_PER_S / t_values},
           "weight_bytes_per_wave_and_pass": T * T * 64,
           "in_play_route": {"fixtures": args.route_fixtures, "seconds": route_s,
                             "scaled_to_all_fixtures_s": route_s * n / args.route_fixtures,
                             "max_abs_diff_of_means": route_diff},
           "numpy": {"fixtures": k, "seconds": ref_s, "scaled_to_all_fixtures_s": ref_s * n / k, "max_abs_diff": diff}}
    kp, km = kern["periods"], kern["markets"]
    i = list(pm).index("draw/home")
    lines = [
        f"league: {n} fixtures x {S} draws x {K} markets (half-time/full-time), max_goals = {G}, split = {SPLIT}, "
        f"quantiles {QS}",
        f"  period_values {kp['period_values']['us_per_call']:.1f} us per call "
        f"({kp['period_values']['launches_per_call']:.0f} launches), market_summary "
        f"{kp['market_summary']['us_per_call']:.1f} us per call",
        f"  predict_markets, 9 markets at the same shape: market_values {km['market_values']['us_per_call']:.1f} us, "
        f"market_summary {km['market_summary']['us_per_call']:.1f} us per call",
        f"  T^2 = {T * T} cells per draw, fixture and pass; {T * T * 64} bytes of weights per wave and pass",
        f"  float64 operations T^2 (1+K) S n = {ops:.3e}: {ops / t_values / 1e12:.2f} T operations/s in period_values = "
        f"{100 * ops / FMA_LANES_PER_S / t_values:.1f} % of the float64 vector rate "
        f"({FMA_LANES_PER_S / 1e12:.1f}e12 fma lanes/s); instructions issued ({passes} passes of {KPASS}) {issued:.3e} = "
        f"{100 * issued / FMA_LANES_PER_S / t_values:.1f} %",
        f"  device call {wall['period_summary']['median_ms']:.3f} ms end to end, predict_periods(data, markets) "
        f"{wall['predict_periods']['median_ms']:.3f} ms; market_summary {wall['market_summary']['median_ms']:.3f} ms, "
        f"predict_markets {wall['predict_markets']['median_ms']:.3f} ms (medians of {args.reps})",
        f"  the route before (predict_in_play over {(G + 1) ** 2} states per fixture + numpy) on the first "
        f"{args.route_fixtures} fixtures {route_s:.2f} s, SCALED to {n}: {route_s * n / args.route_fixtures:.0f} s; "
        f"max |difference| of the means {route_diff:.2e}",
        f"  numpy restatement on the first {k} fixtures {ref_s:.2f} s, SCALED to {n}: {ref_s * n / k:.0f} s; "
        f"max |difference| of mean, sd and quantiles {diff:.2e}",
        f"  fixture 0, draw/home: mean {got['mean'][i, 0]:.4f}, sd {got['sd'][i, 0]:.4f}, 5 % / median / 95 % "
        + " / ".join(f"{v:.4f}" for v in got["quantile"][i, :, 0])]
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(args.out, "periods_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(args.out, "periods_bench.txt"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
