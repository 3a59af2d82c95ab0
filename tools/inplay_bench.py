"""predict_in_play on one MI355X (csrc/dc_inplay.hip.h) at the two cases of tools/markets_bench.py, max_goals = 15,
with a state per fixture drawn as in the tests (score from {0, 1, 2, 3}^2, elapsed from (0, 1)):

    league      380 fixtures x 4000 draws x 12 markets
    world_cup   40 000 fixtures x 4000 draws x 3 markets

    python tools/inplay_bench.py [--out DIR] [--reps N]

Reports per case: the kernel times of `inplay_values` and `inplay_summary` (summed over the chunks of a call) from
a `rocprofv3 --kernel-trace --stats` run of its own (a child process; profiler off for the wall times); the
end-to-end wall time of the device call (HipContext.inplay_summary: H2D + kernels + D2H, median of N after a
warm-up that also builds the team-major copies) and of the public `predict_in_play(data, markets)`; the same four
figures for `predict_markets` at the same shape on the same box (the yardstick: `inplay_values` walks at most the
cells `market_values` walks; `inplay_summary` sorts where `market_summary` selects); and the numpy restatement
(tests/inplay_ref.py) on the first --ref-fixtures fixtures, its time scaled to all of them, with the largest
difference of the means and the share of quantile cells that differ.  Writes inplay_bench.json and
inplay_bench.txt under --out (default: profiles/inplay)."""
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
from markets_bench import G, QS, markets_of, timed  # noqa: E402

KERNELS = {"in_play": ("inplay_values", "inplay_summary"), "markets": ("market_values", "market_summary")}


def in_play_case(name):
    """(model, data with a state per fixture, markets)."""
    import inplay_ref as IR

    m, data = case(name)
    return m, IR.with_states(data, G, seed=7), markets_of(name)


def device_calls(name):
    """(model, data, markets, {"in_play": the device call of the case, "markets": predict_markets' at the same shape})."""
    import markets_ref as MR

    m, data, mk = in_play_case(name)
    W = MR.weights_of(mk, G)
    (_, device, kw), = m._fixture_groups(data, with_goals=True)[0]
    (_, _, kw0), = m._fixture_groups(data, with_goals=False)[0]
    dev = device()
    t = np.asarray(data["elapsed"], dtype=np.float64)
    return m, data, mk, {"in_play": lambda: dev.inplay_summary(**kw, elapsed=t, max_goals=G, weights=W, quantiles=QS),
                         "markets": lambda: dev.market_summary(**kw0, max_goals=G, weights=W, quantiles=QS)}


def kernel_times(name, which, reps):
    """Per device call: the summed duration of each kernel's launches (one per chunk of fixtures)."""
    d = tempfile.mkdtemp(prefix="inplay_rocprof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--child", name, "--which", which, "--reps", str(reps)]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inplay"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-fixtures", type=int, default=100)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--which", default="in_play", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        call = device_calls(args.child)[3][args.which]
        for _ in range(args.reps + 1):
            call()
        return
    import inplay_ref as IR

    os.makedirs(args.out, exist_ok=True)
    res, lines = {}, []
    for name in CASES:
        m, data, mk, calls = device_calls(name)
        n, K = len(data["home_team"]), len(mk)
        wall = {"device_call": timed(calls["in_play"], args.reps),
                "predict_in_play": timed(lambda: m.predict_in_play(data, mk, max_goals=G, quantiles=QS), args.reps),
                "markets_device_call": timed(calls["markets"], args.reps),
                "predict_markets": timed(lambda: m.predict_markets(data, mk, max_goals=G, quantiles=QS), args.reps)}
        kern = {which: kernel_times(name, which, args.reps) for which in KERNELS}
        got = m.predict_in_play(data, mk, max_goals=G, quantiles=QS)
        k = min(args.ref_fixtures, n)
        sub = {key: v[:k] for key, v in data.items()}
        t0 = time.perf_counter()
        ref = IR.predict_in_play(m, sub, mk, G, QS)
        ref_s = time.perf_counter() - t0
        diff = max(float(np.abs(ref[key] - got[key][..., :k]).max()) for key in ("mean", "sd", "log_evidence"))
        qdiff = float(np.abs(ref["quantile"] - got["quantile"][..., :k]).max())
        res[name] = {"draws": S, "fixtures": n, "markets": list(mk), "max_goals": G, "quantiles": list(QS), "wall": wall,
                     "kernel": kern,
                     "numpy": {"fixtures": k, "seconds": ref_s, "scaled_to_all_fixtures_s": ref_s * n / k,
                               "max_abs_diff": diff, "max_abs_diff_quantile": qdiff}}
        ki, km = kern["in_play"], kern["markets"]
        i = list(mk).index("home_win")
        lines += [
            f"{name}: {n} fixtures x {S} draws x {K} markets, max_goals = {G}, quantiles {QS}",
            f"  inplay_values {ki['inplay_values']['us_per_call']:.1f} us per call "
            f"({ki['inplay_values']['launches_per_call']:.0f} launches), inplay_summary "
            f"{ki['inplay_summary']['us_per_call']:.1f} us per call",
            f"  market_values {km['market_values']['us_per_call']:.1f} us per call "
            f"({km['market_values']['launches_per_call']:.0f} launches), market_summary "
            f"{km['market_summary']['us_per_call']:.1f} us per call: values x"
            f"{ki['inplay_values']['us_per_call'] / km['market_values']['us_per_call']:.2f}, summary x"
            f"{ki['inplay_summary']['us_per_call'] / km['market_summary']['us_per_call']:.2f}",
            f"  device call {wall['device_call']['median_ms']:.3f} ms end to end (market_summary "
            f"{wall['markets_device_call']['median_ms']:.3f} ms), predict_in_play(data, markets) "
            f"{wall['predict_in_play']['median_ms']:.3f} ms (predict_markets "
            f"{wall['predict_markets']['median_ms']:.3f} ms) (medians of {args.reps})",
            f"  numpy restatement on the first {k} fixtures {ref_s:.2f} s, scaled to {n}: {ref_s * n / k:.0f} s; "
            f"max |difference| of mean, sd and log evidence {diff:.2e}, of the quantiles {qdiff:.2e}",
            f"  fixture 0 ({data['home_goals'][0]}-{data['away_goals'][0]} at {data['elapsed'][0]:.2f}), home_win: mean "
            f"{got['mean'][i, 0]:.4f}, sd {got['sd'][i, 0]:.4f}, 5 % / median / 95 % "
            + " / ".join(f"{v:.4f}" for v in got["quantile"][i, :, 0]) + f", ess {got['ess'][0]:.0f} of {S}"]
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(args.out, "inplay_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(args.out, "inplay_bench.txt"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
