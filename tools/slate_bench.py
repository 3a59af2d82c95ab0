"""predict_slate on one MI355X (csrc/dc_slate.hip.h) on the league case of tools/loglik_bench.py (20 teams, 380
fixtures, 4000 draws), max_goals = 15, every leg pick("home") (the total is the number of home wins), four shapes:

    1x10     one slate of 10 fixtures
    20x6     20 slates of 6
    38x10    38 slates of 10: the 380 fixtures
    1x127    one slate of 127 0/1 legs: P + 1 = 128, the limit

    python tools/slate_bench.py [--out DIR] [--reps N]

Reports per shape: the kernel times of `slate_values` and of the two `market_summary` launches (over the slates,
over the fixtures) from ONE `rocprofv3 --kernel-trace --stats` run of its own (a child process that makes
reps + 1 device calls per shape in a fixed order; the dispatches of the trace are dealt to the shapes in that
order and the first call of each is dropped; profiler off for the wall times); the counted float64 work of the
walk, 9 (G+1)^2 S n instructions (the same as one `market_values` pass), plus the convolution's fma, and the
share of the float64 vector rate (78.6 TFLOP/s = 39.3e12 fma lanes per second) that count over the `slate_values` time comes to; the wall time of the
device call (HipContext.slate_summary: H2D + kernels + D2H, median of N after a warm-up) and of the public
`predict_slate`; the numpy restatement (tests/slate_ref.py) on the first --ref-slates slates, scaled to all; and
the previous route at the same shape: `predict_markets(return_draws=True)` with the three outcome indicators,
then a numpy convolution loop over the fixtures on the [draws, fixtures] values.  Every wall time is the median
of --reps calls.  The same child also runs `market_values` with 8 markets on the 380 fixtures: its time stands
beside `slate_values` at 38x10.  Every shape fits the library's default workspace, so a device call is one chunk:
three dispatches, which is what the dealing of the trace relies on and checks.  Writes slate_bench.json and slate_bench.txt under --out (default: profiles/slate)."""
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

from loglik_bench import S, case  # noqa: E402

G = 15
QS = (0.05, 0.5, 0.95)
SHAPES = {"1x10": (1, 10), "20x6": (20, 6), "38x10": (38, 10), "1x127": (1, 127)}
FMA_LANES_PER_S = 39.3e12   # float64 vector rate of one MI355X (78.6 TFLOP/s)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * float(np.min(ts)),
            "max_ms": 1e3 * float(np.max(ts)), "reps": reps}


def shape_data(data, name):
    """(data of the shape's fixtures without the goals, slate labels)."""
    J, N = SHAPES[name]
    sub = {k: list(v[:J * N]) for k, v in data.items() if not k.endswith("_goals")}
    return sub, np.repeat(np.arange(J), N)


def device_call(m, data, name):
    """The device call predict_slate makes for the shape, as a function."""
    from bpl import slate as SL

    sub, slate = shape_data(data, name)
    n = slate.size
    (_, device, kw), = m._fixture_groups(sub, with_goals=False)[0]
    tables, leg_table = SL.leg_tables(SL.pick("home"), n, G)
    start = np.concatenate([[0], np.cumsum(np.bincount(slate))]).astype(np.int32)
    dev = device()
    return lambda: dev.slate_summary(**kw, max_goals=G, tables=tables, leg_table=leg_table, start=start, quantiles=QS)


def markets_call(m, data):
    """market_summary with 8 markets on the 380 fixtures, as a function."""
    import markets_ref as MR
    from bpl import markets as MK

    mk = {"home_win": MK.home_win(), "draw": MK.draw(), "away_win": MK.away_win(), "over_2.5": MK.total_over(2.5),
          "under_2.5": MK.total_under(2.5), "btts": MK.btts(), "clean_sheet_home": MK.clean_sheet("home"),
          "clean_sheet_away": MK.clean_sheet("away")}
    sub = {k: v for k, v in data.items() if not k.endswith("_goals")}
    (_, device, kw), = m._fixture_groups(sub, with_goals=False)[0]
    dev, W = device(), MR.weights_of(mk, G)
    return lambda: dev.market_summary(**kw, max_goals=G, weights=W, quantiles=QS)


def child(reps):
    m, data = case("league")
    for name in SHAPES:
        call = device_call(m, data, name)
        for _ in range(reps + 1):
            call()
    call = markets_call(m, data)
    for _ in range(reps + 1):
        call()


def kernel_times(reps):
    """{shape: {kernel: us per call}} and market_values' from the dispatches of one traced child run."""
    d = tempfile.mkdtemp(prefix="slate_rocprof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
        if r.returncode != 0:
            raise RuntimeError(f"the rocprofv3 run exited {r.returncode}: {r.stderr[-2000:]}")
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    low = {k.lower(): v for k, v in row.items()}
                    rows.append((int(low["start_timestamp"]), int(low["end_timestamp"]), low["kernel_name"]))
        rows.sort()
        mine = [(e - s, n) for s, e, n in rows if any(k in n for k in ("slate_values", "market_summary", "market_values"))]
        want = len(SHAPES) * 3 * (reps + 1) + 2 * (reps + 1)
        if len(mine) != want:
            raise RuntimeError(f"the trace holds {len(mine)} dispatches of the kernels, not {want}")
        out, at = {}, 0
        for name in list(SHAPES) + ["markets_8x380"]:
            labels = ("market_values", "market_summary") if name == "markets_8x380" else \
                ("slate_values", "market_summary_slates", "market_summary_fixtures")
            per = {k: [] for k in labels}
            for c in range(reps + 1):
                for k in labels:
                    ns, kernel = mine[at]
                    at += 1
                    if k[:14] not in kernel:   # ("slate_values", "market_summary", "market_values")
                        raise RuntimeError(f"dispatch {at - 1} is {kernel}, not {k}")
                    if c > 0:   # (the first call of a shape is the warm-up)
                        per[k].append(ns / 1e3)
            out[name] = {k: {"us_per_call": float(np.median(v)), "min_us": float(np.min(v)), "max_us": float(np.max(v))}
                         for k, v in per.items()}
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def previous_route(m, sub, slate):
    """The law of the number of home wins per slate without predict_slate: the per-draw outcome probabilities of
    predict_markets, then a convolution loop over the fixtures in numpy.  Returns the mean pmf [J, P+1]."""
    from bpl import markets as MK

    r = m.predict_markets(sub, {"home_win": MK.home_win(), "draw": MK.draw(), "away_win": MK.away_win()}, max_goals=G,
                          quantiles=(), return_draws=True)["draws"]   # [S, 3, n]
    J = slate.max() + 1
    P = np.bincount(slate).max()
    out = np.zeros((J, P + 1))
    for j in range(J):
        pmf = np.zeros((r.shape[0], P + 1))
        pmf[:, 0] = 1.0
        for i in np.nonzero(slate == j)[0]:
            win, other = r[:, 0, i, None], (r[:, 1, i] + r[:, 2, i])[:, None]
            shifted = np.concatenate([np.zeros((r.shape[0], 1)), pmf[:, :-1]], axis=1)
            pmf = other * pmf + win * shifted
        out[j] = pmf.mean(axis=0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slate"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-slates", type=int, default=2)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.reps)
        return
    import slate_ref as SLR
    from bpl import slate as SL

    os.makedirs(args.out, exist_ok=True)
    m, data = case("league")
    leg = SL.pick("home")
    res, lines = {}, []
    try:
        kern = kernel_times(args.reps)
    except Exception as e:  # pylint: disable=broad-except
        kern = None
        res["kernel_times_error"] = str(e)
        lines.append(f"kernel times NOT MEASURED: {e}")
    for name, (J, N) in SHAPES.items():
        sub, slate = shape_data(data, name)
        n = slate.size
        wall = {"device_call": timed(device_call(m, data, name), args.reps),
                "predict_slate": timed(lambda: m.predict_slate(sub, leg, slate=slate, max_goals=G, quantiles=QS), args.reps),
                "previous_route": timed(lambda: previous_route(m, sub, slate), args.reps)}
        got = m.predict_slate(sub, leg, slate=slate, max_goals=G, quantiles=QS)
        prev_diff = float(np.abs(previous_route(m, sub, slate) - got["pmf"]).max())
        k = min(args.ref_slates, J)
        part = {key: v[:k * N] for key, v in sub.items()}
        t0 = time.perf_counter()
        ref = SLR.predict_slate(m, part, leg, slate[:k * N], G, QS)
        ref_s = time.perf_counter() - t0
        diff = max(float(np.abs(ref[key] - got[key][:k]).max()) for key in
                   ("pmf", "pmf_sd", "pmf_quantile", "at_least", "expected", "expected_quantile"))
        walk = 9 * (G + 1) ** 2 * S * n   # one multiplication and eight fma per cell, as one market_values pass
        conv = 2 * S * J * sum(i + 1 for i in range(N))   # sum_i (top_i + m_i)(m_i + 1) fma per draw, m_i = 1
        res[name] = {"draws": S, "slates": J, "legs_per_slate": N, "fixtures": n, "max_goals": G, "quantiles": list(QS),
                     "wall": wall, "float64_instructions_walk": walk, "fma_convolution": conv,
                     "numpy": {"slates": k, "seconds": ref_s, "scaled_to_all_slates_s": ref_s * J / k, "max_abs_diff": diff},
                     "previous_route_max_abs_diff_of_mean_pmf": prev_diff}
        lines.append(f"{name}: {J} slates x {N} legs = {n} fixtures x {S} draws, max_goals = {G}, quantiles {QS}")
        if kern:
            kk = kern[name]
            t_values = kk["slate_values"]["us_per_call"] * 1e-6
            share = (walk + conv) / FMA_LANES_PER_S / t_values
            res[name].update(kernel=kk, float64_valu_share_of_slate_values=share)
            lines += [f"  slate_values {kk['slate_values']['us_per_call']:.1f} us, market_summary over the slates "
                      f"{kk['market_summary_slates']['us_per_call']:.1f} us, over the fixtures "
                      f"{kk['market_summary_fixtures']['us_per_call']:.1f} us (medians of {args.reps} calls)",
                      f"  float64 instructions 9 (G+1)^2 S n = {walk:.3e} + {conv:.3e} fma of the convolution: "
                      f"{100 * share:.1f} % of the float64 vector rate ({FMA_LANES_PER_S / 1e12:.1f}e12 lanes/s) in slate_values"]
        lines += [f"  device call {wall['device_call']['median_ms']:.3f} ms end to end, predict_slate "
                  f"{wall['predict_slate']['median_ms']:.3f} ms (medians of {args.reps})",
                  f"  previous route (predict_markets' draws + numpy convolution loop) {wall['previous_route']['median_ms']:.1f} ms "
                  f"(median of {args.reps}); max |difference| of the mean pmf {prev_diff:.2e}",
                  f"  numpy restatement on the first {k} slates {ref_s:.2f} s, scaled to {J}: {ref_s * J / k:.1f} s; "
                  f"max |difference| {diff:.2e}",
                  f"  slate 0: P(all {N} home wins) {got['top_proba'][0]:.3e} (from posterior means "
                  f"{got['independent_pmf'][0, N]:.3e}), expected home wins {got['expected'][0]:.3f} "
                  f"[{got['expected_quantile'][0, 0]:.3f}, {got['expected_quantile'][0, -1]:.3f}]"]
    if kern:
        mv, sv = kern["markets_8x380"]["market_values"]["us_per_call"], kern["38x10"]["slate_values"]["us_per_call"]
        res["markets_8x380"] = kern["markets_8x380"]
        res["slate_values_over_market_values_380"] = sv / mv
        lines.append(f"380 fixtures, same run: market_values (8 markets) {mv:.1f} us, slate_values (38x10) {sv:.1f} us: "
                     f"ratio {sv / mv:.2f}")
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(args.out, "slate_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(args.out, "slate_bench.txt"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
