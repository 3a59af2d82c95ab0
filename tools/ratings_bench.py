"""team_ratings on one MI355X (csrc/dc_ratings.hip.h) at two shapes, max_goals = 15, all five statistics:

    league      20 teams x 1 000 draws, venue "both" (380 ordered pairs), basic model
    world_cup   211 teams x 4 000 draws on neutral ground (44 310 matches), World-Cup model with confederations

    python tools/ratings_bench.py [--out DIR] [--reps N]

Reports per shape: the kernel times of the three launches `ratings_values`, `market_summary` and `ratings_rank`
(summed over the chunks of a call) from a `rocprofv3 --kernel-trace --stats` run of its own (a child process;
profiler off for the wall times); the counted float64 work of `ratings_values`, R x matches x S walks of
dcs::outcome_probs at depth G with 9 float64 vector instructions per depth (4 multiplications, 3 fma, 2 additions;
the exp calls are not counted), and the share of the float64 vector rate (78.6 TFLOP/s = 39.3e12 fma lanes per
second; a multiplication or an addition issues like an fma) that count over the `ratings_values` time comes to;
the end-to-end wall time of the device call (HipContext.team_ratings: H2D + kernels + D2H, median of N after a
warm-up that also builds the team-major copies) and of the public `team_ratings()`.  At the league shape also
the numpy restatement (tests/ratings_ref.py) with the largest difference of the means and quantiles, and the
only route without this feature: `predict_markets(return_draws=True)` over the 380 ordered pairs with the five
markets that carry the statistics, plus the numpy reduction over the field and the ranks.  Writes
ratings_bench.json and ratings_bench.txt under --out (default: profiles/ratings)."""
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
sys.path[:0] = [os.path.join(ROOT, "bpl-next_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"),
                os.path.join(ROOT, "oracle")]   # (tests/fake_ctx.py, behind the restatement, imports the oracle)

import numpy as np  # noqa: E402

G = 15
QS = (0.05, 0.5, 0.95)
KERNELS = ("ratings_values", "market_summary", "ratings_rank")
FMA_LANES_PER_S = 39.3e12   # float64 vector rate of one MI355X (78.6 TFLOP/s)
WALK_INSTRUCTIONS_PER_DEPTH = 9
CASES = {"league": ("basic", 20, 1000, "both"), "world_cup": ("wc", 211, 4000, "neutral")}


def case(name):
    """(model, keyword arguments of team_ratings)."""
    import loglik_ref as LR
    import ratings_ref as RR

    kind, T, S, venue = CASES[name]
    m = LR.hand_model(kind, S=S, T=T, seed=5, C=6)
    kw = {"venue": venue, "max_goals": G, "quantiles": QS}
    if kind == "wc":
        kw["team_conf"] = RR.conf_of(m)
    return m, kw


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
    """(model, keyword arguments, the device call of the shape as a function)."""
    m, kw = case(name)
    T = len(m.teams)
    idx = np.arange(T, dtype=np.uint16)
    conf = {}
    if "team_conf" in kw:
        cf = m._tournament_conf(kw["team_conf"], [str(t) for t in m.teams])
        conf = {"team_conf": cf, "opponent_conf": cf}
    dev = m._device()
    venue = ("both", "home", "away", "neutral").index(kw["venue"])
    return m, kw, lambda: dev.team_ratings(idx, idx, venue, G, (3, 1, 0), 0, QS, **conf)


def kernel_times(name, reps):
    """Per device call: the summed duration of each kernel's launches."""
    d = tempfile.mkdtemp(prefix="ratings_rocprof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(reps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
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


def markets_route(m, points=(3, 1, 0)):
    """The route without team_ratings: per-draw markets of every ordered pair on the host, then numpy."""
    from bpl import markets as MK

    names = [str(t) for t in m.teams]
    T = len(names)
    pairs = [(h, a) for h in range(T) for a in range(T) if h != a]
    d = {"home_team": [names[h] for h, _ in pairs], "away_team": [names[a] for _, a in pairs]}
    mk = {"home_win": MK.home_win(), "draw": MK.draw(), "away_win": MK.away_win(), "goals_home": MK.goals("home"),
          "goals_away": MK.goals("away")}
    v = m.predict_markets(d, mk, max_goals=G, quantiles=(), return_draws=True)["draws"]   # [S, 5, pairs]
    h = np.array([p[0] for p in pairs])
    a = np.array([p[1] for p in pairs])
    S = v.shape[0]
    out = np.zeros((S, 5, T))
    W, D, L = points
    for side, win, loss, gf, ga in ((h, 0, 2, 3, 4), (a, 2, 0, 4, 3)):
        np.add.at(out[:, 0, :], (slice(None), side), W * v[:, win] + D * v[:, 1] + L * v[:, loss])
        np.add.at(out[:, 1, :], (slice(None), side), v[:, win])
        np.add.at(out[:, 2, :], (slice(None), side), v[:, gf])
        np.add.at(out[:, 3, :], (slice(None), side), v[:, ga])
    out[:, 4, :] = out[:, 2, :] - out[:, 3, :]
    out /= 2 * (T - 1)
    order = np.argsort(-out[:, 0, :], axis=1, kind="stable")
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.arange(T)[None, :], axis=1)
    count = np.stack([(rank == r).sum(axis=0) for r in range(T)], axis=1)
    return {"mean": out.mean(axis=0), "quantile": np.quantile(out, QS, axis=0).transpose(1, 0, 2), "rank_count": count}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ratings"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        call = device_call(args.child)[2]
        for _ in range(args.reps + 1):
            call()
        return
    import ratings_ref as RR

    os.makedirs(args.out, exist_ok=True)
    res, lines = {}, []
    for name, (kind, T, S, venue) in CASES.items():
        m, kw, call = device_call(name)
        wall = {"device_call": timed(call, args.reps), "team_ratings": timed(lambda: m.team_ratings(**kw), args.reps)}
        kern = kernel_times(name, args.reps)
        got = m.team_ratings(**kw)
        matches = int(got["matches"].sum())
        ops = WALK_INSTRUCTIONS_PER_DEPTH * G * matches * S
        t_values = kern["ratings_values"]["us_per_call"] * 1e-6
        share = ops / FMA_LANES_PER_S / t_values
        res[name] = {"model": kind, "teams": T, "draws": S, "venue": venue, "matches": matches, "max_goals": G,
                     "quantiles": list(QS), "wall": wall, "kernel": kern, "float64_walk_instructions": ops,
                     "float64_valu_share_of_ratings_values": share}
        best = int(np.argmin(got["expected_rank"]))
        lines += [
            f"{name}: {T} teams x {S} draws, venue {venue} ({matches} matches), {kind} model, max_goals = {G}",
            "  " + ", ".join(f"{k} {kern[k]['us_per_call']:.1f} us" for k in KERNELS) + " per call",
            f"  counted float64 work 9 G x matches x S = {ops:.3e} lane instructions: {ops / t_values / 1e12:.2f} T/s in "
            f"ratings_values = {100 * share:.1f} % of the float64 vector rate ({FMA_LANES_PER_S / 1e12:.1f}e12 fma lanes/s)",
            f"  device call {wall['device_call']['median_ms']:.3f} ms end to end, team_ratings() "
            f"{wall['team_ratings']['median_ms']:.3f} ms (medians of {args.reps})",
            f"  best team {got['teams'][best]}: {got['mean'][0, best]:.3f} points a match, 5 % / median / 95 % "
            + " / ".join(f"{v:.3f}" for v in got["quantile"][0, :, best])
            + f", P(rank 0) = {got['rank_proba'][best, 0]:.3f}"]
        if name == "league":
            t0 = time.perf_counter()
            ref = RR.team_ratings(m, venue=venue, G=G, quantiles=QS)
            ref_s = time.perf_counter() - t0
            diff = max(float(np.abs(ref[key] - got[key]).max()) for key in ("mean", "sd", "quantile"))
            same = bool((ref["rank_count"] == got["rank_count"]).all())
            route = timed(lambda: markets_route(m), args.reps)
            alt = markets_route(m)
            adiff = max(float(np.abs(alt[key][:2] - got[key][:2]).max()) for key in ("mean", "quantile"))   # points, win
            res[name]["numpy"] = {"seconds": ref_s, "max_abs_diff": diff, "rank_counts_equal": same}
            res[name]["predict_markets_route"] = dict(route, max_abs_diff=adiff,
                                                      rank_counts_equal=bool((alt["rank_count"] == got["rank_count"]).all()))
            lines += [
                f"  numpy restatement {ref_s:.2f} s; max |difference| of mean, sd and quantiles {diff:.2e}; rank counts "
                f"{'equal' if same else 'DIFFER'}",
                f"  predict_markets(return_draws=True) over the 380 ordered pairs + numpy reduction {route['median_ms']:.1f} ms "
                f"(median of {args.reps}); max |difference| of the means and quantiles of points and win {adiff:.2e} (its goal markets stop at max_goals)"]
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(args.out, "ratings_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(args.out, "ratings_bench.txt"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
