"""The head-to-head instantiations of the table simulators on one MI355X (csrc/dc_h2h.hip.h), each next to its
overall-order counterpart launched in the same run at the same shape:

    league      N simulations of a 380-fixture double round robin of 20 teams over 1000 posterior draws:
                dc_season<true> v dc_season<false>, and match_leverage with the default targets:
                dc_leverage_sim<true> v dc_leverage_sim<false> (dc_leverage_count is the same kernel in both);
    tournament  N simulations of the 48-team World Cup format (12 groups of 4, top two + the 8 best thirds):
                dc_tournament<true> v dc_tournament<false>.

    python tools/h2h_bench.py [--out DIR] [--reps N] [--sims N]

Reports the kernel times from a `rocprofv3 --kernel-trace --stats` run of its own (a child process; profiler off
for the wall times), the end-to-end wall time of each device call (medians of N after a warm-up) and the ratios
head-to-head / counterpart.  Writes h2h_bench.json and h2h_bench.txt under --out (default: profiles/h2h)."""
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
# (head-to-head kernel, counterpart) as rocprofv3 names them: the two instantiations of one template, neither
# name a part of the other
PAIRS = (("dc_season<true>", "dc_season<false>"), ("dc_leverage_sim<true>", "dc_leverage_sim<false>"),
         ("dc_tournament<true>", "dc_tournament<false>"))
KERNELS = tuple(k for pair in PAIRS for k in pair) + ("dc_leverage_count",)


def which(name):
    """The kernel of KERNELS a rocprofv3 row names, or None."""
    return next((k for k in KERNELS if k in name), None)


def league():
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
    """{name: (head-to-head device call, counterpart's device call)}, aggregates only."""
    import tournament_ref as R
    from bpl import NeutralDixonColesMatchPredictorWC
    from bpl._ffi import prng_key
    from bpl.base import leverage_targets
    from test_tournament_host import conf_of, hand_posterior

    key = prng_key(SEED)
    m, h, a = league()
    hh, aa, table_idx, table, points, n = m._season_inputs(h, a, n_sims, None, None, (3, 1, 0))
    _, masks = leverage_targets(None, table_idx.size)
    dev = m._device()
    wc = hand_posterior(NeutralDixonColesMatchPredictorWC, T=64, S=S, seed=9)
    kw = R.world_cup_48(list(wc.teams))
    inp = wc._tournament_inputs(kw["knockout"], kw["groups"], kw["advance"], kw["best_of_rest"], None, None, None,
                                (3, 1, 0), n_sims, conf_of(wc))
    wdev = wc._device()

    def tournament(**extra):
        return wdev.simulate_tournament(inp["team_idx"], inp["bracket"], n_sims, key, team_conf=inp["conf"],
                                        team_host=inp["host"], team_group=inp["group"], table=inp["table"],
                                        fix_p=inp["fix_p"], fix_q=inp["fix_q"], advance=inp["advance"],
                                        best_of_rest=inp["best_of_rest"], points=inp["points"], **extra)

    return {
        "season": (lambda: dev.simulate_season(hh, aa, table_idx, table, points, n, key, head_to_head=True),
                   lambda: dev.simulate_season(hh, aa, table_idx, table, points, n, key)),
        "leverage": (lambda: dev.match_leverage(hh, aa, table_idx, table, points, n, key, masks, head_to_head=True),
                     lambda: dev.match_leverage(hh, aa, table_idx, table, points, n, key, masks)),
        "tournament": (lambda: tournament(head_to_head=True), tournament),
    }


def kernel_times(n_sims, reps):
    """Per device call: the summed duration of each kernel's launches."""
    d = tempfile.mkdtemp(prefix="h2h_rocprof_")
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
                    k = which(row["Name"])
                    if k:
                        n = int(row["Calls"])
                        # dc_leverage_count runs under both leverage calls of a repetition
                        per = (reps + 1) * (2 if k == "dc_leverage_count" else 1)
                        out[k] = {"launches": n, "launches_per_call": n / per,
                                  "us_per_call": float(row["TotalDurationNs"]) / 1e3 / per}
        if set(out) != set(KERNELS):
            raise RuntimeError(f"the rocprofv3 stats hold {sorted(out)}, not {sorted(KERNELS)}")
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "h2h"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sims", type=int, default=100_000)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    N = args.sims
    todo = calls(N)
    if args.child:
        for _ in range(args.reps + 1):
            for h2h_call, counterpart in todo.values():
                h2h_call()
                counterpart()
        return
    os.makedirs(args.out, exist_ok=True)
    wall = {name: {"head_to_head": timed(pair[0], args.reps), "counterpart": timed(pair[1], args.reps)}
            for name, pair in todo.items()}
    for w in wall.values():
        w["ratio"] = w["head_to_head"]["median_ms"] / w["counterpart"]["median_ms"]
    kern = kernel_times(N, args.reps)
    ratios = {new: kern[new]["us_per_call"] / kern[old]["us_per_call"] for new, old in PAIRS}
    res = {"simulations": N, "draws": S, "league": {"fixtures": T * (T - 1), "teams": T},
           "tournament": "world_cup_48", "wall": wall, "kernel": kern, "kernel_ratio": ratios}
    lines = [f"{N} simulations, {S} draws; league: {T * (T - 1)} fixtures x {T} teams; tournament: 48-team World Cup format"]
    for (new, old), name in zip(PAIRS, ("season", "leverage", "tournament")):
        w = wall[name]
        lines.append(f"  {new} {kern[new]['us_per_call']:.1f} us per call, {old} {kern[old]['us_per_call']:.1f} us: "
                     f"x {ratios[new]:.2f}; device call end to end {w['head_to_head']['median_ms']:.3f} ms v "
                     f"{w['counterpart']['median_ms']:.3f} ms: x {w['ratio']:.2f} (medians of {args.reps})")
    lines.append(f"  dc_leverage_count (both modes) {kern['dc_leverage_count']['us_per_call']:.1f} us per call")
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(args.out, "h2h_bench.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.join(args.out, "h2h_bench.txt"), "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
