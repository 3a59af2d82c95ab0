"""tournament_paths, tournament_scenarios and tournament_points on the last group matchday on one MI355X
(csrc/dc_tournament_live_queries.hip.h) next to the same queries from kick-off at the same size, the 48-team World Cup
format (tests/tournament_ref.py world_cup_48: 12 groups of 4, the 8 best thirds, a 32-team bracket) over 1000 posterior
draws:

    live    N simulations of the 48 group fixtures still to kick off + the last matchday's 24 matches in play, the
            draws re-weighted by the 24 states and resampled: live_cup_loglik, live_weights and the query's dctq kernel;
    plain   N simulations of the same 72 fixtures from kick-off: the query's kick-off recording kernel, its twin.

    python tools/tournament_live_queries_bench.py [--out DIR] [--reps N] [--runs N] [--sims N] [--parent-lib NAME]

Per query and mode ({overall, head_to_head} x {redraw, extra_time}): the kernel time per device call of the live
recording kernel against its twin from the SAME `rocprofv3 --kernel-trace --stats` run (one child process per run plays
every query and mode both ways; a recording kernel runs once per chunk of the workspace, its launches are summed), the
two weight kernels, the wall time of the device call and of the public method end to end (profiler off), and the numpy
route: the live simulate_tournament(return_stages=True) and the cross-tabulation of its records that stands in for
the query (the in-play outcomes against the targets; it has no opponents, group places, key classes of the ordinary
fixtures or points per simulation).  Everything is measured --runs times (default 3): medians, with the smallest and
the largest run beside them.  Writes tournament_live_queries_bench.json and .txt under --out (default:
profiles/tournament_live_queries).

--parent-lib NAME (a library built from the parent commit, as a file name under bpl-next_amd/bpl/): the DEFAULT path as
well -- the 24 kick-off recording kernels without the keywords, the parent's library against this one in the same
session, alternating, --runs runs each; each median must lie inside the parent's own range of runs or within 1 % of
its median.  Writes default_path.txt."""
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

from paths_bench import S, SEED, world_cup  # noqa: E402
from tournament_live_bench import MODES, WEIGHT_KERNELS, fmt, matchday, spread, table, timed  # noqa: E402

QUERIES = ("paths", "scenarios", "points")
# (live kernel, twin, the twin under an allocation table) as rocprofv3 names them
LIVE = {"paths": "cup_paths_live", "scenarios": "cup_scen_live", "points": "cup_gpoints_live"}
TWIN = {"paths": "dc_paths_sim", "scenarios": "dc_tscen_sim", "points": "dc_gpts_sim"}
TABLE_TWIN = {"paths": "paths_alloc_sim", "scenarios": "scen_alloc_sim", "points": "points_alloc_sim"}
# the scenario keys: the two matches in play of the first group, by one goal or more / by two or more
KEYS, CAPS = (48, 49), (1, 2)


def form(name, tiebreak, rule):
    return f"{name}<{'true' if tiebreak == 'head_to_head' else 'false'}, {'true' if rule == 'extra_time' else 'false'}>"


def calls(n_sims, query, mode_id, allocated=False):
    """{"live": (device call, public method), "plain": (...)} of a query in a mode, tables only."""
    from bpl.base import points_axis

    tiebreak, rule = MODES[mode_id]
    m, kw = world_cup()
    rest, ip, every = matchday(kw)
    alloc = table(kw) if allocated else None
    head = (kw["knockout"], kw["groups"], kw["advance"], kw["best_of_rest"])
    tail = (None, None, (3, 1, 0), n_sims, SEED, None, tiebreak, None, rule, None, 1 / 3, None, False, alloc)
    _, live = m._tournament_call(*head, rest, *tail, ip, None, True)
    inp, plain = m._tournament_call(*head, every, *tail)
    dev = m._device()
    public = dict(kw, num_simulations=n_sims, random_state=SEED, tiebreak=tiebreak, knockout_rule=rule)
    if allocated:
        public["best_allocation"] = alloc
    extra, more = {}, {}
    if query == "scenarios":
        extra, more = {"key_fixture": KEYS, "key_cap": CAPS}, {"fixtures": KEYS, "margin_cap": CAPS}
    if query == "points":
        points_min, n_bins = points_axis(inp["table"][:, 0], inp["fix_p"], inp["fix_q"], inp["points"])
        extra = {"points_min": points_min, "n_bins": n_bins, "gd_cap": 3}
    device, method = getattr(dev, f"tournament_{query}"), getattr(m, f"tournament_{query}")
    device_live = getattr(dev, f"tournament_{query}_live")
    return {"live": (lambda: device_live(*live["args"], **extra, **live["kwargs"]),
                     lambda: method(group_fixtures=rest, in_play=ip, **more, **public)),
            "plain": (lambda: device(*plain["args"], **extra, **plain["kwargs"]),
                      lambda: method(group_fixtures=every, **more, **public))}


def numpy_route(n_sims):
    """Seconds of the route without the live queries: the live simulate_tournament with its records, and the in-play
    outcomes cross-tabulated against the targets on the host."""
    m, kw = world_cup()
    rest, ip, _ = matchday(kw)
    t0 = time.perf_counter()
    res = m.simulate_tournament(group_fixtures=rest, in_play=ip, num_simulations=n_sims, random_state=SEED,
                                return_stages=True, **kw)
    margin = res["in_play_home_goals"].astype(np.int64) - res["in_play_away_goals"].astype(np.int64)
    rounds = res["round_proba"].shape[1]
    reach = (res["stage"][:, :, None] >= np.arange(1, rounds + 1)[None, None, :]).reshape(n_sims, -1)
    onehot = ((1 - np.sign(margin))[:, :, None] == np.arange(3)[None, None, :]).reshape(n_sims, -1)
    joint = onehot.astype(np.float32).T @ reach.astype(np.float32)   # (0 / 1 products: exact below 2^24)
    assert joint.sum() > 0
    return time.perf_counter() - t0


def profiled(child_args, names, reps):
    """{kernel: (total us, launches)} of the kernels `names`, from one rocprofv3 --kernel-trace --stats run of this file
    as a child process."""
    d = tempfile.mkdtemp(prefix="cup_live_queries_rocprof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--reps", str(reps)] + child_args
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=540)
        if r.returncode != 0:
            raise RuntimeError(f"the rocprofv3 run exited {r.returncode}: {r.stderr[-2000:]}")
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    for k in names:
                        if k + "(" in row["Name"] or (("<" not in k) and k in row["Name"]):
                            out[k] = (float(row["TotalDurationNs"]) / 1e3, int(row["Calls"]))
        if set(out) != set(names):
            found = [os.path.relpath(p, d) for p in glob.glob(os.path.join(d, "**", "*"), recursive=True)]
            raise RuntimeError(f"the rocprofv3 stats hold {sorted(out)}, not {sorted(names)}; files {found}; the child "
                               f"wrote {r.stdout[-1500:]!r} and {r.stderr[-1500:]!r}")
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def default_path(args, out_dir):
    """The 24 kick-off recording kernels without the keywords: the parent's library against this one, alternating."""
    names = [form(k[q], tb, rule) for q in QUERIES for k in (TWIN, TABLE_TWIN) for tb, rule in MODES.values()]
    runs = {"parent": [], "new": []}
    for _ in range(args.runs):
        for which, lib in (("parent", ["--lib", args.parent_lib]), ("new", [])):
            run = profiled(["--child", "default", "--sims", str(args.sims)] + lib, names, args.reps)
            runs[which].append({k: total / launches for k, (total, launches) in run.items()})
    lines = [f"Default path (no in_play, no log_weights): kernel time per launch in us at the World Cup shape ({args.sims} "
             f"simulations, 48 teams, {S} draws, 72 group fixtures), the parent commit's library against this commit's, "
             f"both timed in one session, alternating; median of {args.runs} runs (smallest .. largest), each run "
             f"{args.reps} calls after a warm-up under rocprofv3 --kernel-trace --stats.",
             "Rule: the new median lies inside the parent's smallest-to-largest range, or within 1 % of the parent's "
             "median."]
    ok = True
    for k in names:
        p, q = spread([r[k] for r in runs["parent"]]), spread([r[k] for r in runs["new"]])
        inside = p["min"] <= q["median"] <= p["max"] or abs(q["median"] / p["median"] - 1.0) <= 0.01
        ok = ok and inside
        lines.append(f"{k:36s} parent {fmt(p)}  new {fmt(q)}  new/parent {q['median'] / p['median']:.4f}  "
                     f"rule: {'inside' if inside else 'OUTSIDE'}")
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(out_dir, "default_path.txt"), "w") as fh:
        fh.write(text + "\n")
    return ok


def child(args):
    if args.lib:
        import ctypes

        import torch  # noqa: F401  (before the library, as HipContext loads them: torch's HIP runtime comes first)

        from bpl import _ffi

        _ffi._LIB_NAME = args.lib   # (an older build: the symbols it does not have are not bound)
        have = ctypes.CDLL(_ffi.lib_path())
        for name in [n for n in _ffi._SIGNATURES if not hasattr(have, n)]:
            del _ffi._SIGNATURES[name]
    if args.child == "default":
        todo = [calls(args.sims, q, mode_id, allocated)["plain"][0] for q in QUERIES for mode_id in MODES
                for allocated in (False, True)]
    else:
        todo = [fn[0] for q in QUERIES for mode_id in MODES for fn in calls(args.sims, q, mode_id).values()]
    for fn in todo:
        for _ in range(args.reps + 1):
            fn()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tournament_live_queries"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sims", type=int, default=100_000)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only-default", action="store_true", help="the default-path comparison alone")
    ap.add_argument("--child", choices=("live", "default"), help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    os.makedirs(args.out, exist_ok=True)
    if args.parent_lib and not default_path(args, args.out):
        sys.exit("the default path moved: see default_path.txt")
    if args.only_default:
        return
    N = args.sims
    names = [form(k[q], tb, rule) for q in QUERIES for k in (LIVE, TWIN) for tb, rule in MODES.values()]
    names += list(WEIGHT_KERNELS)
    kernel_runs = [{k: total for k, (total, _) in profiled(["--child", "live", "--sims", str(N)], names, args.reps).items()}
                   for _ in range(args.runs)]
    # (the totals of a run over its reps + 1 calls of every form; the weight kernels run in every live call)
    calls_per_form = args.reps + 1
    res = {"simulations": N, "draws": S, "teams": 48, "fixtures": 48, "in_play": 24, "runs": args.runs, "queries": {}}
    lines = [f"{N} simulations, {S} draws, 48 teams (12 groups of 4, the 8 best thirds, a bracket of 32): 48 fixtures + 24 "
             f"in play v 72 fixtures from kick-off; kernel time per device call (the launches of all chunks summed); "
             f"medians of {args.runs} runs (smallest .. largest)"]
    for q in QUERIES:
        res["queries"][q] = {}
        for mode_id, (tb, rule) in MODES.items():
            live_k, twin_k = form(LIVE[q], tb, rule), form(TWIN[q], tb, rule)
            todo = calls(N, q, mode_id)
            wall = {kind: {"device_call_ms": spread([timed(pair[0], args.reps) for _ in range(args.runs)]),
                           "end_to_end_ms": spread([timed(pair[1], args.reps) for _ in range(args.runs)])}
                    for kind, pair in todo.items()}
            kern = {"live_us": spread([r[live_k] / calls_per_form for r in kernel_runs]),
                    "twin_us": spread([r[twin_k] / calls_per_form for r in kernel_runs]),
                    "ratio": spread([r[live_k] / r[twin_k] for r in kernel_runs])}
            res["queries"][q][mode_id] = {"kernel": kern, "wall": wall}
            lines.append(f"{q} {mode_id}: {live_k} {fmt(kern['live_us'])} us per call, {twin_k} {fmt(kern['twin_us'])} us: "
                         f"x {kern['ratio']['median']:.3f} ({kern['ratio']['min']:.3f} .. {kern['ratio']['max']:.3f})")
            for kind in ("live", "plain"):
                w = wall[kind]
                lines.append(f"    {kind}: device call {w['device_call_ms']['median']:.3f} ms "
                             f"({w['device_call_ms']['min']:.3f} .. {w['device_call_ms']['max']:.3f}), public method end to "
                             f"end {w['end_to_end_ms']['median']:.3f} ms ({w['end_to_end_ms']['min']:.3f} .. "
                             f"{w['end_to_end_ms']['max']:.3f})")
    live_calls = calls_per_form * len(QUERIES) * len(MODES)
    res["weight_kernels_us"] = {k: spread([r[k] / live_calls for r in kernel_runs]) for k in WEIGHT_KERNELS}
    lines.append("  " + ", ".join(f"{k} {fmt(v)} us per call" for k, v in res["weight_kernels_us"].items()))
    res["numpy_route_seconds"] = route = spread([numpy_route(N) for _ in range(args.runs)])
    lines.append(f"  the numpy route (live simulate_tournament(return_stages=True) and the in-play outcomes cross-tabulated "
                 f"against the targets on the host): {route['median']:.3f} s ({route['min']:.3f} .. {route['max']:.3f})")
    lines.append("  beside it: the live simulator costs x 1.03 .. 1.14 over its twin (profiles/tournament_live/), the "
                 "season's live queries x 1.10 .. 1.11 (profiles/live_queries/); no ratio is a gate")
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(args.out, "tournament_live_queries_bench.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.join(args.out, "tournament_live_queries_bench.txt"), "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
