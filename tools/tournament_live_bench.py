"""simulate_tournament on the last group matchday on one MI355X (csrc/dc_tournament_live.hip.h) next to the kick-off
simulator at the same size, the 48-team World Cup format (tests/tournament_ref.py world_cup_48: 12 groups of 4, the 8
best thirds, a 32-team bracket) over 1000 posterior draws:

    live    N simulations of the 48 group fixtures still to kick off + the last matchday's 24 matches in play, the
            draws re-weighted by the 24 states and resampled: live_cup_loglik, live_weights and the mode's dctl kernel;
    plain   N simulations of the same 72 fixtures from kick-off: the mode's dct kernel, the live kernel's twin.

    python tools/tournament_live_bench.py [--out DIR] [--reps N] [--runs N] [--sims N] [--parent-lib NAME]

Per mode ({overall, head_to_head} x {redraw, extra_time}): the kernel time of the live kernel against its twin from
the SAME `rocprofv3 --kernel-trace --stats` run (one child process per run plays every mode both ways), the two weight
kernels, and the wall time of the device call and of the public method end to end (profiler off); and the numpy
restatement's time at 1000 simulations.  Everything is measured --runs times (default 3): medians, with the smallest
and the largest run beside them.  Writes tournament_live_bench.json and tournament_live_bench.txt under --out
(default: profiles/tournament_live).

--parent-lib NAME (a library built from the parent commit, as a file name under bpl-next_amd/bpl/): the DEFAULT path as
well, section 42's way -- the eight kick-off kernels without the keywords, the parent's library against this one in the
same session, alternating, --runs runs each; each median must lie inside the parent's own range of runs or within 1 %
of its median.  Writes default_path.txt."""
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

MODES = {"overall-redraw": ("overall", "redraw"), "h2h-redraw": ("head_to_head", "redraw"),
         "overall-extra_time": ("overall", "extra_time"), "h2h-extra_time": ("head_to_head", "extra_time")}
# (live kernel, twin) as rocprofv3 names them, per mode and with / without an allocation table
LIVE = {"redraw": "live_cup", "extra_time": "live_cup_et"}
TWIN = {"redraw": "dc_tournament", "extra_time": "dc_tournament_et"}
TABLE_TWIN = {"redraw": "cup_alloc", "extra_time": "cup_alloc_et"}
WEIGHT_KERNELS = ("live_cup_loglik", "live_weights")
# the last matchday of a group (a, b, c, d): a v d and b v c; (goals, goals, elapsed) cycled over the 24 matches
STATES = ((0, 0, 0.0), (1, 0, 0.66), (0, 1, 0.35), (1, 1, 0.5), (2, 0, 0.5), (0, 0, 0.6), (2, 1, 0.7), (0, 2, 0.8))


def form(name, tiebreak):
    return f"{name}<{'true' if tiebreak == 'head_to_head' else 'false'}>"


def matchday(kw):
    """(the 48 fixtures still to kick off, the 24 matches in play as `in_play`, all 72 in that order)."""
    rest, last = [], []
    for members in kw["groups"].values():
        a, b, c, d = members
        rest += [(a, b), (a, c), (b, d), (c, d)]
        last += [(a, d), (b, c)]
    st = [STATES[i % len(STATES)] for i in range(len(last))]
    ip = {"home_team": [p for p, _ in last], "away_team": [q for _, q in last], "home_goals": [s[0] for s in st],
          "away_goals": [s[1] for s in st], "elapsed": [s[2] for s in st]}
    return rest, ip, rest + last


def table(kw):
    from bpl import allocation

    names = list(kw["groups"])
    return allocation.from_constraints(kw["groups"], [[g for i, g in enumerate(names) if i != k] for k in range(8)])


def calls(n_sims, mode_id, allocated=False):
    """{"live": (device call, public method), "plain": (...)} of a mode, aggregates only; and the checked inputs."""
    tiebreak, rule = MODES[mode_id]
    m, kw = world_cup()
    rest, ip, every = matchday(kw)
    alloc = table(kw) if allocated else None
    head = (kw["knockout"], kw["groups"], kw["advance"], kw["best_of_rest"])
    tail = (None, None, (3, 1, 0), n_sims, SEED, None, tiebreak, None, rule, None, 1 / 3, None, False, alloc)
    inp, live = m._tournament_call(*head, rest, *tail, ip, None, True)
    _, plain = m._tournament_call(*head, every, *tail)
    dev = m._device()
    public = dict(kw, num_simulations=n_sims, random_state=SEED, tiebreak=tiebreak, knockout_rule=rule)
    if allocated:
        public["best_allocation"] = alloc
    return {"live": (lambda: dev.simulate_tournament_live(*live["args"], **live["kwargs"]),
                     lambda: m.simulate_tournament(group_fixtures=rest, in_play=ip, **public)),
            "plain": (lambda: dev.simulate_tournament(*plain["args"], **plain["kwargs"]),
                      lambda: m.simulate_tournament(group_fixtures=every, **public))}, (m, inp, live)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def restatement_seconds(n_sims=1000):
    import tournament_live_ref as TLR
    import tournament_ref as TR
    from bpl._ffi import prng_key

    _, (m, inp, _) = calls(n_sims, "overall-redraw")
    t0 = time.perf_counter()
    TLR.simulate_tournament_live(TR.model_tables(m), inp, prng_key(SEED), inp["in_play"])
    return time.perf_counter() - t0


def profiled(child_args, names, reps):
    """{kernel: mean us per launch} of the kernels `names`, from one rocprofv3 --kernel-trace --stats run of this
    file as a child process."""
    d = tempfile.mkdtemp(prefix="cup_live_rocprof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--reps", str(reps)] + child_args
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
        if r.returncode != 0:
            raise RuntimeError(f"the rocprofv3 run exited {r.returncode}: {r.stderr[-2000:]}")
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    for k in names:
                        if k + "(" in row["Name"] or (("<" not in k) and k in row["Name"]):
                            out[k] = float(row["TotalDurationNs"]) / 1e3 / int(row["Calls"])   # one launch per call
        if set(out) != set(names):
            found = [os.path.relpath(p, d) for p in glob.glob(os.path.join(d, "**", "*"), recursive=True)]
            raise RuntimeError(f"the rocprofv3 stats hold {sorted(out)}, not {sorted(names)}; files {found}; the child "
                               f"wrote {r.stdout[-1500:]!r} and {r.stderr[-1500:]!r}")
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def spread(values):
    return {"median": float(np.median(values)), "min": float(np.min(values)), "max": float(np.max(values))}


def fmt(v):
    return f"{v['median']:8.1f} ({v['min']:.1f} .. {v['max']:.1f})"


def default_path(args, out_dir):
    """The eight kick-off kernels without the keywords: the parent's library against this one, alternating."""
    names = [form(k[rule], tb) for k in (TWIN, TABLE_TWIN) for tb, rule in MODES.values()]
    runs = {"parent": [], "new": []}
    for _ in range(args.runs):
        runs["parent"].append(profiled(["--child", "default", "--sims", str(args.sims), "--lib", args.parent_lib], names,
                                       args.reps))
        runs["new"].append(profiled(["--child", "default", "--sims", str(args.sims)], names, args.reps))
    lines = [f"Default path (no in_play, no log_weights): kernel time per call in us at the World Cup shape ({args.sims} "
             f"simulations, 48 teams, {S} draws), the parent commit's library against this commit's, both timed in one "
             f"session, alternating; median of {args.runs} runs (smallest .. largest), each run {args.reps} calls after a "
             "warm-up under rocprofv3 --kernel-trace --stats.",
             "Rule: the new median lies inside the parent's smallest-to-largest range, or within 1 % of the parent's "
             "median."]
    ok = True
    for k in names:
        p, q = spread([r[k] for r in runs["parent"]]), spread([r[k] for r in runs["new"]])
        inside = p["min"] <= q["median"] <= p["max"] or abs(q["median"] / p["median"] - 1.0) <= 0.01
        ok = ok and inside
        lines.append(f"{k:28s} parent {fmt(p)}  new {fmt(q)}  new/parent {q['median'] / p['median']:.4f}  "
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
        todo = [calls(args.sims, mode_id, allocated)[0]["plain"][0] for mode_id in MODES for allocated in (False, True)]
    else:
        todo = [fn[0] for mode_id in MODES for fn in calls(args.sims, mode_id)[0].values()]
    for fn in todo:
        for _ in range(args.reps + 1):
            fn()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tournament_live"))
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
    # every mode's live kernel and twin in one run; the weight kernels run once per live call, in every mode
    names = [form(k[rule], tb) for k in (LIVE, TWIN) for tb, rule in MODES.values()] + list(WEIGHT_KERNELS)
    kernel_runs = [profiled(["--child", "live", "--sims", str(N)], names, args.reps) for _ in range(args.runs)]
    res = {"simulations": N, "draws": S, "teams": 48, "fixtures": 48, "in_play": 24, "runs": args.runs, "modes": {}}
    lines = [f"{N} simulations, {S} draws, 48 teams (12 groups of 4, the 8 best thirds, a bracket of 32): 48 fixtures + 24 "
             f"in play v 72 fixtures from kick-off; medians of {args.runs} runs (smallest .. largest)"]
    for mode_id, (tb, rule) in MODES.items():
        live_k, twin_k = form(LIVE[rule], tb), form(TWIN[rule], tb)
        todo, _ = calls(N, mode_id)
        wall = {kind: {"device_call_ms": spread([timed(pair[0], args.reps) for _ in range(args.runs)]),
                       "end_to_end_ms": spread([timed(pair[1], args.reps) for _ in range(args.runs)])}
                for kind, pair in todo.items()}
        kern = {"live_us": spread([r[live_k] for r in kernel_runs]), "twin_us": spread([r[twin_k] for r in kernel_runs]),
                "ratio": spread([r[live_k] / r[twin_k] for r in kernel_runs])}
        res["modes"][mode_id] = {"kernel": kern, "wall": wall}
        lines.append(f"{mode_id}: {live_k} {fmt(kern['live_us'])} us per call, {twin_k} {fmt(kern['twin_us'])} us: "
                     f"x {kern['ratio']['median']:.3f} ({kern['ratio']['min']:.3f} .. {kern['ratio']['max']:.3f})")
        for kind in ("live", "plain"):
            w = wall[kind]
            lines.append(f"    {kind}: device call {w['device_call_ms']['median']:.3f} ms "
                         f"({w['device_call_ms']['min']:.3f} .. {w['device_call_ms']['max']:.3f}), public method end to end "
                         f"{w['end_to_end_ms']['median']:.3f} ms ({w['end_to_end_ms']['min']:.3f} .. "
                         f"{w['end_to_end_ms']['max']:.3f})")
    res["weight_kernels_us"] = {k: spread([r[k] for r in kernel_runs]) for k in WEIGHT_KERNELS}
    lines.append("  " + ", ".join(f"{k} {fmt(v)} us per call" for k, v in res["weight_kernels_us"].items()))
    res["restatement_seconds_at_1000_simulations"] = ref_s = restatement_seconds()
    lines.append(f"  the numpy restatement at 1000 simulations: {ref_s:.2f} s")
    lines.append("  beside it: the season's live simulator costs x 1.14 over dc_season (profiles/live/); no ratio is a gate")
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(args.out, "tournament_live_bench.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.join(args.out, "tournament_live_bench.txt"), "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
