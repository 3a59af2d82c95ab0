"""What a `best_allocation` costs on one MI355X at the World Cup case: N = 100 000 simulations of 48 teams (12 groups
of 4, 72 group fixtures, the 8 best thirds, a 32-team bracket) over 1000 posterior draws, with a 495-row table from
`bpl.allocation.from_constraints` ("slot k never takes the third of group k") and without one, in both tie-break
modes and under either knockout rule.

    python tools/allocation_bench.py [--out DIR] [--reps N] [--runs N] [--sims N] [--knockout-rule RULE]

Reports, per mode: the kernel time of `dc_tournament` and of the three recording kernels `dc_paths_sim`,
`dc_tscen_sim` and `dc_gpts_sim` (summed over the chunks of a call) without the table, and of their allocation twins
`cup_alloc`, `paths_alloc_sim`, `scen_alloc_sim` and `points_alloc_sim` with it, from `rocprofv3 --kernel-trace
--stats` runs of their own (child processes, one per setting, run one after the other in every run), and the ratio
with / without of every run.
Everything is measured --runs times (default 3): the figures are the medians over the runs, with the smallest and
largest run beside them.  Writes allocation_bench.json and allocation_bench.txt under --out (default:
profiles/allocation)."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "bpl-next_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402

from paths_bench import S, SEED, world_cup  # noqa: E402

KERNELS = ("dc_tournament", "dc_paths_sim", "dc_tscen_sim", "dc_gpts_sim")
TWINS = {"dc_tournament": "cup_alloc", "dc_paths_sim": "paths_alloc_sim", "dc_tscen_sim": "scen_alloc_sim",
         "dc_gpts_sim": "points_alloc_sim"}   # the kernels that run under a table, reported under their twins' names
MODES = ("overall", "head_to_head")
GD_CAP = 3


def table(kw):
    """The 495-row table of the case: slot k may take the third of every group but the k-th."""
    from bpl import allocation

    names = list(kw["groups"])
    return allocation.from_constraints(kw["groups"], [[g for i, g in enumerate(names) if i != k] for k in range(8)])


def calls(n_sims, tiebreak, rule, allocated):
    """The four device calls at the case's shape, under the table or without one."""
    from bpl.base import points_axis

    m, kw = world_cup()
    inp, call = m._tournament_call(kw["knockout"], kw["groups"], kw["advance"], kw["best_of_rest"], None, None, None,
                                   (3, 1, 0), n_sims, SEED, None, tiebreak, None, rule, None, 1 / 3, None, False,
                                   table(kw) if allocated else None)
    assert ("allocation" in call["kwargs"]) == bool(allocated)
    pmin, bins = points_axis(inp["table"][:, 0], inp["fix_p"], inp["fix_q"], inp["points"])
    dev = m._device()
    return (lambda: dev.simulate_tournament(*call["args"], **call["kwargs"]),
            lambda: dev.tournament_paths(*call["args"], **call["kwargs"]),
            lambda: dev.tournament_scenarios(*call["args"], key_fixture=[2, 3], key_cap=[3, 3], **call["kwargs"]),
            lambda: dev.tournament_points(*call["args"], points_min=pmin, n_bins=bins, gd_cap=GD_CAP, **call["kwargs"]))


def kernel_times(n_sims, reps, tiebreak, rule, allocated):
    """Per device call: the summed duration of each kernel's launches (the recording kernels run once per chunk)."""
    d = tempfile.mkdtemp(prefix="alloc_rocprof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--child", tiebreak, "--table", str(int(allocated)),
           "--sims", str(n_sims), "--reps", str(reps), "--knockout-rule", rule]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
        if r.returncode != 0:
            raise RuntimeError(f"the rocprofv3 run exited {r.returncode}: {r.stderr[-2000:]}")
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    for k in KERNELS:
                        if (TWINS[k] if allocated else k) in row["Name"]:
                            out[k] = float(row["TotalDurationNs"]) / 1e3 / (reps + 1)
        if set(out) != set(KERNELS):
            raise RuntimeError(f"the rocprofv3 stats hold {sorted(out)}, not {KERNELS}")
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def spread(values):
    v = [float(x) for x in values]
    return {"median": float(np.median(v)), "min": min(v), "max": max(v), "runs": v}


def fmt(s, unit="", digits=1):
    return f"{s['median']:.{digits}f}{unit} ({s['min']:.{digits}f} .. {s['max']:.{digits}f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "allocation"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sims", type=int, default=100_000)
    ap.add_argument("--knockout-rule", default="redraw", choices=("redraw", "extra_time"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--table", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    N, rule = args.sims, args.knockout_rule
    if args.child:
        device_calls = calls(N, args.child, rule, args.table)
        for _ in range(args.reps + 1):
            for fn in device_calls:
                fn()
        return
    os.makedirs(args.out, exist_ok=True)
    res = {"simulations": N, "draws": S, "teams": 48, "table_rows": 495, "knockout_rule": rule, "runs": args.runs,
           "reps": args.reps, "modes": {}}
    lines = []
    for tiebreak in MODES:
        runs = [(kernel_times(N, args.reps, tiebreak, rule, False), kernel_times(N, args.reps, tiebreak, rule, True))
                for _ in range(args.runs)]
        without = {k: spread([a[k] for a, _ in runs]) for k in KERNELS}
        with_table = {k: spread([b[k] for _, b in runs]) for k in KERNELS}
        ratio = {k: spread([b[k] / a[k] for a, b in runs]) for k in KERNELS}
        res["modes"][tiebreak] = {"without_us_per_call": without, "with_table_us_per_call": with_table,
                                  "with_over_without": ratio}
        lines.append(f"{tiebreak}:")
        lines += [f"  {k}: without {fmt(without[k], ' us')}, with the table {fmt(with_table[k], ' us')} per call; "
                  f"with / without = {fmt(ratio[k], '', 4)}" for k in KERNELS]
    head = (f"World Cup: {N} simulations x 48 teams x 72 group fixtures x 5 rounds ({rule}), {S} draws, a 495-row table; "
            f"medians over {args.runs} runs (smallest .. largest run), each run {args.reps} calls after a warm-up")
    text = "\n".join([head] + lines)
    print(text)
    suffix = "" if rule == "redraw" else "_" + rule
    with open(os.path.join(args.out, f"allocation_bench{suffix}.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.join(args.out, f"allocation_bench{suffix}.txt"), "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
