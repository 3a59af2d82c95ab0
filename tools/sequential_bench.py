"""sequential_scores on one MI355X at the two cases of tools/loglik_bench.py, S = 4000 draws, max_goals = 15:
the league (20 teams, 380 fixtures, 38 blocks of 10) and the World-Cup form (200 teams, 6 confederations, 40 000
fixtures, 100 blocks of 400), beside the numpy restatement.

    python tools/sequential_bench.py [--out DIR] [--reps N]

Reports per case: the kernel times of block_ll_tiles, block_ll_reduce, psis_rows, weighted_tiles and
weighted_reduce from a `rocprofv3 --kernel-trace --stats` run of its own (a child process; profiler off for the
wall times); the wall time of the three device calls together and of the public `sequential_scores(data, block)`
(medians of N after a warm-up that also builds the team-major copies); and the numpy restatement
(tests/sequential_ref.py: the full log-likelihood matrix, PSIS with a full sort, full grids) on the first
--ref-fixtures fixtures of every block, its time scaled to all of them.  Writes sequential_bench.json and
sequential_bench.txt under --out (default: profiles/sequential).  No time is a pass / fail gate."""
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
BLOCKS = {"league": 38, "world_cup": 100}
KERNELS = ("block_ll_tiles", "block_ll_reduce", "psis_rows", "weighted_tiles", "weighted_reduce")


def blocks_of(name, n):
    """Equal blocks in fixture order, labelled 1..B."""
    return 1 + (np.arange(n) * BLOCKS[name]) // n


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * float(np.min(ts)),
            "max_ms": 1e3 * float(np.max(ts)), "reps": reps}


def device_calls(dev, kw, idx, B):
    from bpl.sequential import log_ratios

    A = dev.block_loglik(**kw, block_idx=idx, n_blocks=B)
    w = dev.psis_weights(log_ratios(A))
    return dev.weighted_scores(**kw, block_idx=idx, log_weights=w["log_weights"], max_goals=G)


def kernel_times(name, reps):
    d = tempfile.mkdtemp(prefix=f"sequential_rocprof_{name}_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(reps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
        if r.returncode != 0:
            raise RuntimeError(f"the rocprofv3 run exited {r.returncode}: {r.stderr[-2000:]}")
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    for k in KERNELS:
                        if k in row["Name"]:
                            out[k] = {"calls": int(row["Calls"]), "mean_us": float(row["AverageNs"]) / 1e3,
                                      "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
        if set(out) != set(KERNELS):
            raise RuntimeError(f"the rocprofv3 stats hold {sorted(out)}, not {KERNELS}")
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def run_case(name, reps, ref_fixtures):
    m, data = case(name)
    n = len(data["home_goals"])
    block = blocks_of(name, n)
    B = BLOCKS[name]
    idx = (block - 1).astype(np.int32)
    (_, device, kw), = m._loglik_groups(data)[0]
    dev = device()
    wall = {"device_calls": timed(lambda: device_calls(dev, kw, idx, B), reps),
            "sequential_scores": timed(lambda: m.sequential_scores(data, block, max_goals=G), reps)}
    kern = kernel_times(name, reps)
    got = m.sequential_scores(data, block, max_goals=G)

    import sequential_ref as QR

    keep = np.concatenate([np.nonzero(block == b)[0][:ref_fixtures] for b in range(1, B + 1)])
    sub = {key: np.asarray(v)[keep] if isinstance(v, np.ndarray) else [v[i] for i in keep] for key, v in data.items()}
    t0 = time.perf_counter()
    QR.scores(m, sub, block[keep], G=G)
    ref_s = time.perf_counter() - t0
    k = got["pareto_k"]
    res = {"draws": S, "fixtures": n, "blocks": B, "max_goals": G, "wall": wall, "kernel": kern,
           "numpy": {"fixtures": int(keep.size), "seconds": ref_s, "scaled_to_all_fixtures_s": ref_s * n / keep.size},
           "refit_from": got["refit_from"], "pareto_k_max": float(np.max(k)), "ess_min": float(np.min(got["ess"])),
           "elpd": got["elpd"], "rps": got["rps"]}
    kernel_us = sum(v["mean_us"] for v in kern.values())
    lines = [
        f"{name}: {len(m.teams)} teams, {n} fixtures in {B} blocks, S = {S} draws, max_goals = {G}",
        "  kernels: " + ", ".join(f"{kk} {kern[kk]['mean_us']:.1f} us" for kk in KERNELS) + f"; {kernel_us / 1e3:.3f} ms in all",
        f"  device calls {wall['device_calls']['median_ms']:.3f} ms end to end, sequential_scores(data, block) "
        f"{wall['sequential_scores']['median_ms']:.3f} ms (medians of {reps})",
        f"  numpy restatement on {keep.size} fixtures {ref_s:.2f} s, scaled to {n}: {ref_s * n / keep.size:.1f} s",
        f"  refit_from {got['refit_from']}, largest k {res['pareto_k_max']:.2f}, least ess {res['ess_min']:.1f}"]
    return res, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sequential"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ref-fixtures", type=int, default=4, help="fixtures of every block the restatement runs on")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        m, data = case(args.child)
        n = len(data["home_goals"])
        (_, device, kw), = m._loglik_groups(data)[0]
        dev = device()
        idx = (blocks_of(args.child, n) - 1).astype(np.int32)
        for _ in range(args.reps + 1):
            device_calls(dev, kw, idx, BLOCKS[args.child])
        return
    os.makedirs(args.out, exist_ok=True)
    results, text = {}, []
    for name in CASES:
        results[name], lines = run_case(name, args.reps, args.ref_fixtures)
        text += lines
    print("\n".join(text))
    with open(os.path.join(args.out, "sequential_bench.json"), "w") as f:
        json.dump(results, f, indent=1)
    with open(os.path.join(args.out, "sequential_bench.txt"), "w") as f:
        f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
