"""match_leverage, points_needed and match_scenarios with matches in progress on one MI355X
(csrc/dc_live_queries.hip.h) next to their kick-off forms at tools/live_bench.py's shape:

    live    N simulations of 370 fixtures still to kick off + 10 matches in play (a 20-team double round robin with
            one round in progress) over 1000 posterior draws, the draws re-weighted by the ten states and resampled;
    plain   N simulations of the same 380 fixtures from kick-off.

    python tools/live_queries_bench.py [--out DIR] [--reps N] [--sims N]

Reports, from ONE `rocprofv3 --kernel-trace --stats` run (a child process; profiler off for the wall times): the time
of each live recording kernel beside its kick-off twin's, and dc_season_live beside dc_season in that same run -- the
ratio the three new ones are read against; the wall time of every device call and public method (medians of N after a
warm-up); and the only route without the keywords, `simulate_season(in_play=..., return_tables=True,
return_scores=True)` plus the numpy cross-tabulations of tests/leverage_ref.py, points_ref.py and scenarios_ref.py,
whose tables must equal the device's.  The key fixtures of match_scenarios are three of the matches in play, cap 1.
Writes live_queries_bench.json and live_queries_bench.txt under --out (default: profiles/live_queries)."""
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

from live_bench import S, SEED, STATES, T, league, timed  # noqa: E402

# (query, its live recording kernel, the kick-off twin); dc_season_live / dc_season lead as the yardstick
PAIRS = (("simulate_season", "dc_season_live<false>", "dc_season<false>"),
         ("match_leverage", "live_leverage_sim<false>", "dc_leverage_sim<false>"),
         ("points_needed", "live_points_sim<false>", "dc_points_sim<false>"),
         ("match_scenarios", "live_scenario_sim<false>", "dc_scenario_sim<false>"))
OTHERS = ("live_loglik", "live_weights", "dc_leverage_count", "dc_points_count", "dc_scenario_count")
KERNELS = tuple(k for _, a, b in PAIRS for k in (a, b)) + OTHERS
N_KEYS = 3


def calls(n_sims):
    """{query: {"live" | "plain": (the device call, the public method)}} and what the numpy route needs."""
    from bpl._ffi import prng_key
    from bpl.base import leverage_targets, points_axis

    key = prng_key(SEED)
    m, h, a, live, ip = league()
    hh, aa, table_idx, table, points, n = m._season_inputs(h, a, n_sims, None, None, (3, 1, 0))
    ipr = m._in_play_inputs(ip)
    _, masks = leverage_targets(None, table_idx.size)
    points_min, n_bins = points_axis(table[:, 0], hh, aa, points)      # (slots are the model indices here)
    F = int((~live).sum())
    keys_live = list(range(F, F + N_KEYS))                              # matches 0..2 in play
    keys_plain = [int(f) for f in np.flatnonzero(live)[:N_KEYS]]        # the same matches in the full list
    caps = [1] * N_KEYS
    dev = m._device()
    lv, pl = (hh[~live], aa[~live], table_idx, table, points, n, key), (hh, aa, table_idx, table, points, n, key)
    kw = dict(num_simulations=n_sims, random_state=SEED)
    return {
        "simulate_season": {
            "live": (lambda: dev.simulate_season_live(*lv, in_play=ipr),
                     lambda: m.simulate_season(h[~live], a[~live], in_play=ip, **kw)),
            "plain": (lambda: dev.simulate_season(*pl), lambda: m.simulate_season(h, a, **kw))},
        "match_leverage": {
            "live": (lambda: dev.match_leverage_live(*lv, masks, in_play=ipr),
                     lambda: m.match_leverage(h[~live], a[~live], in_play=ip, **kw)),
            "plain": (lambda: dev.match_leverage(*pl, masks), lambda: m.match_leverage(h, a, **kw))},
        "points_needed": {
            "live": (lambda: dev.season_points_live(*lv, masks, points_min, n_bins, in_play=ipr),
                     lambda: m.points_needed(h[~live], a[~live], in_play=ip, **kw)),
            "plain": (lambda: dev.season_points(*pl, masks, points_min, n_bins), lambda: m.points_needed(h, a, **kw))},
        "match_scenarios": {
            "live": (lambda: dev.season_scenarios_live(*lv, masks, keys_live, caps, in_play=ipr),
                     lambda: m.match_scenarios(h[~live], a[~live], keys_live, in_play=ip, **kw)),
            "plain": (lambda: dev.season_scenarios(*pl, masks, keys_plain, caps),
                      lambda: m.match_scenarios(h, a, keys_plain, **kw))},
    }, (m, h, a, live, ip, keys_live, caps)


def kernel_times(n_sims, reps):
    """Per device call: the summed duration of each kernel's launches (the stages run once per chunk; live_loglik
    and live_weights run once per live call, so theirs is the sum over the four live calls)."""
    d = tempfile.mkdtemp(prefix="live_queries_rocprof_")
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
                    k = next((k for k in KERNELS if k in row["Name"]), None)
                    if k:
                        n = int(row["Calls"])
                        out[k] = {"launches": n, "launches_per_call": n / (reps + 1),
                                  "us_per_call": float(row["TotalDurationNs"]) / 1e3 / (reps + 1)}
        if set(out) != set(KERNELS):
            raise RuntimeError(f"the rocprofv3 stats hold {sorted(out)}, not {sorted(KERNELS)}")
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def numpy_route(todo, ctx, n_sims):
    """The route without the keywords: one live season with per-simulation tables and scores, then one numpy
    cross-tabulation per query; (seconds, whether every integer table equals the device's)."""
    import leverage_ref as VR
    import points_ref as PR
    import scenarios_ref as SR
    from bpl.base import LEVERAGE_TARGETS

    m, h, a, live, ip, keys, caps = ctx
    t0 = time.perf_counter()
    sim = m.simulate_season(h[~live], a[~live], num_simulations=n_sims, random_state=SEED, in_play=ip,
                            return_tables=True, return_scores=True)
    hg = np.concatenate([sim["home_goals"], sim["in_play_home_goals"]], axis=1)
    ag = np.concatenate([sim["away_goals"], sim["in_play_away_goals"]], axis=1)
    secs = {"simulate_season_s": time.perf_counter() - t0}
    inside = VR.target_masks(LEVERAGE_TARGETS, T)
    got = {q: todo[q]["live"][1]() for q in ("match_leverage", "points_needed", "match_scenarios")}
    pts = got["points_needed"]["points"]
    routes = {"match_leverage": (("outcome_count", "target_count", "joint_count"),
                                 lambda: VR.counts(sim["position"], hg, ag, inside)),
              "points_needed": (("team_points_count", "team_target_count", "position_points_count", "gap_count"),
                                lambda: PR.counts(sim["points"], sim["position"], inside, int(pts[0]), pts.size)),
              "match_scenarios": (("scenario_count", "joint_count"),
                                  lambda: SR.counts(sim["position"], hg, ag, inside, keys, caps))}
    same = {}
    for q, (names, fn) in routes.items():
        t0 = time.perf_counter()
        ref = fn()
        secs[q + "_numpy_s"] = time.perf_counter() - t0
        same[q] = bool(all(np.array_equal(got[q][k], r) for k, r in zip(names, ref)))
    return secs, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "live_queries"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sims", type=int, default=100_000)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    N = args.sims
    todo, ctx = calls(N)
    if args.child:
        for _ in range(args.reps + 1):
            for modes in todo.values():
                for pair in modes.values():
                    pair[0]()
        return
    os.makedirs(args.out, exist_ok=True)
    wall = {q: {mode: {"device_call": timed(pair[0], args.reps), "end_to_end": timed(pair[1], args.reps)}
                for mode, pair in modes.items()} for q, modes in todo.items()}
    kern = kernel_times(N, args.reps)
    route, same = numpy_route(todo, ctx, N)
    ratios = {q: kern[lk]["us_per_call"] / kern[pk]["us_per_call"] for q, lk, pk in PAIRS}
    F, L = T * (T - 1) - len(STATES), len(STATES)
    res = {"simulations": N, "draws": S, "teams": T, "fixtures": F, "in_play": L, "key_fixtures": ctx[5],
           "wall": wall, "kernel": kern, "live_over_kick_off_kernel_time": ratios, "numpy_route": route,
           "tables_equal_the_numpy_route": same}
    lines = [f"{N} simulations, {S} draws, {T} teams: {F} fixtures + {L} in play v {T * (T - 1)} fixtures from kick-off"]
    for q, lk, pk in PAIRS:
        w = wall[q]
        lines.append(f"  {q}: {lk} {kern[lk]['us_per_call']:.1f} us per call ({kern[lk]['launches_per_call']:.0f} "
                     f"launches), {pk} {kern[pk]['us_per_call']:.1f} us: x {ratios[q]:.2f}; device call "
                     f"{w['live']['device_call']['median_ms']:.3f} ms live v {w['plain']['device_call']['median_ms']:.3f} "
                     f"ms, public method {w['live']['end_to_end']['median_ms']:.3f} v "
                     f"{w['plain']['end_to_end']['median_ms']:.3f} ms (medians of {args.reps})")
    lines.append(f"  live_loglik {kern['live_loglik']['us_per_call'] / 4:.1f} us, live_weights "
                 f"{kern['live_weights']['us_per_call'] / 4:.1f} us per live call; dc_leverage_count "
                 f"{kern['dc_leverage_count']['us_per_call'] / 2:.1f} us, dc_points_count "
                 f"{kern['dc_points_count']['us_per_call'] / 2:.1f} us, dc_scenario_count "
                 f"{kern['dc_scenario_count']['us_per_call'] / 2:.1f} us per call (live and kick-off alike)")
    lines.append(f"  without the keywords: simulate_season(in_play, return_tables, return_scores) "
                 f"{route['simulate_season_s']:.3f} s, then numpy")
    for q in ("match_leverage", "points_needed", "match_scenarios"):
        total = route["simulate_season_s"] + route[q + "_numpy_s"]
        lines.append(f"    {q}: + {route[q + '_numpy_s']:.3f} s = {total:.3f} s: "
                     f"{total * 1e3 / wall[q]['live']['end_to_end']['median_ms']:.0f} x the public method; tables equal: "
                     f"{same[q]}")
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(args.out, "live_queries_bench.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.join(args.out, "live_queries_bench.txt"), "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
