"""season_trajectory restated in numpy (csrc/dc_trajectory.hip.h, bpl/base.py): from the per-simulation scorelines
of simulate_season(return_scores=True) the table after every matchday is rebuilt from the fixtures whose label is at
most that matchday and ranked with tests/h2h_ref.py's rules (`season_positions` for the head-to-head order,
`overall_ahead` and `words` for the overall one); the paths are cross-tabulated into the eight integer tables and the
derived floats are written out cell by cell from their definitions.  Nothing here calls the code under test."""
import numpy as np

import h2h_ref as H


def paths(home_slot, away_slot, matchday, home_goals, away_goals, table, points, key, head_to_head=False,
          pair_init=None):
    """(matchdays [R], position int64 [N, R, n], points int64 [N, R, n]): the table after each matchday of every
    simulation.  home_slot / away_slot [F] table slots, matchday [F] labels, home_goals / away_goals [N, F] in the
    fixtures' order, table [n, 3], key the threefry key of the run."""
    hs, as_ = np.asarray(home_slot, np.int64), np.asarray(away_slot, np.int64)
    labels = np.asarray(matchday).astype(np.int64)
    x, y = np.asarray(home_goals).astype(np.int64), np.asarray(away_goals).astype(np.int64)
    table = np.asarray(table).astype(np.int64)
    N, n = x.shape[0], table.shape[0]
    days = np.unique(labels)
    position = np.empty((N, days.size, n), dtype=np.int64)
    pts_out = np.empty((N, days.size, n), dtype=np.int64)
    win, draw, loss = points
    w = None if head_to_head else H.words(key, N, n)
    for r, day in enumerate(days):
        sel = labels <= day
        if head_to_head:
            position[:, r], pts_out[:, r] = H.season_positions(hs[sel], as_[sel], x[:, sel], y[:, sel], table, points,
                                                                key, pair_init)
            continue
        xs, ys = x[:, sel], y[:, sel]
        pts, gf, ga = (np.tile(table[:, c], (N, 1)) for c in range(3))
        rows = np.broadcast_to(np.arange(N)[:, None], xs.shape)
        Hs, As = np.broadcast_to(hs[sel], xs.shape), np.broadcast_to(as_[sel], xs.shape)
        ph = np.where(xs > ys, win, np.where(xs == ys, draw, loss))
        pa = np.where(ys > xs, win, np.where(xs == ys, draw, loss))
        for acc, sl, v in ((pts, Hs, ph), (pts, As, pa), (gf, Hs, xs), (gf, As, ys), (ga, Hs, ys), (ga, As, xs)):
            np.add.at(acc, (rows, sl), v)
        position[:, r] = H.overall_ahead(pts, gf, ga, w).sum(axis=1)
        pts_out[:, r] = pts
    return days, position, pts_out


def counts(position, points, inside):
    """position, points [N, R, n] and inside [K, n] (target, position) -> the eight tables as a dict, int64."""
    pos, pts, inside = np.asarray(position), np.asarray(points), np.asarray(inside)
    N, R, n = pos.shape
    K = inside.shape[0]
    rr = np.broadcast_to(np.arange(R)[None, :, None], pos.shape)
    tt = np.broadcast_to(np.arange(n)[None, None, :], pos.shape)
    position_count = np.zeros((R, n, n), dtype=np.int64)
    np.add.at(position_count, (rr, tt, pos), 1)
    within = inside[:, pos].transpose(1, 2, 3, 0)                       # [N, R, n, K]
    final = within[:, R - 1][:, None]                                   # [N, 1, n, K]
    out = {
        "position_count": position_count,
        "target_count": within.sum(axis=0).astype(np.int64),
        "target_final_count": (within & final).sum(axis=0).astype(np.int64),
        "points_sum": pts.sum(axis=0).astype(np.int64),
        "points_sq_sum": (pts * pts).sum(axis=0).astype(np.int64),
        "rounds_inside_count": np.zeros((n, K, R + 1), dtype=np.int64),
        "secured_count": np.zeros((n, K, R + 1), dtype=np.int64),
        "lead_changes_count": np.zeros(R, dtype=np.int64),
    }
    spent = within.sum(axis=1)                                          # [N, n, K]
    # the earliest matchday from which inside after it and every later one: one past the last matchday outside
    day = np.arange(1, R + 1)[None, :, None, None]
    since = np.where(within, 0, day).max(axis=1)                        # [N, n, K]; R: outside at the end
    tk = np.broadcast_to(np.arange(n)[None, :, None], spent.shape)
    kk = np.broadcast_to(np.arange(K)[None, None, :], spent.shape)
    np.add.at(out["rounds_inside_count"], (tk, kk, spent), 1)
    np.add.at(out["secured_count"], (tk, kk, since), 1)
    leader = (pos == 0).argmax(axis=2)                                  # [N, R]
    assert ((pos == 0).sum(axis=2) == 1).all()
    np.add.at(out["lead_changes_count"], (leader[:, 1:] != leader[:, :-1]).sum(axis=1), 1)
    return out


def derived(tables, n_sims):
    """The host-side floats from the eight integer tables, one cell at a time."""
    pc, tc, tf = tables["position_count"], tables["target_count"], tables["target_final_count"]
    R, n, K = tc.shape
    N = int(n_sims)
    out = {
        "position_proba": np.empty((R, n, n)), "target_proba": np.empty((R, n, K)),
        "final_given_inside": np.full((R, n, K), np.nan), "final_given_inside_se": np.full((R, n, K), np.nan),
        "final_given_outside": np.full((R, n, K), np.nan), "final_given_outside_se": np.full((R, n, K), np.nan),
        "points_mean": np.empty((R, n)), "points_sd": np.empty((R, n)),
        "expected_rounds_inside": np.empty((n, K)), "secured_by_proba": np.empty((n, K, R)),
    }
    for r in range(R):
        for t in range(n):
            for p in range(n):
                out["position_proba"][r, t, p] = int(pc[r, t, p]) / N
            s1, s2 = int(tables["points_sum"][r, t]), int(tables["points_sq_sum"][r, t])
            out["points_mean"][r, t] = float(s1) / N
            out["points_sd"][r, t] = np.sqrt(float(N * s2 - s1 * s1)) / N
            for k in range(K):
                m, both, end = int(tc[r, t, k]), int(tf[r, t, k]), int(tc[R - 1, t, k])
                out["target_proba"][r, t, k] = m / N
                if m > 0:
                    q = both / m
                    out["final_given_inside"][r, t, k] = q
                    out["final_given_inside_se"][r, t, k] = np.sqrt(q * (1.0 - q) / m)
                if N - m > 0:
                    q = (end - both) / (N - m)
                    out["final_given_outside"][r, t, k] = q
                    out["final_given_outside_se"][r, t, k] = np.sqrt(q * (1.0 - q) / (N - m))
    for t in range(n):
        for k in range(K):
            out["expected_rounds_inside"][t, k] = sum(
                b * int(v) for b, v in enumerate(tables["rounds_inside_count"][t, k])) / N
            run = 0
            for r in range(R):
                run += int(tables["secured_count"][t, k, r])
                out["secured_by_proba"][t, k, r] = run / N
    out["expected_lead_changes"] = sum(b * int(v) for b, v in enumerate(tables["lead_changes_count"])) / N
    return out
