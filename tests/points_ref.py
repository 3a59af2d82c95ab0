"""points_needed restated in numpy (csrc/dc_points.hip.h, bpl/base.py): the cross-tabulation of per-simulation
points and finishing positions -- what simulate_season(return_tables=True) gives -- into the four integer count
tables, the points axis, and the derived floats written out cell by cell from their definitions."""
import numpy as np


def axis(init_points, home_slot, away_slot, points):
    """(points_min, P): slot t with m_t remaining matches ends on init_t + m_t min(points) .. init_t + m_t max(points)."""
    lo, hi = [], []
    for t, p0 in enumerate(init_points):
        m = sum(1 for s in home_slot if s == t) + sum(1 for s in away_slot if s == t)
        lo.append(int(p0) + m * min(points))
        hi.append(int(p0) + m * max(points))
    return min(lo), max(hi) - min(lo) + 1


def counts(points, position, inside, points_min, P):
    """points [N, n] and position [N, n] (slot -> finishing position), inside [K, n] (target, position) ->
    team_points int64 [n, P], team_target [n, P, K], position_points [n, P], gap [n - 1, P]."""
    pts = np.asarray(points).astype(np.int64) - points_min
    pos = np.asarray(position).astype(np.int64)
    inside = np.asarray(inside)
    N, n = pts.shape
    K = inside.shape[0]
    assert pts.min() >= 0 and pts.max() < P
    slots = np.broadcast_to(np.arange(n), (N, n))
    team_points = np.zeros((n, P), dtype=np.int64)
    np.add.at(team_points, (slots, pts), 1)
    team_target = np.zeros((n, P, K), dtype=np.int64)
    for k in range(K):
        np.add.at(team_target[:, :, k], (slots, pts), inside[k][pos].astype(np.int64))
    by_pos = np.empty_like(pts)                                # [N, position] -> bin
    np.put_along_axis(by_pos, pos, pts, axis=1)
    position_points = np.zeros((n, P), dtype=np.int64)
    np.add.at(position_points, (slots, by_pos), 1)
    gap = np.zeros((n - 1, P), dtype=np.int64)
    if n > 1:
        d = by_pos[:, :-1] - by_pos[:, 1:]
        assert d.min() >= 0
        np.add.at(gap, (slots[:, :-1], d), 1)
    return team_points, team_target, position_points, gap


def derived(team_points, team_target, position_points, gap, points_min, n_sims, levels):
    """The host-side floats from the integer tables, one cell at a time."""
    n, P, K = team_target.shape
    L = len(levels)
    pts = [points_min + p for p in range(P)]
    out = {
        "team_points_proba": np.empty((n, P)), "target_count": np.zeros((n, K), dtype=np.int64),
        "target_proba": np.empty((n, K)),
        "proba_given_points": np.full((n, P, K), np.nan), "se_given_points": np.full((n, P, K), np.nan),
        "proba_given_at_least": np.full((n, P, K), np.nan), "points_needed": np.full((n, K, L), np.nan),
        "position_points_mean": np.empty(n), "position_points_quantile": np.empty((L, n), dtype=np.int64),
        "level_proba": np.empty(n - 1),
    }
    for t in range(n):
        for p in range(P):
            m = int(team_points[t, p])
            out["team_points_proba"][t, p] = m / n_sims
            at_least = sum(int(v) for v in team_points[t, p:])
            for k in range(K):
                if m > 0:
                    q = int(team_target[t, p, k]) / m
                    out["proba_given_points"][t, p, k] = q
                    out["se_given_points"][t, p, k] = np.sqrt(q * (1.0 - q) / m)
                if at_least > 0:
                    out["proba_given_at_least"][t, p, k] = sum(int(v) for v in team_target[t, p:, k]) / at_least
        for k in range(K):
            total = sum(int(v) for v in team_target[t, :, k])
            out["target_count"][t, k] = total
            out["target_proba"][t, k] = total / n_sims
            for l, level in enumerate(levels):
                for p in range(P):
                    q = out["proba_given_at_least"][t, p, k]
                    if not np.isnan(q) and q >= level:
                        out["points_needed"][t, k, l] = pts[p]
                        break
        out["position_points_mean"][t] = sum(int(position_points[t, p]) * pts[p] for p in range(P)) / n_sims
        for l, level in enumerate(levels):
            run = 0
            for p in range(P):
                run += int(position_points[t, p])
                if run / n_sims >= level:
                    out["position_points_quantile"][l, t] = pts[p]
                    break
    for g in range(n - 1):
        out["level_proba"][g] = int(gap[g, 0]) / n_sims
    return out
