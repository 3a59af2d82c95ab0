"""numpy restatement of `posterior_predictive_check` (bpl/ppc.py, csrc/dc_ppc.hip.h) for the tests: the
rates of each class, operation for operation (dc_season's plain form; tournament_ref's venue form with
on = 1 - neutral_venue; the dynamic class's per-gameweek tables), season_ref's threefry blocks (r, f) and
exact sampler, and the per-replication tallies and statistics written out independently of bpl/ppc.py.
A replication is flagged when a comparison of one of its walks came within season_ref.FLAG_TOL of its
boundary, the only place where exp's last bit can change a draw."""
import numpy as np

import season_ref as SR
import tournament_ref as TR
from bpl.base import BaseMatchPredictor
from bpl.dynamic_dixon_coles import DynamicNeutralDixonColesMatchPredictor
from bpl.neutral_dixon_coles_WC import NeutralDixonColesMatchPredictorWC


def queries(m, data):
    """Model indices and goals of data's fixtures: dict of h, a, x, y and, per class, nv, hc, ac, gw."""
    names = {t: i for i, t in enumerate(m.teams)}
    q = {"h": np.array([names[t] for t in data["home_team"]], dtype=np.int64),
         "a": np.array([names[t] for t in data["away_team"]], dtype=np.int64),
         "x": np.asarray(data["home_goals"], dtype=np.int64), "y": np.asarray(data["away_goals"], dtype=np.int64)}
    if not isinstance(m, BaseMatchPredictor):
        q["nv"] = np.asarray(data["neutral_venue"], dtype=np.int64)
    if isinstance(m, NeutralDixonColesMatchPredictorWC):
        conf = {c: i for i, c in enumerate(m.conferences)}
        q["hc"] = np.array([conf[c] for c in data["home_conf"]], dtype=np.int64)
        q["ac"] = np.array([conf[c] for c in data["away_conf"]], dtype=np.int64)
    if isinstance(m, DynamicNeutralDixonColesMatchPredictor):
        q["gw"] = np.asarray(data["gameweek"], dtype=np.int64)
    return q


def rates(m, q, s):
    """Home and away rates [R, n] of replications drawing posterior draws s [R]."""
    S2, F2 = np.meshgrid(np.asarray(s, dtype=np.int64), np.arange(q["h"].size), indexing="ij")
    H2, A2 = q["h"][F2], q["a"][F2]
    if isinstance(m, BaseMatchPredictor):
        ha = np.asarray(m.home_advantage, np.float64)
        edge = ha[S2] if ha.ndim == 1 else ha[S2, H2]
        att, dfn = np.asarray(m.attack, np.float64), np.asarray(m.defence, np.float64)
        return np.exp((att[S2, H2] - dfn[S2, A2]) + edge), np.exp(att[S2, A2] - dfn[S2, H2])
    on = q["nv"][F2] == 0
    if isinstance(m, DynamicNeutralDixonColesMatchPredictor):
        # week w's [S, T] tables, gathered per fixture: index (s, w * T + t) of the [S, G * T] reshape
        W2 = q["gw"][F2]
        T = len(m.teams)
        tabs = {nm: np.asarray(getattr(m, nm), np.float64).reshape(np.shape(getattr(m, nm))[0], -1) for nm in
                ("attack", "defence", "home_attack", "away_attack", "home_defence", "away_defence")}
        return TR.rates(tabs, S2, W2 * T + H2, W2 * T + A2, on)
    tabs = TR.model_tables(m)
    ch = ca = None
    if tabs["confederation_strength"] is not None:
        ch, ca = q["hc"][F2], q["ac"][F2]
    return TR.rates(tabs, S2, H2, A2, on, ch, ca)


def replicate(m, data, num_replications, key, fixture_id=None):
    """x, y int64 [R, n] and flagged [R] of the R replications under the threefry key (hi, lo).
    fixture_id [n]: the fixtures' counters (HipContext.ppc's fixture_id; None: 0..n-1, their positions)."""
    q = queries(m, data)
    R, n = int(num_replications), q["h"].size
    S = int(np.shape(m.corr_coef)[0])
    r = np.arange(R, dtype=np.int64)
    s = r % S
    lh, la = rates(m, q, s)
    fid = np.arange(n, dtype=np.uint32) if fixture_id is None else np.asarray(fixture_id, dtype=np.int64).astype(np.uint32)
    o0, o1 = SR.threefry_block(key, r[:, None].astype(np.uint32), fid[None, :])
    rho = np.broadcast_to(np.asarray(m.corr_coef, np.float64)[s][:, None], (R, n))
    x, y, fl = SR.sample_scorelines(lh.ravel(), la.ravel(), rho.ravel(), SR.unit_open(o0).ravel(),
                                    SR.unit_open(o1).ravel())
    return x.reshape(R, n), y.reshape(R, n), fl.reshape(R, n).any(axis=1)


def raw_tallies(x, y, hs, as_, k, max_goals):
    """HipContext.ppc's raw layout for replications x, y [R, n]: "score" [R, G+1, G+1], "outcome" [R, 3],
    "sums" [R, 5], "team" [R, k, 4] (goals for, against, wins, draws)."""
    x, y = np.atleast_2d(np.asarray(x, np.int64)), np.atleast_2d(np.asarray(y, np.int64))
    R, n = x.shape
    g1 = max_goals + 1
    cell = np.minimum(x, max_goals) * g1 + np.minimum(y, max_goals)
    score = np.stack([np.bincount(c, minlength=g1 * g1) for c in cell]).reshape(R, g1, g1)
    hw, dr = (x > y).sum(axis=1), (x == y).sum(axis=1)
    outcome = np.stack([hw, dr, n - hw - dr], axis=1)
    sums = np.stack([x.sum(1), y.sum(1), (x * x).sum(1), (y * y).sum(1), (x * y).sum(1)], axis=1)
    team = np.zeros((R, k, 4), dtype=np.int64)
    for j in range(R):
        for col, vh, va in ((0, x[j], y[j]), (1, y[j], x[j]), (2, x[j] > y[j], y[j] > x[j]),
                            (3, x[j] == y[j], x[j] == y[j])):
            team[j, :, col] = np.bincount(hs, weights=vh, minlength=k) + np.bincount(as_, weights=va, minlength=k)
    return {"score": score, "outcome": outcome, "sums": sums, "team": team}


def stats(x, y, hs, as_, k, max_goals, points=(3, 1, 0)):
    """The statistics of replications x, y [R, n] (or one data set [n]) with a leading axis, from
    numpy's own var and corrcoef (float results agree with bpl/ppc.py's to rounding)."""
    x, y = np.atleast_2d(np.asarray(x, np.int64)), np.atleast_2d(np.asarray(y, np.int64))
    raw = raw_tallies(x, y, hs, as_, k, max_goals)
    vx, vy = x.var(axis=1), y.var(axis=1)
    corr = np.array([0.0 if a == 0 or b == 0 else np.corrcoef(xi, yi)[0, 1] for a, b, xi, yi in zip(vx, vy, x, y)])
    games = np.bincount(hs, minlength=k) + np.bincount(as_, minlength=k)
    w, d = raw["team"][..., 2], raw["team"][..., 3]
    return {"scoreline": raw["score"], "outcome": raw["outcome"], "home_goals": raw["sums"][:, 0],
            "away_goals": raw["sums"][:, 1], "home_goals_var": vx, "away_goals_var": vy, "goals_corr": corr,
            "team_goals_for": raw["team"][..., 0], "team_goals_against": raw["team"][..., 1],
            "team_points": points[0] * w + points[1] * d + points[2] * (games - w - d)}


def slots(m, data):
    """(teams [k] model indices, home slots, away slots) of data's fixtures."""
    q = queries(m, data)
    idx = np.union1d(q["h"], q["a"])
    return idx, np.searchsorted(idx, q["h"]), np.searchsorted(idx, q["a"])
