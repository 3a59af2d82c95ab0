"""Posterior predictive checks: replicated datasets drawn from a fitted model on the fixtures of `data`,
and test statistics of the observed data set against their replicated distribution (no reference
counterpart).  Replication r takes ONE posterior draw, r mod draws, for every fixture, so the replicated
statistics carry the parameter uncertainty the fixtures share.  The device kernel is csrc/dc_ppc.hip.h;
it reduces each replication to integer tallies, and everything derived from them (variances,
correlation, points, p-values) is computed here, by the same function for the observed data and for
every replication (definition: DESIGN.md section 13)."""

from __future__ import annotations

from typing import Dict

import numpy as np

from bpl._util import MAX_MATCH_POINTS, check_points

# include/bplhip.h BPLHIP_PPC_*
PPC_MAX_FIXTURES = 1 << 22
PPC_MAX_TEAMS = 1024
PPC_MAX_GOALS = 15
PPC_MAX_REPLICATIONS = 1 << 20
PPC_MAX_TEAM_CELLS = 1 << 26
PPC_MAX_SCORE_CELLS = 1 << 30
PPC_MAX_MATCH_POINTS = MAX_MATCH_POINTS   # as simulate_season's

STATISTICS = ("scoreline", "outcome", "home_goals", "away_goals", "home_goals_var", "away_goals_var",
              "goals_corr", "team_goals_for", "team_goals_against", "team_points")


def _count(value, name: str, lo: int, hi: int) -> int:
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
        raise ValueError(f"{name} must be an integer")
    if not lo <= int(value) <= hi:
        raise ValueError(f"{name} must be in [{lo}, {hi}], not {value}")
    return int(value)


def tallies(home_goals, away_goals, home_slot, away_slot, n_slots: int, max_goals: int) -> Dict[str, np.ndarray]:
    """The device's per-replication tallies (HipContext.ppc) of ONE data set, with a leading axis of 1:
    "score" [1, G+1, G+1], "outcome" [1, 3], "sums" [1, 5], "team" [1, k, 4] (int64)."""
    x, y = np.asarray(home_goals, dtype=np.int64), np.asarray(away_goals, dtype=np.int64)
    hs, as_ = np.asarray(home_slot, dtype=np.int64), np.asarray(away_slot, dtype=np.int64)
    g1 = max_goals + 1
    score = np.zeros((g1, g1), dtype=np.int64)
    np.add.at(score, (np.minimum(x, max_goals), np.minimum(y, max_goals)), 1)
    hw, dr = int(np.sum(x > y)), int(np.sum(x == y))
    team = np.zeros((n_slots, 4), dtype=np.int64)
    for col, sl, v in ((0, hs, x), (0, as_, y), (1, hs, y), (1, as_, x), (2, hs, x > y), (2, as_, y > x),
                       (3, hs, x == y), (3, as_, x == y)):
        np.add.at(team[:, col], sl, v.astype(np.int64))
    return {"score": score[None], "outcome": np.array([[hw, dr, x.size - hw - dr]], dtype=np.int64),
            "sums": np.array([[x.sum(), y.sum(), (x * x).sum(), (y * y).sum(), (x * y).sum()]], dtype=np.int64),
            "team": team[None]}


def moments(sums, n: int):
    """(home_goals_var, away_goals_var, goals_corr) from integer sums [..., 5] = (sum x, sum y, sum x^2,
    sum y^2, sum x y) over n fixtures: population variances and the Pearson correlation (0 when a
    variance is 0).  The centred numerators n sum x^2 - (sum x)^2 etc. are exact in int64."""
    s = np.asarray(sums, dtype=np.int64)
    sx, sy, sxx, syy, sxy = (s[..., i] for i in range(5))
    n = np.int64(n)
    vx, vy, cxy = n * sxx - sx * sx, n * syy - sy * sy, n * sxy - sx * sy
    n2 = float(n) * float(n)
    ok = (vx > 0) & (vy > 0)
    denom = np.sqrt(np.where(ok, vx, 1).astype(np.float64) * np.where(ok, vy, 1).astype(np.float64))
    corr = np.where(ok, np.clip(cxy / denom, -1.0, 1.0), 0.0)
    return vx / n2, vy / n2, corr


def statistics(raw: Dict[str, np.ndarray], n: int, games: np.ndarray, points) -> Dict[str, np.ndarray]:
    """Every test statistic, with a leading replication axis, from tallies in HipContext.ppc's layout.
    games [k]: each slot's number of fixtures; points = (win, draw, loss)."""
    team = np.asarray(raw["team"], dtype=np.int64)
    sums = np.asarray(raw["sums"], dtype=np.int64)
    win, draw, loss = points
    wins, draws = team[..., 2], team[..., 3]
    var_x, var_y, corr = moments(sums, n)
    return {"scoreline": np.asarray(raw["score"], dtype=np.int64),
            "outcome": np.asarray(raw["outcome"], dtype=np.int64),
            "home_goals": sums[..., 0], "away_goals": sums[..., 1], "home_goals_var": var_x,
            "away_goals_var": var_y, "goals_corr": corr, "team_goals_for": team[..., 0],
            "team_goals_against": team[..., 1],
            "team_points": win * wins + draw * draws + loss * (np.asarray(games, dtype=np.int64) - wins - draws)}


class PosteriorPredictiveCheck:
    """`posterior_predictive_check` for a predictor class.  Uses the class's PointwiseLikelihood
    interface: `_loglik_groups(data)` (host checks, team lookups, one device query per group) and
    `_loglik_draws()`."""

    def posterior_predictive_check(self, data, num_replications=None, random_state=None, max_goals: int = 6,
                                   points=(3, 1, 0), return_replications: bool = False) -> Dict:
        """Posterior predictive check on the fixtures of `data` (the dict `log_likelihood` takes: the keys
        `fit` reads per fixture; others are ignored).

        Replication r (0 <= r < R, R = num_replications, default the number of posterior draws) takes
        posterior draw r mod draws for EVERY fixture and draws each fixture's scoreline exactly as
        `simulate_season` does, from max(tau, 0) Poisson Poisson / Z with that draw's rates (no
        max_goals truncation; goals capped at 255), on threefry block (r, f), f the fixture's 0-based
        position in `data`.  The dynamic class uses each fixture's own gameweek.  `random_state` seeds
        the key (None: the clock).

        Each statistic is computed identically for the observed data and for every replication; k is
        the number of teams in `data` (model order, "teams"):
          "scoreline"   [G+1, G+1] counts, G = max_goals (1..15); the last row / column is "G or more"
          "outcome"     [3] home wins, draws, away wins (exact scorelines)
          "home_goals", "away_goals"            totals
          "home_goals_var", "away_goals_var"    population variances over the fixtures
          "goals_corr"  Pearson correlation of home and away goals (0 when a variance is 0)
          "team_goals_for", "team_goals_against", "team_points"   [k]; points = (win, draw, loss)
        Returns a dict with, per statistic, a dict of "observed" (the statistic's shape), "replicated"
        ([R] + that shape), "p_upper" = mean over r of (replicated >= observed) and "p_lower" = mean of
        (replicated <= observed) (the statistic's shape); and "n" (fixtures), "num_replications" (R),
        "teams" [k].  With return_replications also "replications": {"home_goals", "away_goals"}, the
        replicated scorelines as uint8 [R, n] in data order (a dict of its own: the top-level "home_goals"
        and "away_goals" are the goal-total statistics).  Every argument check runs on the host before any
        device call (ValueError)."""
        from bpl._ffi import prng_key
        from bpl.base import _wall_clock_seed

        draws = self._loglik_draws()
        R = draws if num_replications is None else _count(num_replications, "num_replications", 1,
                                                                PPC_MAX_REPLICATIONS)
        if R > PPC_MAX_REPLICATIONS:
            raise ValueError(f"{R} posterior draws: pass num_replications <= {PPC_MAX_REPLICATIONS}")
        G = _count(max_goals, "max_goals", 1, PPC_MAX_GOALS)
        pts = check_points(points)
        groups, n = self._loglik_groups(data)
        if n == 0:
            raise ValueError("posterior_predictive_check needs at least one fixture")
        if n > PPC_MAX_FIXTURES:
            raise ValueError(f"{n} fixtures: at most {PPC_MAX_FIXTURES}")
        h, a = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
        x, y = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
        for positions, _, kw in groups:
            at = slice(None) if positions is None else positions
            h[at], a[at], x[at], y[at] = kw["home_idx"], kw["away_idx"], kw["home_goals"], kw["away_goals"]
        team_idx = np.union1d(h, a)
        k = team_idx.size
        if k > PPC_MAX_TEAMS:
            raise ValueError(f"{k} teams in data: at most {PPC_MAX_TEAMS}")
        if R * k > PPC_MAX_TEAM_CELLS:
            raise ValueError(f"num_replications x teams = {R * k}: at most {PPC_MAX_TEAM_CELLS}")
        if return_replications and R * n > PPC_MAX_SCORE_CELLS:
            raise ValueError(f"num_replications x fixtures = {R * n} replicated scorelines: at most "
                             f"{PPC_MAX_SCORE_CELLS}")
        hs, as_ = np.searchsorted(team_idx, h), np.searchsorted(team_idx, a)
        key = prng_key(_wall_clock_seed() if random_state is None else random_state)

        g1 = G + 1
        raw = {"score": np.zeros((R, g1, g1), dtype=np.int64), "outcome": np.zeros((R, 3), dtype=np.int64),
               "sums": np.zeros((R, 5), dtype=np.int64), "team": np.zeros((R, k, 4), dtype=np.int64)}
        reps = {}
        if return_replications:
            reps = {"home_goals": np.empty((R, n), dtype=np.uint8), "away_goals": np.empty((R, n), dtype=np.uint8)}
        for positions, device, kw in groups:
            at = slice(None) if positions is None else positions
            part = device().ppc(kw["home_idx"], kw["away_idx"], hs[at], as_[at], k, G, R, key,
                                fixture_id=None if positions is None else positions, neutral=kw.get("neutral"),
                                conf=kw.get("conf"), return_scores=return_replications)
            for nm in raw:
                raw[nm] += part[nm]
            for nm in reps:
                reps[nm][:, at] = part[nm]

        games = np.bincount(hs, minlength=k) + np.bincount(as_, minlength=k)
        rep = statistics(raw, n, games, pts)
        obs = statistics(tallies(x, y, hs, as_, k, G), n, games, pts)
        out = {"n": n, "num_replications": R, "teams": np.asarray(self.teams)[team_idx]}
        for nm in STATISTICS:
            o, r = obs[nm][0], rep[nm]
            out[nm] = {"observed": o, "replicated": r, "p_upper": np.mean(r >= o, axis=0),
                       "p_lower": np.mean(r <= o, axis=0)}
        if return_replications:
            out["replications"] = reps
        return out
