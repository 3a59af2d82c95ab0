"""Team ratings: how good each team is against a field of opponents, how sure we are, and who is ahead of whom
(the part of numpyro's `print_summary()` a team-strength model is asked for first; no reference counterpart).

The posterior tables are identified only up to a shift and live in log-rate units.  A rating puts them in
results: per posterior draw every rated team plays every opponent of the field (both venues, one venue, or
neutral ground), and its expected points, win probability and scoring rates are averaged over those matches.
The device (csrc/dc_ratings.hip.h) forms the five statistics PER DRAW, in float64, summarises them over the
draws (mean, standard deviation, quantiles from exact order statistics) and ranks the rated teams per draw:
ranks exist only per draw, so none of this can be put together from posterior means, and the per-draw values
never leave the device unless asked for (definition: DESIGN.md section 27)."""

from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from bpl._util import check_points
from bpl.elpd import check_draws
from bpl.markets import MARKET_MAX_GOALS, check_quantiles
from bpl.scoring import _count

RATINGS_MAX_TEAMS = 1024   # include/bplhip.h BPLHIP_RATINGS_MAX_TEAMS
STATISTICS = ("points", "win", "goals_for", "goals_against", "goal_difference")   # the device's order
VENUES = ("both", "home", "away", "neutral")                                      # the device's codes
_PER_WEEK = ("mean", "sd", "quantile", "rank_count", "rank_proba", "better_count", "better_proba", "expected_rank",
             "draws")


def _names(value, table: Dict, what: str, default=None):
    """A list of team names of the model (one name, or a sequence): 1..RATINGS_MAX_TEAMS of them, no duplicates."""
    if value is None:
        value = default
    try:
        items = [value] if isinstance(value, (str, np.str_)) else list(value)
    except TypeError as e:
        raise ValueError(f"{what} must be team names") from e
    for v in items:
        if not isinstance(v, (str, np.str_)) or v not in table:
            raise ValueError(f"{what}: unknown team {v!r}")
    items = [str(v) for v in items]
    if not 1 <= len(items) <= RATINGS_MAX_TEAMS:
        raise ValueError(f"{what}: between 1 and {RATINGS_MAX_TEAMS} teams, not {len(items)}")
    if len(set(items)) != len(items):
        raise ValueError(f"{what}: a team is listed twice")
    return items


def finish(raw: Dict, draws: int) -> Dict:
    """The posterior-dependent entries of a result from one device call's raw arrays: the counts as int64 and
    the floats formed from them on the host."""
    R = raw["rank_count"].shape[0]
    rank_count = raw["rank_count"].astype(np.int64)
    better_count = raw["better_count"].astype(np.int64)
    out = {"mean": raw["mean"], "sd": raw["sd"], "quantile": raw["quantile"], "rank_count": rank_count,
           "rank_proba": rank_count / float(draws), "better_count": better_count,
           "better_proba": better_count / float(draws),
           "expected_rank": (rank_count * np.arange(R, dtype=np.int64)).sum(axis=1) / float(draws)}
    if "draws" in raw:
        out["draws"] = raw["draws"]
    return out


class TeamRatings:
    """`team_ratings` for a predictor class.  Uses the class's `teams`, `_loglik_draws()` and `_device()`; a
    venue-aware class sets `_ratings_venue_model` (its default venue is neutral ground), resolves confederations
    with `_tournament_conf` and, with one posterior per gameweek, passes `weeks`."""

    _ratings_venue_model = False

    # pylint: disable=too-many-arguments,too-many-locals
    def _team_ratings(self, teams, opponents, venue, max_goals, points, rank_by, quantiles, return_draws,
                      team_conf=None, weeks=None) -> Dict:
        draws = self._loglik_draws()
        check_draws(draws)
        table = {str(t): i for i, t in enumerate(self.teams)}
        rated = _names(teams, table, "teams", default=list(table))
        field = _names(opponents, table, "opponents", default=rated)
        in_field = set(field)
        others = np.array([len(field) - (t in in_field) for t in rated], dtype=np.int64)   # (no duplicates in field)
        if not others.all():
            raise ValueError(f"teams: {rated[int(np.argmin(others))]!r} has no opponent other than itself")
        if venue is None:
            venue = "neutral" if self._ratings_venue_model else "both"
        if not isinstance(venue, str) or venue not in VENUES:
            raise ValueError(f"venue must be one of {VENUES}, not {venue!r}")
        if venue == "neutral" and not self._ratings_venue_model:
            raise ValueError('venue="neutral" needs a venue-aware model')
        G = _count(max_goals, "max_goals", 0, MARKET_MAX_GOALS)
        pts = check_points(points)
        if not isinstance(rank_by, str) or rank_by not in STATISTICS:
            raise ValueError(f"rank_by must be one of {STATISTICS}, not {rank_by!r}")
        q = check_quantiles(quantiles)
        conf = getattr(self, "_tournament_conf", None)
        team_cf = conf(team_conf, rated) if conf else None
        field_cf = conf(team_conf, field) if conf else None
        t_idx = np.array([table[t] for t in rated], dtype=np.uint16)
        o_idx = np.array([table[t] for t in field], dtype=np.uint16)
        kw = {"venue": VENUES.index(venue), "max_goals": G, "points": pts, "rank_by": STATISTICS.index(rank_by),
              "quantiles": q, "team_conf": team_cf, "opponent_conf": field_cf, "return_draws": bool(return_draws)}
        out = {"kind": "ratings", "teams": rated, "opponents": field, "venue": venue, "statistics": STATISTICS,
               "quantiles": q, "matches": others * (2 if venue == "both" else 1)}
        if weeks is None:
            out.update(finish(self._device().team_ratings(t_idx, o_idx, **kw), draws))
            return out
        parts = [finish(self._week_device(week).team_ratings(t_idx, o_idx, **kw), draws) for week in weeks]
        out["gameweeks"] = np.array(weeks, dtype=np.int64)
        for key in _PER_WEEK:
            if key in parts[0]:
                out[key] = np.stack([p[key] for p in parts])
        return out

    def team_ratings(self, teams=None, opponents=None, venue: Optional[str] = None, max_goals: int = 15,
                     points=(3, 1, 0), rank_by: str = "points", quantiles=(0.05, 0.5, 0.95),
                     return_draws: bool = False) -> Dict:
        """Each team's strength against a field of opponents, with credible intervals and rank probabilities.

        `teams`: the rated teams (names, or one name; default every team of the model; the order is kept;
        1..1024, no duplicates).  `opponents`: the field every rated team is measured against (default the
        rated teams; 1..1024, no duplicates); a team never meets itself and needs at least one other opponent.
        `venue`: "both" (every pairing twice, the rated team hosting first and visiting second), "home" or
        "away" (one match per pairing) or "neutral" (one match on neutral ground, venue-aware classes only);
        None is "both" on the league classes and "neutral" on the venue-aware ones.

        Per posterior draw and rated team, averaged over its matches in that order (`matches` of them), with
        (p_win, p_draw, p_loss) from `forecast_scores`'s grid 0..`max_goals` (0..63, not renormalised):
        "points" = W p_win + D p_draw + L p_loss for `points` = (W, D, L); "win" = p_win; "goals_for" and
        "goals_against" the two scoring rates of the match; "goal_difference" their difference.  The rates are
        the marginal means of the unclipped Dixon-Coles law (tau leaves the marginals Poisson): they are NOT
        truncated at `max_goals`.  Over the draws, per statistic and team: the mean, the standard deviation
        (ddof=1; 0 for one draw) and `quantiles` (at most 16, each in [0, 1]) as `predict_markets` gives them.

        Ranks are per draw among the rated teams by `rank_by` (a statistic name), larger better; equal values
        rank in the order of `teams`, so a draw's ranks are a permutation.

        Returns a dict: "kind" = "ratings", "teams", "opponents", "venue", "statistics" (the five names),
        "quantiles" [Q], "mean" and "sd" float64 [5, R], "quantile" [5, Q, R], "rank_count" int64 [R, R]
        (row t, column r: the draws in which t held rank r, 0 the best), "rank_proba" = rank_count / draws,
        "better_count" int64 [R, R] ([t, u]: the draws with t strictly above u), "better_proba",
        "expected_rank" [R], "matches" int [R] and, with `return_draws`, "draws" [draws, 5, R].  Every
        argument check runs on the host before any device call (ValueError)."""
        return self._team_ratings(teams, opponents, venue, max_goals, points, rank_by, quantiles, return_draws)


def format_table(result: Dict, sort_by: str = "points", statistic: Optional[str] = None) -> str:
    """A text table of a `team_ratings()` result: team, the mean and the outer quantiles of `statistic`
    (default `sort_by`), the expected rank and P(rank 0), best first by the mean of `sort_by`.  A result of
    the dynamic class prints its last gameweek."""
    names = tuple(result["statistics"])
    statistic = sort_by if statistic is None else statistic
    for nm in (sort_by, statistic):
        if nm not in names:
            raise ValueError(f"statistic must be one of {names}, not {nm!r}")
    last = (lambda a: np.asarray(a)[-1]) if "gameweeks" in result else np.asarray
    mean, quant = last(result["mean"]), last(result["quantile"])
    erank, p0 = last(result["expected_rank"]), last(result["rank_proba"])[:, 0]
    k = names.index(statistic)
    q = np.asarray(result["quantiles"])
    order = np.argsort(-mean[names.index(sort_by)], kind="stable")
    teams = [str(t) for t in result["teams"]]
    width = max([len(t) for t in teams] + [4])
    head = f"{'team':<{width}} {statistic:>15}"
    if q.size:
        head += f" {f'q{q[0]:g}':>10} {f'q{q[-1]:g}':>10}"
    lines = [head + f" {'E[rank]':>8} {'P(rank 0)':>9}"]
    for i in order:
        row = f"{teams[i]:<{width}} {mean[k, i]:>15.4g}"
        if q.size:
            row += f" {quant[k, 0, i]:>10.4g} {quant[k, -1, i]:>10.4g}"
        lines.append(row + f" {erank[i]:>8.2f} {p0[i]:>9.3f}")
    lines.append(f"{len(teams)} teams against {len(result['opponents'])} opponents, venue {result['venue']}")
    return "\n".join(lines)
