"""Match markets with credible intervals: over / under, both teams to score, clean sheets, handicaps, expected
goals, correct scores and the three outcomes, each as a posterior distribution rather than a posterior mean
(no reference counterpart).

Every market is a linear functional of one draw's scoreline grid: weights W[x, y] (axis 0 the home goals)
on q(x, y) = max(tau, 0) Poisson Poisson over 0..max_goals, not renormalised -- the grid `forecast_scores`
sums into triangles.  The device kernel (csrc/dc_market.hip.h) forms sum_xy W q PER DRAW, in float64, and
summarises over the draws: mean, standard deviation and quantiles from exact order statistics.  A quantile
of a sum is not a sum of quantiles, so none of this can be put together from posterior means; the
[draws, fixtures, G+1, G+1] grids are never stored (definition: DESIGN.md section 16)."""

from __future__ import annotations

import math
from typing import Callable, Dict

import numpy as np

from bpl.elpd import check_draws
from bpl.scoring import _count

MARKET_MAX_GOALS = 63      # csrc/dc_market.hip.h MARKET_MAX_GOALS
MARKET_MAX_MARKETS = 64    # include/bplhip.h BPLHIP_MARKET_MAX_MARKETS
MARKET_MAX_QUANTILES = 16  # include/bplhip.h BPLHIP_MARKET_MAX_QUANTILES


class Market:
    """A market: `weights(G)` gives its float64 [G+1, G+1] weights on the grid 0..G (axis 0 the home goals)."""

    def __init__(self, name: str, cell: Callable[[np.ndarray, np.ndarray], np.ndarray]):
        self.name = name
        self._cell = cell

    def weights(self, max_goals: int) -> np.ndarray:
        x, y = np.meshgrid(np.arange(max_goals + 1), np.arange(max_goals + 1), indexing="ij")
        return np.ascontiguousarray(np.broadcast_to(self._cell(x, y), x.shape), dtype=np.float64)

    def __repr__(self):
        return f"Market({self.name})"


def _side(side: str) -> bool:
    if side not in ("home", "away"):
        raise ValueError(f"side must be 'home' or 'away', not {side!r}")
    return side == "home"


def _line(line) -> float:
    if isinstance(line, (bool, np.bool_)) or not isinstance(line, (int, float, np.integer, np.floating)) \
            or not math.isfinite(float(line)):
        raise ValueError(f"line must be a finite number, not {line!r}")
    return float(line)


def home_win() -> Market:
    return Market("home_win", lambda x, y: x > y)


def draw() -> Market:
    return Market("draw", lambda x, y: x == y)


def away_win() -> Market:
    return Market("away_win", lambda x, y: x < y)


def total_over(line) -> Market:
    """More than `line` goals in the match; with an integer line the cells on it (the push) weigh 0."""
    line = _line(line)
    return Market(f"total_over({line:g})", lambda x, y: x + y > line)


def total_under(line) -> Market:
    """Fewer than `line` goals in the match; with an integer line the cells on it (the push) weigh 0."""
    line = _line(line)
    return Market(f"total_under({line:g})", lambda x, y: x + y < line)


def handicap(line, side: str = "home") -> Market:
    """`side` wins after `line` goals are added to its score: home goals + line > away goals for "home"."""
    line, home = _line(line), _side(side)
    return Market(f"handicap({line:g}, {side})", (lambda x, y: x + line > y) if home else (lambda x, y: y + line > x))


def btts() -> Market:
    """Both teams score."""
    return Market("btts", lambda x, y: (x > 0) & (y > 0))


def clean_sheet(side: str) -> Market:
    """`side` concedes nothing: away goals = 0 for "home"."""
    home = _side(side)
    return Market(f"clean_sheet({side})", (lambda x, y: y == 0) if home else (lambda x, y: x == 0))


def correct_score(home_goals: int, away_goals: int) -> Market:
    """The scoreline itself; all zeros if the cell is off the grid."""
    hx, ay = _count(home_goals, "home_goals", 0, 255), _count(away_goals, "away_goals", 0, 255)
    return Market(f"correct_score({hx}, {ay})", lambda x, y: (x == hx) & (y == ay))


def goals(side: str) -> Market:
    """The goals of `side` (weight x for "home", y for "away"): its expected goals on the grid."""
    home = _side(side)
    return Market(f"goals({side})", (lambda x, y: x + 0 * y) if home else (lambda x, y: y + 0 * x))


def total_goals() -> Market:
    return Market("total_goals", lambda x, y: x + y)


def first_goal(side: str) -> Market:
    """`side` scores the first goal of the match: weight x / (x + y) for "home", y / (x + y) for "away" and 0 at
    0-0 -- P(that side scores first | final score) when goal times are exchangeable within the match, the
    assumption of `predict_in_play` and `predict_periods`."""
    home = _side(side)
    return Market(f"first_goal({side})",
                  lambda x, y: np.where(x + y > 0, (x if home else y) / np.maximum(x + y, 1), 0.0))


def market_weights(markets, max_goals: int):
    """(names, float64 [K, G+1, G+1]) of a non-empty dict name -> Market or array [G+1, G+1]; ValueError for
    anything else, a wrong shape or a non-finite weight."""
    if not isinstance(markets, dict) or not markets:
        raise ValueError("markets must be a non-empty dict name -> market")
    if len(markets) > MARKET_MAX_MARKETS:
        raise ValueError(f"at most {MARKET_MAX_MARKETS} markets, not {len(markets)}")
    g1 = max_goals + 1
    out = np.empty((len(markets), g1, g1), dtype=np.float64)
    for k, (name, market) in enumerate(markets.items()):
        if isinstance(market, Market):
            w = market.weights(max_goals)
        else:
            try:
                w = np.asarray(market, dtype=np.float64)
            except (TypeError, ValueError) as e:
                raise ValueError(f"market {name!r} is neither a market nor an array") from e
            if w.shape != (g1, g1):
                raise ValueError(f"market {name!r} has shape {w.shape}, not {(g1, g1)}")
        if not np.all(np.isfinite(w)):
            raise ValueError(f"market {name!r} has a non-finite weight")
        out[k] = w
    return tuple(markets), out


def check_quantiles(quantiles) -> np.ndarray:
    try:
        q = np.asarray(quantiles, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError("quantiles must be numbers") from e
    if q.ndim != 1:
        raise ValueError("quantiles must be a sequence of numbers")
    if q.size > MARKET_MAX_QUANTILES:
        raise ValueError(f"at most {MARKET_MAX_QUANTILES} quantiles, not {q.size}")
    if not np.all(np.isfinite(q) & (q >= 0.0) & (q <= 1.0)):
        raise ValueError("quantiles must be finite and in [0, 1]")
    return np.ascontiguousarray(q)


def scatter_groups(out: Dict, groups, n: int, query) -> Dict:
    """`out` completed by one device query per group of `_fixture_groups`: query(device, kw, at) returns the summary
    of the group's fixtures (positions `at` of the n), and each of its arrays [..., len(at)] goes to out[key][..., at],
    float64 [..., n] made when the key is first seen (so the keys follow in the query's order)."""
    for positions, device, kw in groups:
        at = slice(None) if positions is None else positions
        for key, value in query(device(), kw, at).items():
            if key not in out:
                out[key] = np.empty(value.shape[:-1] + (n,), dtype=np.float64)
            out[key][..., at] = value
    return out


class PredictMarkets:
    """`predict_markets` for a predictor class.  Uses the class's `_fixture_groups(data, with_goals=False)` (host
    checks, team lookups, one device query per group: the fixture part of `_loglik_groups`) and
    `_loglik_draws()`."""

    def predict_markets(self, data, markets, max_goals: int = 15, quantiles=(0.05, 0.5, 0.95),
                        return_draws: bool = False) -> Dict:
        """Posterior mean, standard deviation and quantiles of match markets on the fixtures of `data` (the
        dict `log_likelihood` takes, without the goal columns -- ignored if present; at least one fixture;
        the dynamic class needs `gameweek`).

        `markets`: a non-empty dict name -> market (at most 64; its order is kept), a market being one of
        this module's builders (`home_win`, `draw`, `away_win`, `total_over`, `total_under`, `handicap`,
        `btts`, `clean_sheet`, `correct_score`, `goals`, `total_goals`, `first_goal`) or a finite array [max_goals+1,
        max_goals+1] of weights W[x, y], axis 0 the home goals.  Per posterior draw and fixture a market's
        value is sum_xy W[x, y] q(x, y) with q = max(tau, 0) Poisson Poisson over 0..max_goals (0..63), not
        renormalised: the grid of `forecast_scores`.  Over the draws, per market and fixture: the mean, the
        standard deviation (ddof=1; 0 for one draw) and for each of `quantiles` (at most 16, each in
        [0, 1]; none is allowed) the linearly interpolated quantile of the exact per-draw values (numpy's
        default method).

        Returns a dict: "kind" = "markets", "n", "markets" (the names), "quantiles" float64 [Q], "mean" and
        "sd" float64 [K, n], "quantile" [K, Q, n] and, with `return_draws`, "draws" [draws, K, n].  Every
        argument check runs on the host before any device call (ValueError)."""
        draws = self._loglik_draws()
        check_draws(draws)
        G = _count(max_goals, "max_goals", 0, MARKET_MAX_GOALS)
        names, w = market_weights(markets, G)
        q = check_quantiles(quantiles)
        groups, n = self._fixture_groups(data, with_goals=False)
        if n == 0:
            raise ValueError("predict_markets needs at least one fixture")
        out = {"kind": "markets", "n": n, "markets": names, "quantiles": q}
        return scatter_groups(out, groups, n, lambda device, kw, at: device.market_summary(
            **kw, max_goals=G, weights=w, quantiles=q, return_draws=bool(return_draws)))
