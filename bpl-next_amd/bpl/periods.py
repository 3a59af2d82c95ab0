"""Period markets with credible intervals: the half-time result, half-time/full-time, win both halves, score in
both halves, the highest-scoring half, a comeback, and any "by the minute" question -- a goal in the first ten
minutes, ahead after an hour (no reference counterpart).

None of these is a functional of the final scoreline grid, so `predict_markets` cannot express them.  They need
no new assumption: `predict_in_play` already lets the times of a side's goals be exchangeable within the match
(bpl/inplay.py), so its goals before the share f of the match's scoring are Binomial(final goals, f), and
Pois(x; l) Binom(a; x, f) = Pois(a; f l) Pois(x - a; (1 - f) l) fixes the joint law of the score (a, b) at the
split and the final score (x, y) of one draw:

    p(a, b, x, y) = F(x, y) Pois(a; f lh) Pois(x - a; (1 - f) lh) Pois(b; f la) Pois(y - b; (1 - f) la)

on 0 <= a <= x <= max_goals, 0 <= b <= y <= max_goals, with F the Dixon-Coles factor max(tau, 0) on the FINAL score
with the FULL-MATCH rates.  It is not renormalised and is truncated by the final score only, so summed over
(a, b) it is the grid of `predict_markets` for every f: a market that looks only at the final score has
`predict_markets`' value.  Every period market is a linear functional of p, weights W[a, b, x, y]; the device
kernel (csrc/dc_period.hip.h) forms sum W p PER DRAW in float64 and the draws are summarised as `predict_markets`
summarises them (definition: DESIGN.md section 39).

Not modelled: more than one split per call, markets given a state in progress (period markets for a match already
under way), re-weighted draws (`log_weights`), scoring intensity that differs between the periods beyond what
`split` expresses, extra time, and time-of-goal markets other than through `split`."""

from __future__ import annotations

from typing import Callable, Dict

import numpy as np

from bpl import markets as _markets
from bpl.elpd import check_draws
from bpl.markets import Market, check_quantiles, scatter_groups
from bpl.scoring import _count

PERIOD_MAX_GOALS = 31     # include/bplhip.h BPLHIP_PERIOD_MAX_GOALS
PERIOD_MAX_MARKETS = 32   # include/bplhip.h BPLHIP_PERIOD_MAX_MARKETS


class PeriodMarket:
    """A period market: `weights(G)` gives its float64 [G+1, G+1, G+1, G+1] weights indexed [a, b, x, y], (a, b) the
    score at the split and (x, y) the final score on 0..G (home goals first).  Entries with a > x or b > y are
    never read."""

    def __init__(self, name: str, weights: Callable[[int], np.ndarray]):
        self.name = name
        self._weights = weights

    def weights(self, max_goals: int) -> np.ndarray:
        g1 = max_goals + 1
        return np.ascontiguousarray(np.broadcast_to(self._weights(max_goals), (g1,) * 4), dtype=np.float64)

    def __repr__(self):
        return f"PeriodMarket({self.name})"


def _axes(max_goals: int):
    """a, b, x, y as broadcastable index arrays of the [G+1]^4 array."""
    return np.ix_(*(np.arange(max_goals + 1),) * 4)


_PICKS = {"home": _markets.home_win, "draw": _markets.draw, "away": _markets.away_win}


def _market(market) -> Market:
    """A `bpl.markets` market, or the outcome "home" | "draw" | "away"."""
    if isinstance(market, Market):
        return market
    if isinstance(market, str) and market in _PICKS:
        return _PICKS[market]()
    raise ValueError(f"expected a bpl.markets market or 'home', 'draw' or 'away', not {market!r}")


def _home(side) -> bool:
    if not isinstance(side, str) or side not in ("home", "away"):
        raise ValueError(f"side must be 'home' or 'away', not {side!r}")
    return side == "home"


def first_period(market) -> PeriodMarket:
    """`market` (a `bpl.markets` market or "home" | "draw" | "away") on the score at the split."""
    m = _market(market)

    def w(G):
        a, b, _, _ = _axes(G)
        return m.weights(G)[a, b]
    return PeriodMarket(f"first_period({m.name})", w)


def second_period(market) -> PeriodMarket:
    """`market` on the goals scored after the split, (x - a, y - b): the second period taken on its own."""
    m = _market(market)

    def w(G):
        a, b, x, y = _axes(G)
        return m.weights(G)[np.maximum(x - a, 0), np.maximum(y - b, 0)]   # (a > x or b > y: never read)
    return PeriodMarket(f"second_period({m.name})", w)


def full_time(market) -> PeriodMarket:
    """`market` on the final score: `predict_markets`' market, whatever the split."""
    m = _market(market)

    def w(G):
        _, _, x, y = _axes(G)
        return m.weights(G)[x, y]
    return PeriodMarket(f"full_time({m.name})", w)


def all_of(*period_markets) -> PeriodMarket:
    """The product of the weights: the "and" of 0/1 markets."""
    if not period_markets or not all(isinstance(m, PeriodMarket) for m in period_markets):
        raise ValueError("all_of takes one or more period markets")

    def w(G):
        out = period_markets[0].weights(G)
        for m in period_markets[1:]:
            out = out * m.weights(G)
        return out
    return PeriodMarket("all_of(" + ", ".join(m.name for m in period_markets) + ")", w)


def ht_ft(first: str, final: str) -> PeriodMarket:
    """Half-time/full-time: the outcome `first` at the split and the outcome `final` of the match, each "home" |
    "draw" | "away"; `ht_ft("draw", "home")` is level at the break, home win."""
    for pick in (first, final):
        if not isinstance(pick, str) or pick not in _PICKS:
            raise ValueError(f"an outcome must be 'home', 'draw' or 'away', not {pick!r}")
    m = all_of(first_period(first), full_time(final))
    m.name = f"ht_ft({first}, {final})"
    return m


def _from_cells(name: str, cell) -> PeriodMarket:
    return PeriodMarket(name, lambda G: cell(*_axes(G)))


def win_both_periods(side: str) -> PeriodMarket:
    """`side` wins each period taken on its own."""
    home = _home(side)
    return _from_cells(f"win_both_periods({side})",
                       (lambda a, b, x, y: (a > b) & (x - a > y - b)) if home else
                       (lambda a, b, x, y: (a < b) & (x - a < y - b)))


def win_either_period(side: str) -> PeriodMarket:
    """`side` wins at least one period taken on its own."""
    home = _home(side)
    return _from_cells(f"win_either_period({side})",
                       (lambda a, b, x, y: (a > b) | (x - a > y - b)) if home else
                       (lambda a, b, x, y: (a < b) | (x - a < y - b)))


def score_in_both_periods(side: str) -> PeriodMarket:
    """`side` scores before the split and after it."""
    home = _home(side)
    return _from_cells(f"score_in_both_periods({side})",
                       (lambda a, b, x, y: (a > 0) & (x - a > 0)) if home else
                       (lambda a, b, x, y: (b > 0) & (y - b > 0)))


def highest_scoring_period(which: str) -> PeriodMarket:
    """By the goals of both sides in the two periods: "first", "second" or "equal"."""
    if not isinstance(which, str) or which not in ("first", "second", "equal"):
        raise ValueError(f"which must be 'first', 'second' or 'equal', not {which!r}")
    cell = {"first": lambda a, b, x, y: a + b > (x - a) + (y - b),
            "second": lambda a, b, x, y: a + b < (x - a) + (y - b),
            "equal": lambda a, b, x, y: a + b == (x - a) + (y - b)}[which]
    return _from_cells(f"highest_scoring_period({which})", cell)


def comeback(side: str) -> PeriodMarket:
    """`side` is behind at the split and wins the match."""
    home = _home(side)
    return _from_cells(f"comeback({side})",
                       (lambda a, b, x, y: (a < b) & (x > y)) if home else (lambda a, b, x, y: (a > b) & (x < y)))


def period_weights(markets, max_goals: int):
    """(names, float64 [K, G+1, G+1, G+1, G+1]) of a non-empty dict name -> PeriodMarket or array [G+1, G+1, G+1,
    G+1]; ValueError for anything else, a wrong shape or a non-finite weight."""
    if not isinstance(markets, dict) or not markets:
        raise ValueError("markets must be a non-empty dict name -> period market")
    if len(markets) > PERIOD_MAX_MARKETS:
        raise ValueError(f"at most {PERIOD_MAX_MARKETS} markets, not {len(markets)}")
    shape = (max_goals + 1,) * 4
    out = np.empty((len(markets),) + shape, dtype=np.float64)
    for k, (name, market) in enumerate(markets.items()):
        if isinstance(market, PeriodMarket):
            w = market.weights(max_goals)
        elif isinstance(market, Market):
            raise ValueError(f"market {name!r} is a full-time market: wrap it in first_period, second_period or full_time")
        else:
            try:
                w = np.asarray(market, dtype=np.float64)
            except (TypeError, ValueError) as e:
                raise ValueError(f"market {name!r} is neither a period market nor an array") from e
            if w.shape != shape:
                raise ValueError(f"market {name!r} has shape {w.shape}, not {shape}")
        if not np.all(np.isfinite(w)):
            raise ValueError(f"market {name!r} has a non-finite weight")
        out[k] = w
    return tuple(markets), out


def check_split(split, n: int) -> np.ndarray:
    """float64 [n] of one number or one per fixture, every entry finite and in [0, 1]; ValueError otherwise."""
    if isinstance(split, (bool, np.bool_)):
        raise ValueError("split must be a number or one number per fixture")
    try:
        t = np.asarray(list(split) if not isinstance(split, (np.ndarray, int, float, np.number)) else split,
                       dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError("split must be a number or one number per fixture") from e
    if t.ndim == 0:
        t = np.full(n, float(t))
    if t.shape != (n,):
        raise ValueError("split must be one number or one per fixture")
    if not np.all((t >= 0.0) & (t <= 1.0)):   # (NaN fails both)
        raise ValueError("split must be finite and in [0, 1]: the share of the match's scoring before the split")
    return np.ascontiguousarray(t)


class PredictPeriods:
    """`predict_periods` for a predictor class.  Uses the class's `_fixture_groups(data, with_goals=False)` and
    `_loglik_draws()`, as `PredictMarkets` does."""

    def predict_periods(self, data, markets, split=0.5, max_goals: int = 15, quantiles=(0.05, 0.5, 0.95),
                        return_draws: bool = False) -> Dict:
        """Posterior mean, standard deviation and quantiles of PERIOD markets on the fixtures of `data` (the
        dict `predict_markets` takes; at least one fixture; the dynamic class needs `gameweek`): markets on the
        score at a split of the match together with the final score.

        `split`: one number or one per fixture, finite and in [0, 1] -- the share of the match's SCORING that
        falls before the split, not a minute.  Mapping the clock to it is yours: 0.5 treats the halves alike,
        0.45 allows for fewer goals before the break, 10 / 90 asks about the first ten minutes.  0 and 1 are
        legal (everything after, everything before).

        `markets`: a non-empty dict name -> period market (at most 32; its order is kept), a period market
        being one of this module's builders -- `first_period`, `second_period`, `full_time` (each of a
        `bpl.markets` market or "home" | "draw" | "away"), `all_of`, `ht_ft`, `win_both_periods`,
        `win_either_period`, `score_in_both_periods`, `highest_scoring_period`, `comeback` -- or a finite array
        [max_goals+1] * 4 of weights W[a, b, x, y], (a, b) the score at the split and (x, y) the final score;
        entries with a > x or b > y are never read.  Per posterior draw and fixture a market's value is
        sum W[a, b, x, y] p(a, b, x, y) over 0 <= a <= x <= max_goals, 0 <= b <= y <= max_goals (0..31), with
        p = F(x, y) Pois(a; f lh) Pois(x - a; (1 - f) lh) Pois(b; f la) Pois(y - b; (1 - f) la): goal times
        exchangeable within the match, as in `predict_in_play`; the Dixon-Coles factor F on the final score with
        the full-match rates; not renormalised, so `full_time(m)` has `predict_markets`' value of m.  Over the
        draws: the mean, standard deviation and quantiles of `predict_markets`.

        Not modelled: more than one split per call, markets given a state in progress, re-weighted draws
        (`log_weights`), scoring intensity that differs between the periods beyond what `split` expresses, extra
        time, and time-of-goal markets other than through `split`.

        Returns `predict_markets`' dict with "kind" = "periods" and "split" float64 [n] added.  Every argument
        check runs on the host before any device call (ValueError)."""
        draws = self._loglik_draws()
        check_draws(draws)
        G = _count(max_goals, "max_goals", 0, PERIOD_MAX_GOALS)
        names, w = period_weights(markets, G)
        q = check_quantiles(quantiles)
        groups, n = self._fixture_groups(data, with_goals=False)
        if n == 0:
            raise ValueError("predict_periods needs at least one fixture")
        f = check_split(split, n)
        out = {"kind": "periods", "n": n, "markets": names, "quantiles": q, "split": f}
        return scatter_groups(out, groups, n, lambda device, kw, at: device.period_summary(
            **kw, split=f[at], max_goals=G, weights=w, quantiles=q, return_draws=bool(return_draws)))
