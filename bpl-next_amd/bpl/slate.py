"""Several fixtures at once: accumulators, the number of home wins of a matchday, the points of a prediction-league
entry, a pools coupon (no reference counterpart).

A leg gives every final score (x, y) of its fixture an integer number of points 0..7; a slate is a list of
fixtures and its total is the sum of their legs.  The fixtures share the posterior -- a draw in which one club is
strong lifts every leg on that club -- so E_draw[prod p_i] is not prod E_draw[p_i], and multiplying posterior means
under-prices accumulators.  Given ONE draw the fixtures are independent, so that draw's law of the total is exact:
the convolution of the legs' value laws on the grid of `predict_markets` (q = max(tau, 0) Poisson Poisson over
0..max_goals, not renormalised).  The device kernel (csrc/dc_slate.hip.h) forms it PER DRAW, in float64, and only
then summarises over the draws: mean, standard deviation and quantiles from exact order statistics.  No Monte
Carlo; results are bit-reproducible (definition: DESIGN.md section 31)."""

from __future__ import annotations

from typing import Dict

import numpy as np

from bpl.elpd import check_draws
from bpl.markets import MARKET_MAX_GOALS, Market, away_win, check_quantiles, draw, home_win
from bpl.scoring import _count
from bpl.sequential import relabel_blocks

SLATE_VALUES = 8         # include/bplhip.h BPLHIP_SLATE_VALUES: a leg's values are 0..7
SLATE_MAX_TOTAL = 127    # include/bplhip.h BPLHIP_SLATE_MAX_TOTAL
SLATE_MAX_LEGS = 1024    # include/bplhip.h BPLHIP_SLATE_MAX_LEGS


def pick(outcome: str) -> Market:
    """1 when the match ends as picked: "home", "draw" or "away"."""
    if outcome not in ("home", "draw", "away"):
        raise ValueError(f"outcome must be 'home', 'draw' or 'away', not {outcome!r}")
    return {"home": home_win, "draw": draw, "away": away_win}[outcome]()


def capped(market: Market, cap: int) -> Market:
    """min(the market's weights, cap), cap 1..7: `capped(total_goals(), 3)` counts goals up to three."""
    if not isinstance(market, Market):
        raise ValueError(f"capped takes a market, not {market!r}")
    cap = _count(cap, "cap", 1, SLATE_VALUES - 1)
    return Market(f"capped({market.name}, {cap})", lambda x, y: np.minimum(market._cell(x, y), cap))


def prediction_points(home_goals: int, away_goals: int, exact: int = 3, goal_difference=None, result: int = 1) -> Market:
    """Prediction-league scoring of the predicted score home_goals-away_goals: the exact score scores `exact`;
    otherwise the right goal difference scores `goal_difference` if given; otherwise the right result scores
    `result`; otherwise 0.  Integers with 0 <= result <= goal_difference <= exact <= 7."""
    hx, ay = _count(home_goals, "home_goals", 0, 255), _count(away_goals, "away_goals", 0, 255)
    e = _count(exact, "exact", 0, SLATE_VALUES - 1)
    gd = None if goal_difference is None else _count(goal_difference, "goal_difference", 0, e)
    r = _count(result, "result", 0, e if gd is None else gd)

    def cell(x, y):
        points = np.where(np.sign(x - y) == np.sign(hx - ay), r, 0)
        if gd is not None:
            points = np.where(x - y == hx - ay, gd, points)
        return np.where((x == hx) & (y == ay), e, points)

    return Market(f"prediction_points({hx}, {ay}, exact={e}, goal_difference={gd}, result={r})", cell)


def leg_tables(legs, n: int, max_goals: int):
    """(tables uint8 [L, G+1, G+1], leg_table int32 [n]) of `legs`: one leg for every fixture or a sequence of n
    legs, a leg being a Market or an array [G+1, G+1] (an ndarray or a nested list of numbers) with integer values
    0..7 on the grid.  Equal legs share a table.  ValueError for anything else, naming the fixture."""
    g1 = max_goals + 1
    if isinstance(legs, (list, tuple)) and legs and all(isinstance(row, (list, tuple)) and row and not
                                                        isinstance(row[0], (list, tuple, np.ndarray, Market))
                                                        for row in legs):
        try:   # a nested list [G+1][G+1] of numbers is one leg: a leg of a sequence is itself two-dimensional
            legs = np.asarray(legs, dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError("legs given as a nested list must be one rectangular array of numbers") from e
    if isinstance(legs, Market) or isinstance(legs, np.ndarray) and legs.ndim == 2:
        legs = [legs] * n
    try:
        legs = list(legs)
    except TypeError as e:
        raise ValueError("legs must be one leg or a sequence with one leg per fixture") from e
    if len(legs) != n:
        raise ValueError(f"{len(legs)} legs for {n} fixtures")
    tables, index, seen, by_id = [], np.empty(n, dtype=np.int32), {}, {}
    for i, leg in enumerate(legs):
        if id(leg) in by_id:
            index[i] = by_id[id(leg)]
            continue
        if isinstance(leg, Market):
            w = leg.weights(max_goals)
        else:
            try:
                w = np.asarray(leg, dtype=np.float64)
            except (TypeError, ValueError) as e:
                raise ValueError(f"the leg of fixture {i} is neither a market nor an array") from e
            if w.shape != (g1, g1):
                raise ValueError(f"the leg of fixture {i} has shape {w.shape}, not {(g1, g1)}")
        if not np.all(np.isfinite(w) & (w == np.round(w)) & (w >= 0)):
            raise ValueError(f"the leg of fixture {i} must give every score a whole number of points, 0 or more")
        if w.max() > SLATE_VALUES - 1:
            raise ValueError(f"the leg of fixture {i} is worth up to {w.max():g} points, at most {SLATE_VALUES - 1}: "
                             "cap it (bpl.slate.capped)")
        t = w.astype(np.uint8)
        key = t.tobytes()
        if key not in seen:
            seen[key] = len(tables)
            tables.append(t)
        index[i] = by_id[id(leg)] = seen[key]
    return np.stack(tables), index


def slate_index(slate, n: int):
    """(labels int64 [J], index int64 [n]) of `slate`: None (one slate, label 0) or one integer label per fixture."""
    if slate is None:
        return np.zeros(1, dtype=np.int64), np.zeros(n, dtype=np.int64)
    try:
        return relabel_blocks(slate, n)
    except (TypeError, ValueError) as e:
        raise ValueError(f"slate must be None or one integer label per fixture: {e}") from e


def independent_pmf(leg_proba, leg_top, index, J: int, rows: int) -> np.ndarray:
    """[J, rows]: every slate's law of the total from the posterior MEANS of its legs' laws -- `leg_proba` [n, 8],
    leg i with the values 0..leg_top[i] -- convolved in list order in float64: what ignoring the shared posterior
    gives."""
    out = np.zeros((J, rows))
    for j in range(J):
        pmf = np.ones(1)
        for i in np.nonzero(index == j)[0]:
            pmf = np.convolve(pmf, leg_proba[i, :leg_top[i] + 1])
        out[j, :pmf.size] = pmf
    return out


def _rows(kw, at):
    """The query keyword arguments of `_fixture_groups` for the fixtures `at` of the group."""
    return {k: None if v is None else tuple(np.asarray(c)[at] for c in v) if isinstance(v, tuple) else np.asarray(v)[at]
            for k, v in kw.items()}


class PredictSlate:
    """`predict_slate` for a predictor class.  Uses the class's `_fixture_groups(data, with_goals=False)` and
    `_loglik_draws()`, as `PredictMarkets` does."""

    def predict_slate(self, data, legs, slate=None, max_goals: int = 15, quantiles=(0.05, 0.5, 0.95),
                      return_draws: bool = False) -> Dict:
        """The law of the total of `legs` over slates of the fixtures of `data` (`predict_markets`' data; at least
        one fixture; the dynamic class needs `gameweek`, and a slate's fixtures must lie in one gameweek).

        `legs`: one leg for every fixture or a sequence with one per fixture.  A leg gives every final score on
        the grid 0..max_goals (0..63) a whole number of points 0..7: a `bpl.markets` market with such weights
        (`home_win()`, `btts()`, `total_over(2.5)`, `correct_score(..)` ...), an integer array [max_goals+1,
        max_goals+1] (axis 0 the home goals) or one of this module's builders `pick`, `capped`,
        `prediction_points`.  `slate`: None (all fixtures are one slate) or one integer label per fixture; the
        distinct labels, sorted, are the J slates, each with its fixtures in list order, at most 1024 of them,
        whose largest values add up to at most 127.

        Per posterior draw a slate's total T has the law pmf = the convolution of its legs' value laws on the
        grid of `predict_markets` (exact given the draw; not renormalised, so it sums to `mass`, the product of
        the fixtures' grid masses).  Per draw also at_least[t] = P(T >= t) and expected = sum_t t pmf[t].  Over
        the draws each has its mean, standard deviation (ddof=1) and `quantiles`, as in `predict_markets`.

        Returns a dict: "kind" = "slate", "n", "slates" int64 [J] (the labels), "size", "max_total" int64 [J],
        "totals" = arange(P+1) with P the largest max_total, "quantiles" [Q]; "pmf", "pmf_sd", "at_least",
        "at_least_sd" float64 [J, P+1] (an exact 0 beyond a slate's max_total), "pmf_quantile",
        "at_least_quantile" [J, Q, P+1]; "expected", "expected_sd", "mass" [J], "expected_quantile" [J, Q];
        "top_proba" [J] = pmf[j, max_total[j]], the accumulator when every leg is 0/1; "leg_proba" [n, 8], each
        leg's value law averaged over the draws; "independent_pmf", "independent_at_least" [J, P+1], what
        convolving those posterior means gives -- the answer that ignores the shared posterior, for comparison;
        with `return_draws`, "pmf_draws" [draws, J, P+1].  Every argument check runs on the host before any
        device call (ValueError)."""
        draws = self._loglik_draws()
        check_draws(draws)
        G = _count(max_goals, "max_goals", 0, MARKET_MAX_GOALS)
        q = check_quantiles(quantiles)
        groups, n = self._fixture_groups(data, with_goals=False)
        if n == 0:
            raise ValueError("predict_slate needs at least one fixture")
        tables, leg_table = leg_tables(legs, n, G)
        labels, index = slate_index(slate, n)
        J = labels.size
        size = np.bincount(index, minlength=J).astype(np.int64)
        tops = tables.reshape(tables.shape[0], -1).max(axis=1).astype(np.int64)
        max_total = np.bincount(index, weights=tops[leg_table], minlength=J).astype(np.int64)
        for j in range(J):
            if size[j] > SLATE_MAX_LEGS:
                raise ValueError(f"slate {labels[j]} has {size[j]} legs, at most {SLATE_MAX_LEGS}")
            if max_total[j] > SLATE_MAX_TOTAL:
                raise ValueError(f"slate {labels[j]} can total {max_total[j]} points, at most {SLATE_MAX_TOTAL}")
        group_of = np.full(J, -1)
        for g, (positions, _, _) in enumerate(groups):
            for j in np.unique(index if positions is None else index[positions]):
                if group_of[j] >= 0:
                    raise ValueError(f"slate {labels[j]} spans more than one gameweek")
                group_of[j] = g
        P = int(max_total.max())
        Q = q.size
        out = {"kind": "slate", "n": n, "slates": labels, "size": size, "max_total": max_total,
               "totals": np.arange(P + 1), "quantiles": q, "leg_proba": np.empty((n, SLATE_VALUES))}
        for name in ("pmf", "at_least"):
            out[name], out[f"{name}_sd"] = np.zeros((J, P + 1)), np.zeros((J, P + 1))
            out[f"{name}_quantile"] = np.zeros((J, Q, P + 1))
        for name in ("expected", "expected_sd", "mass"):
            out[name] = np.empty(J)
        out["expected_quantile"] = np.empty((J, Q))
        if return_draws:
            out["pmf_draws"] = np.zeros((draws, J, P + 1))
        for positions, device, kw in groups:
            at = np.arange(n) if positions is None else np.asarray(positions)
            order = np.argsort(index[at], kind="stable")   # each slate's fixtures together, in list order
            at = at[order]
            js, counts = np.unique(index[at], return_counts=True)
            start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
            part = device().slate_summary(**_rows(kw, order), max_goals=G, tables=tables, leg_table=leg_table[at],
                                          start=start, quantiles=q, return_draws=bool(return_draws))
            pt = (part["mean"].shape[0] - 2) // 2   # this call's P + 1
            for name, lo in (("pmf", 0), ("at_least", pt)):
                out[name][js, :pt] = part["mean"][lo:lo + pt].T
                out[f"{name}_sd"][js, :pt] = part["sd"][lo:lo + pt].T
                out[f"{name}_quantile"][js, :, :pt] = part["quantile"][lo:lo + pt].transpose(2, 1, 0)
            out["expected"][js], out["expected_sd"][js] = part["mean"][2 * pt], part["sd"][2 * pt]
            out["expected_quantile"][js] = part["quantile"][2 * pt].T
            out["mass"][js] = part["mean"][2 * pt + 1]
            out["leg_proba"][at] = part["leg_proba"]
            if return_draws:
                out["pmf_draws"][:, js, :pt] = part["draws"]
        out["top_proba"] = out["pmf"][np.arange(J), max_total]
        out["independent_pmf"] = independent_pmf(out["leg_proba"], tops[leg_table], index, J, P + 1)
        out["independent_at_least"] = np.cumsum(out["independent_pmf"][:, ::-1], axis=1)[:, ::-1].copy()
        return out
