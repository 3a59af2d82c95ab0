"""Markets of a match in progress: `predict_markets` given the minute and the score, with the posterior draws
re-weighted by what has happened so far (no reference counterpart).

Under one draw's Dixon-Coles law the final score (x, y) has probability tau(x, y) Pois(x; lh) Pois(y; la).  Let the
times of a side's goals be exchangeable within the match (iid uniform given their number): the goals scored
before the elapsed fraction t are then Binomial(x, t), and Pois(x; l) Binom(a; x, t) = Pois(a; l t)
Pois(x - a; l (1 - t)) factorises the joint law of the state (a, b) at t and the final score:

    P_s(state, final) = Pois(a; lh t) Pois(b; la t) * tau_s(x, y) Pois(x - a; lh r) Pois(y - b; la r),  r = 1 - t

The second factor, normalised, is the conditional law of the final score of that draw: a shifted grid with
thinned rates whose four tau cells still sit on the FINAL score with the FULL-MATCH rates.  The first factor
times the normaliser Z is the likelihood of the state under the draw: evidence about the team strengths, by
which the draws are re-weighted -- what `sequential_scores` does between gameweeks, applied inside a match.  The
device kernels are csrc/dc_inplay.hip.h (definition: DESIGN.md section 25).

Not modelled: goal intensity that varies over the match (late goals are more frequent than early ones), red cards
and game state (a side protecting a lead), stoppage time (the caller maps the clock to `elapsed`), and a joint
update over several matches in progress: every fixture re-weights the draws on its own."""

from __future__ import annotations

from typing import Dict

import numpy as np

from bpl.markets import MARKET_MAX_GOALS, check_quantiles, market_weights, scatter_groups
from bpl.scoring import _count

INPLAY_MAX_DRAWS = 12288   # include/bplhip.h BPLHIP_INPLAY_MAX_DRAWS


def check_elapsed(elapsed, n: int) -> np.ndarray:
    """float64 [n], every entry in [0, 1); ValueError otherwise."""
    try:
        t = np.asarray(list(elapsed) if not isinstance(elapsed, np.ndarray) else elapsed, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError("elapsed must be numbers") from e
    if t.shape != (n,):
        raise ValueError("elapsed must be one value per fixture")
    if not np.all((t >= 0.0) & (t < 1.0)):   # (NaN fails both)
        raise ValueError("elapsed must be in [0, 1): the fraction of the match played")
    return np.ascontiguousarray(t)


def check_log_weights(log_weights, draws: int):
    """None, or float64 [draws], all finite; ValueError otherwise."""
    if log_weights is None:
        return None
    try:
        lw = np.asarray(log_weights, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError("log_weights must be numbers") from e
    if lw.shape != (draws,):
        raise ValueError(f"log_weights must have shape ({draws},), one value per posterior draw")
    if not np.all(np.isfinite(lw)):
        raise ValueError("log_weights must be finite")
    return np.ascontiguousarray(lw)


class PredictInPlay:
    """`predict_in_play` for a predictor class.  Uses the class's `_fixture_groups(data, with_goals=True)` (host
    checks, team lookups, one device query per group) and `_loglik_draws()`, as `PredictMarkets` does."""

    def predict_in_play(self, data, markets, max_goals: int = 15, quantiles=(0.05, 0.5, 0.95), reweight: bool = True,
                        log_weights=None, return_draws: bool = False) -> Dict:
        """Posterior mean, standard deviation and quantiles of match markets on matches IN PROGRESS: `data` is
        the dict `predict_markets` takes plus `home_goals`, `away_goals` (the current score, each at most
        `max_goals`) and `elapsed` (the fraction of the match played, in [0, 1); 0 only at 0-0).  The same
        fixture may appear many times with different states: that is a win-probability chart.

        Per posterior draw a market's value is sum_xy W[x, y] p(x, y | state), W indexed by the FINAL score
        (every builder of `bpl.markets` means what it says) and p the draw's conditional law of the final
        score: remaining goals Poisson with the rates thinned by 1 - elapsed, the Dixon-Coles factor on the
        final score with the full-match rates, normalised over all scores; the mass beyond `max_goals` is
        dropped, as in `predict_markets`.  With `reweight` the draws are weighted, per fixture, by the
        likelihood of the state under each draw (a side that is 3-0 up after half an hour was probably
        underrated); `log_weights` [draws], e.g. a row of `sequential_scores(return_weights=True)
        ["log_weights"]`, is added to the log weights, and with `reweight=False` and a kick-off state gives
        the updated-without-a-refit forecast with credible intervals.  Over the weighted draws, per market and
        fixture: the mean, the standard deviation (population form: no ddof) and for each of `quantiles` the
        weighted inverted CDF -- the draws sorted by value, the first whose cumulative weight reaches q times
        the total; no interpolation (equal weights: numpy's method="inverted_cdf"); q = 0 is the minimum and
        q = 1 the maximum.

        Not modelled: goal intensity that varies over the match, red cards and game state, stoppage time (map
        the clock to `elapsed` yourself), and a joint update over several matches in progress: every fixture
        re-weights the draws on its own (`simulate_season(in_play=..., return_weights=True)["log_weights"]` holds
        the joint weights; pass them as `log_weights` with `reweight=False`).

        Returns a dict: "kind" = "in_play", "n", "markets" (the names), "quantiles" float64 [Q], "mean" and
        "sd" float64 [K, n], "quantile" [K, Q, n], "ess" [n] (the effective sample size of the weights, at
        most the number of draws), "log_evidence" [n] (the posterior-predictive log probability of the state,
        whatever `reweight` is) and, with `return_draws`, "draws" [draws, K, n] and "draw_log_evidence"
        [draws, n].  At most 12 288 draws.  Every argument check runs on the host before any device call
        (ValueError)."""
        draws = self._loglik_draws()
        if draws > INPLAY_MAX_DRAWS:
            raise ValueError(f"{draws} posterior draws: predict_in_play takes at most {INPLAY_MAX_DRAWS}")
        G = _count(max_goals, "max_goals", 0, MARKET_MAX_GOALS)
        names, w = market_weights(markets, G)
        q = check_quantiles(quantiles)
        lw = check_log_weights(log_weights, draws)
        if not isinstance(data, dict) or "elapsed" not in data:
            raise ValueError("data has no 'elapsed'")
        groups, n = self._fixture_groups(data, with_goals=True)
        if n == 0:
            raise ValueError("predict_in_play needs at least one fixture")
        t = check_elapsed(data["elapsed"], n)
        for positions, _, kw in groups:
            at = slice(None) if positions is None else positions
            x, y = np.asarray(kw["home_goals"]), np.asarray(kw["away_goals"])
            if x.max() > G or y.max() > G:
                raise ValueError(f"a current score beyond max_goals = {G}")
            if np.any((t[at] == 0.0) & ((x != 0) | (y != 0))):
                raise ValueError("elapsed = 0 with a score other than 0-0")
        out = {"kind": "in_play", "n": n, "markets": names, "quantiles": q}
        return scatter_groups(out, groups, n, lambda device, kw, at: device.inplay_summary(
            **kw, elapsed=t[at], max_goals=G, weights=w, quantiles=q, reweight=bool(reweight), log_weights=lw,
            return_draws=bool(return_draws)))
