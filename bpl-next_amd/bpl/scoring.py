"""Forecast verification: proper scoring rules of a fitted model's win / draw / loss forecasts on fixtures
with known results -- usually held-out ones -- and `compare_scores` to rank several fits on the same
matches (no reference counterpart).  The held-out companion of waic / loo / compare_elpd (bpl/elpd.py).

Per posterior draw s and fixture n the outcome probabilities p(s, n) = (p_H, p_D, p_A) are the triangle
sums of max(tau, 0) Poisson Poisson on the grid 0..max_goals, not renormalised: exactly what
`predict_outcome_proba(max_goals=...)` averages.  The device kernel (csrc/dc_score.hip.h) evaluates them
in float64 in O(max_goals) each and reduces over both axes: the forecast P = mean_s p(s, n) per fixture,
and per draw the sums over the fixtures of the three rules on that draw's own p.  The rules on P, the
standard errors and the reliability table are computed here (definition: DESIGN.md section 15)."""

from __future__ import annotations

import math
from typing import Dict

import numpy as np

from bpl.elpd import check_draws

SCORE_MAX_GOALS = 63   # GRID_MAX_GOALS (bpl/base.py), csrc/dc_score.hip.h SCORE_MAX_GOALS
SCORE_MAX_BINS = 1000
RULES = ("rps", "brier", "log_score")   # lower is better for the first two, higher for the log score


def _count(value, name: str, lo: int, hi: int) -> int:
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
        raise ValueError(f"{name} must be an integer")
    if not lo <= int(value) <= hi:
        raise ValueError(f"{name} must be in [{lo}, {hi}], not {value}")
    return int(value)


def outcomes(home_goals, away_goals) -> np.ndarray:
    """Observed classes from the actual goals: 0 home win, 1 draw, 2 away win (uint8)."""
    x, y = np.asarray(home_goals, dtype=np.int64), np.asarray(away_goals, dtype=np.int64)
    return np.where(x > y, 0, np.where(x == y, 1, 2)).astype(np.uint8)


def rules(proba, outcome) -> Dict[str, np.ndarray]:
    """The three rules of probability triples `proba` [..., n, 3] against `outcome` [n]: "log_score" =
    log p_o (-inf for p_o = 0), "brier" = sum_k (p_k - 1[k = o])^2 and "rps" = ((p_H - o_H)^2 +
    (p_H + p_D - o_H - o_D)^2) / 2, each [..., n]."""
    p = np.asarray(proba, dtype=np.float64)
    o = np.asarray(outcome, dtype=np.int64)
    hit = np.eye(3)[o]
    with np.errstate(divide="ignore"):
        log_score = np.log(np.take_along_axis(p, np.broadcast_to(o[:, None], p.shape[:-1] + (1,)), axis=-1)[..., 0])
    d = p - hit
    c2 = (p[..., 0] + p[..., 1]) - (hit[:, 0] + hit[:, 1])
    return {"log_score": log_score, "brier": np.sum(d * d, axis=-1), "rps": 0.5 * (d[..., 0] ** 2 + c2 * c2)}


def _se_mean(pointwise: np.ndarray) -> float:
    """std(pointwise, ddof=1) / sqrt(n); 0 for one fixture, inf when a pointwise value is infinite."""
    n = pointwise.size
    if n < 2:
        return 0.0
    if not np.all(np.isfinite(pointwise)):
        return math.inf
    return float(np.std(pointwise, ddof=1) / math.sqrt(n))


def calibration_table(proba, outcome, bins: int = 10) -> Dict[str, np.ndarray]:
    """Reliability table of forecasts `proba` [n, 3] against `outcome` [n], per class (rows: home win,
    draw, away win) over `bins` equal-width bins of [0, 1], bin b = [edge_b, edge_b+1) and the last one
    closed at 1: "bin_edges" [bins+1], "count" int64 [3, bins], "mean_proba" (the mean forecast of the
    class in the bin) and "observed" (how often the class then happened) [3, bins]; an empty bin holds
    count 0 and NaN in the other two."""
    p = np.asarray(proba, dtype=np.float64)
    o = np.asarray(outcome, dtype=np.int64)
    edges = np.linspace(0.0, 1.0, bins + 1)
    count = np.zeros((3, bins), dtype=np.int64)
    mean_proba = np.full((3, bins), np.nan)
    observed = np.full((3, bins), np.nan)
    for k in range(3):
        b = np.clip(np.searchsorted(edges, p[:, k], side="right") - 1, 0, bins - 1)
        count[k] = np.bincount(b, minlength=bins)
        some = count[k] > 0
        mean_proba[k, some] = np.bincount(b, weights=p[:, k], minlength=bins)[some] / count[k, some]
        observed[k, some] = np.bincount(b, weights=(o == k).astype(np.float64), minlength=bins)[some] / count[k, some]
    return {"bin_edges": edges, "count": count, "mean_proba": mean_proba, "observed": observed}


def pit_histogram(pit, bins: int = 10) -> np.ndarray:
    """Non-randomised probability integral transform histogram of count forecasts (Czado, Gneiting and Held
    2009) from `pit` [n, 2]: per fixture (lower, upper), the forecast distribution function just below and at
    the observed count (`loo_scores`' "pit_home" or "pit_away").  With F(u) the mean over the fixtures of
    clip((u - lower) / (upper - lower), 0, 1) -- the step 1[u >= lower] where upper == lower -- bin j of
    `bins` (1..1000) equal-width bins of [0, 1] holds F((j + 1) / bins) - F(j / bins): float64 [bins], summing
    to 1 when every upper <= 1 (mass beyond the forecast grid is missing otherwise).  A flat histogram means
    calibrated counts, a U shape under-dispersed forecasts, a hump over-dispersed ones."""
    p = np.asarray(pit, dtype=np.float64)
    bins = _count(bins, "bins", 1, SCORE_MAX_BINS)
    if p.ndim != 2 or p.shape[1] != 2 or p.shape[0] < 1:
        raise ValueError("pit must have shape [n, 2] with at least one fixture")
    if not np.all(np.isfinite(p)) or np.any(p[:, 1] < p[:, 0]):
        raise ValueError("pit must hold finite (lower, upper) pairs with lower <= upper")
    lower, width = p[:, :1], (p[:, 1] - p[:, 0])[:, None]
    u = np.linspace(0.0, 1.0, bins + 1)[None, :]
    flat = width == 0.0
    ramp = np.clip((u - lower) / np.where(flat, 1.0, width), 0.0, 1.0)
    F = np.where(flat, (u >= lower).astype(np.float64), ramp).mean(axis=0)
    return np.diff(F)


class ForecastScores:
    """`forecast_scores` for a predictor class.  Uses the class's PointwiseLikelihood interface:
    `_loglik_groups(data)` (host checks, team lookups, one device query per group) and `_loglik_draws()`."""

    def forecast_scores(self, data, max_goals: int = 15, bins: int = 10) -> Dict:
        """Ranked probability score, Brier score and log score of this model's win / draw / loss
        forecasts on the fixtures of `data` (the dict `log_likelihood` takes, at least one fixture; give
        it matches the fit did not see), with a reliability table.

        Per posterior draw and fixture the outcome probabilities are the triangle sums of max(tau, 0)
        Poisson Poisson over 0..max_goals (0..63), not renormalised; a fixture's forecast P is their mean
        over the draws: what `predict_outcome_proba(max_goals=...)` returns, in float64.  The observed
        class comes from the actual goals (0 home win, 1 draw, 2 away win; goals may exceed max_goals).
        For a triple p and observed class o: log = log p_o, brier = sum_k (p_k - 1[k = o])^2,
        rps = ((p_H - o_H)^2 + (p_H + p_D - o_H - o_D)^2) / 2.

        Returns a dict (float64 arrays unless said): "kind" = "scores", "n"; "outcome" uint8 [n];
        "outcome_proba" [n, 3], the forecasts P; "log_score_i", "brier_i", "rps_i" [n], the rules on P;
        "log_score", "brier", "rps", their means over the fixtures, and "log_score_se", "brier_se",
        "rps_se" = std(ddof=1) / sqrt(n) (0 for one fixture, inf if a pointwise value is infinite);
        "log_score_draws", "brier_draws", "rps_draws" [draws]: the mean over the fixtures of the rule
        applied to each draw's OWN probabilities -- the posterior distribution of the model's skill.
        The mean of these over the draws is NOT the score of the mean forecast (the rules are not
        linear in p; the forecast P scores better than the average draw).  "calibration": the
        reliability table of P (`calibration_table`, `bins` in 1..1000 equal-width bins).
        A class probability of zero gives -inf log scores; no result is NaN.  Every argument check
        runs on the host before any device call (ValueError)."""
        draws = self._loglik_draws()
        check_draws(draws)
        G = _count(max_goals, "max_goals", 0, SCORE_MAX_GOALS)
        bins = _count(bins, "bins", 1, SCORE_MAX_BINS)
        groups, n = self._loglik_groups(data)
        if n == 0:
            raise ValueError("forecast_scores needs at least one fixture")
        proba = np.empty((n, 3), dtype=np.float64)
        outcome = np.empty(n, dtype=np.uint8)
        draw_sums = np.zeros((draws, 3), dtype=np.float64)
        for positions, device, kw in groups:
            at = slice(None) if positions is None else positions
            part = device().outcome_scores(**kw, max_goals=G)
            proba[at] = part["proba"]
            outcome[at] = outcomes(kw["home_goals"], kw["away_goals"])
            draw_sums += part["draw_sums"]   # (group order; -inf stays -inf, nothing is +inf)
        out = {"kind": "scores", "n": n, "outcome": outcome, "outcome_proba": proba}
        on_mean = rules(proba, outcome)
        for k, name in enumerate(("log_score", "brier", "rps")):
            pointwise = on_mean[name]
            out[f"{name}_i"] = pointwise
            out[name] = float(np.mean(pointwise))
            out[f"{name}_se"] = _se_mean(pointwise)
            out[f"{name}_draws"] = draw_sums[:, k] / n
        out["calibration"] = calibration_table(proba, outcome, bins)
        return out


def compare_scores(results: Dict[str, Dict], rule: str = "rps") -> Dict[str, Dict]:
    """Rank `forecast_scores` results of several models on the SAME fixtures by `rule` ("rps", "brier":
    lower is better; "log_score": higher is better), best first.  Per model: "rank" (0 = best), "score"
    (the mean over the fixtures), "se", "diff" (to the best, >= 0 in the direction of worse) and
    "se_diff" = std(pointwise difference to the best, ddof=1) / sqrt(n) (0 for the best; inf when a
    pointwise score is infinite).  ValueError for no results, an unknown rule, results of another kind,
    different fixture counts or different "outcome" arrays (the fits were not scored on the same matches)."""
    if not results:
        raise ValueError("compare_scores needs at least one result")
    if rule not in RULES:
        raise ValueError(f"rule must be one of {RULES}, not {rule!r}")
    if any(not isinstance(r, dict) or r.get("kind") != "scores" for r in results.values()):
        raise ValueError("compare_scores takes forecast_scores() results")
    sizes = {name: int(r["n"]) for name, r in results.items()}
    if len(set(sizes.values())) != 1:
        raise ValueError(f"results have different fixture counts: {sizes}")
    first = np.asarray(next(iter(results.values()))["outcome"])
    if any(not np.array_equal(np.asarray(r["outcome"]), first) for r in results.values()):
        raise ValueError("results have different outcomes: the models were not scored on the same fixtures")
    sign = -1.0 if rule == "log_score" else 1.0   # sign * score: lower is better
    order = sorted(results, key=lambda name: sign * results[name][rule])
    best = results[order[0]]
    best_i = np.asarray(best[f"{rule}_i"], dtype=np.float64)
    out = {}
    for rank, name in enumerate(order):
        r = results[name]
        pointwise = np.asarray(r[f"{rule}_i"], dtype=np.float64)
        if rank == 0 or r[rule] == best[rule]:
            diff = 0.0
        else:
            diff = sign * (r[rule] - best[rule])
        if rank == 0:
            se_diff = 0.0
        elif not (np.all(np.isfinite(pointwise)) and np.all(np.isfinite(best_i))):
            se_diff = math.inf
        else:
            se_diff = _se_mean(pointwise - best_i)
        out[name] = {"rank": rank, "score": r[rule], "se": r[f"{rule}_se"], "diff": float(diff), "se_diff": se_diff}
    return out
