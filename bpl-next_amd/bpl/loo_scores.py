"""Leave-one-out forecasts: what a fitted model would have predicted for each match it was fitted on, had the
fit not seen that match -- the predictive distribution behind `loo`, which returns only the log density of the
exact scoreline (no reference counterpart; in ArviZ terms this is loo_pit plus LOO-weighted forecasts).
`forecast_scores` on the fitted matches uses the full posterior and is optimistic; `sequential_scores` leaves
the future out; `posterior_predictive_check` replicates from the full posterior.

The device kernel is csrc/dc_loo.hip.h (definition: DESIGN.md section 32): one wave per fixture smooths that
fixture's own importance ratios exactly as `loo` does and applies the weights to the fixture's per-draw outcome
probabilities and goal-count distributions.  The [draws, fixtures] log-likelihood matrix is never stored.  The
rules, the standard errors and the reliability table are computed here, as in bpl/scoring.py."""

from __future__ import annotations

from typing import Dict

import numpy as np

from bpl.elpd import check_draws
from bpl.scoring import SCORE_MAX_BINS, SCORE_MAX_GOALS, _count, _se_mean, calibration_table, outcomes, rules
from bpl.sequential import _finite_number


class LooScores:
    """`loo_scores` for a predictor class.  Uses the class's PointwiseLikelihood interface:
    `_loglik_groups(data)` (host checks, team lookups, one device query per group) and `_loglik_draws()`."""

    def loo_scores(self, data, r_eff: float = 1.0, max_goals: int = 15, bins: int = 10,
                   k_threshold: float = 0.7) -> Dict:
        """Leave-one-out win / draw / loss forecasts, their proper scores and the probability integral
        transform (PIT) of the goal counts, on the fixtures of `data` (the dict `log_likelihood` takes, at least
        one fixture; usually the matches the model was fitted on).

        With ll the values of `log_likelihood`: per fixture i the ratios r_s = -ll[s, i] are Pareto smoothed
        over the draws exactly as `loo(data, r_eff)` smooths them (raw where nothing is smoothed: a tail of at
        most 4 draws or no usable fit, pareto_k = +inf) and normalised to weights w_s.  With p(s, i) the
        per-draw outcome probabilities and q the scoreline grid of `forecast_scores(max_goals=...)` (0..63, not
        renormalised): the leave-one-out forecast is sum_s w_s p(s, i); the in-sample forecast mean_s p(s, i)
        is what `forecast_scores` returns; pit_home = (lower, upper) with lower = sum_s w_s sum_{a < x} sum_b
        q(a, b) and upper the same with a <= x, x the actual home goals (a, b over 0..max_goals, so a count
        above max_goals gives lower = upper = the weighted grid mass); pit_away likewise on the away marginal.
        `bpl.scoring.pit_histogram` turns either into a histogram: flat means calibrated goal counts.  If some
        draw has ll = -inf (a clipped tau cell) the weights are the limit of the definition: uniform over
        those draws, zero elsewhere; elpd_loo_i = -inf, pareto_k = +inf, tail_len = 0, ess = their number.

        Returns a dict that `compare_scores` takes next to `forecast_scores(data)` (float64 arrays unless
        said): "kind" = "scores", "n", "outcome" uint8 [n]; "outcome_proba" [n, 3], the leave-one-out
        forecasts; "log_score_i", "brier_i", "rps_i" [n], the rules on them, their means "log_score", "brier",
        "rps" and "log_score_se", "brier_se", "rps_se"; "calibration", their reliability table
        (`calibration_table`, `bins` in 1..1000); "outcome_proba_in_sample" [n, 3] and "in_sample", a dict
        with the means "log_score", "brier", "rps" of the rules on it (the gap to the leave-one-out means is
        the optimism of scoring a fit on its own matches); "elpd_loo_i" [n] and "elpd_loo", its sum;
        "pareto_k", "ess" = 1 / sum_s w_s^2 [n], "tail_len" int32 [n]; "reliable" bool [n] = (pareto_k <=
        k_threshold) and "warning" (some fixture is not); "pit_home", "pit_away" [n, 2].  There are no per-draw
        scores: a single draw's skill has no leave-one-out meaning.  No result is NaN.  Every argument check
        runs on the host before any device call (ValueError)."""
        draws = self._loglik_draws()
        if r_eff is None:   # (check_draws reads None as "no PSIS")
            raise ValueError("r_eff must be a number")
        check_draws(draws, r_eff)
        G = _count(max_goals, "max_goals", 0, SCORE_MAX_GOALS)
        bins = _count(bins, "bins", 1, SCORE_MAX_BINS)
        threshold = _finite_number(k_threshold, "k_threshold")
        groups, n = self._loglik_groups(data)
        if n == 0:
            raise ValueError("loo_scores needs at least one fixture")
        shapes = {"proba": (n, 3), "proba_in_sample": (n, 3), "pit": (n, 4), "elpd_loo": (n,), "pareto_k": (n,),
                  "ess": (n,), "tail_len": (n,)}
        got = {k: np.empty(shape, dtype=np.int32 if k == "tail_len" else np.float64) for k, shape in shapes.items()}
        outcome = np.empty(n, dtype=np.uint8)
        for positions, device, kw in groups:
            at = slice(None) if positions is None else positions
            part = device().loo_scores(**kw, max_goals=G, r_eff=float(r_eff))
            for k in shapes:
                got[k][at] = part[k]
            outcome[at] = outcomes(kw["home_goals"], kw["away_goals"])
        proba = got["proba"]
        out = {"kind": "scores", "n": n, "outcome": outcome, "outcome_proba": proba}
        on_loo = rules(proba, outcome)
        for name in ("log_score", "brier", "rps"):
            pointwise = on_loo[name]
            out[f"{name}_i"] = pointwise
            out[name] = float(np.mean(pointwise))
            out[f"{name}_se"] = _se_mean(pointwise)
        out["calibration"] = calibration_table(proba, outcome, bins)
        on_fit = rules(got["proba_in_sample"], outcome)
        k = got["pareto_k"]
        reliable = k <= threshold
        out.update({"outcome_proba_in_sample": got["proba_in_sample"],
                    "in_sample": {name: float(np.mean(on_fit[name])) for name in ("log_score", "brier", "rps")},
                    "elpd_loo_i": got["elpd_loo"], "elpd_loo": float(np.sum(got["elpd_loo"])), "pareto_k": k,
                    "ess": got["ess"], "tail_len": got["tail_len"], "reliable": reliable,
                    "warning": bool(not np.all(reliable)),
                    "pit_home": np.ascontiguousarray(got["pit"][:, :2]),
                    "pit_away": np.ascontiguousarray(got["pit"][:, 2:])})
        return out
