"""Sequential forecasts: what a fitted model predicts for gameweek g once the results of the gameweeks before
g are taken into account WITHOUT a refit, and from which gameweek on the old fit is too stale for that (no
reference counterpart).  This is Pareto-smoothed importance-sampling leave-future-out cross-validation
(Buerkner, Gabry and Vehtari 2020): the posterior draws are re-weighted by the likelihood of the results seen
since the fit, and the Pareto k of each step is the refit signal.  `forecast_scores` scores the frozen
forecast; `loo` leaves one fixture out of the data the fit saw.

The device kernels are csrc/dc_sequential.hip.h (definition: DESIGN.md section 17): per-draw sums of the
log-likelihood over blocks of fixtures, PSIS over the draws of their running sums, and weighted reductions
over the draws.  The only reduction left on the host is the O(blocks x draws) running sum."""

from __future__ import annotations

import math
from typing import Dict, Tuple

import numpy as np

from bpl.elpd import check_draws
from bpl.scoring import SCORE_MAX_GOALS, _count, _se_mean, outcomes, rules

SEQ_MAX_BLOCKS = 4096   # include/bplhip.h BPLHIP_SEQ_MAX_BLOCKS


def relabel_blocks(block, n: int) -> Tuple[np.ndarray, np.ndarray]:
    """(block_values [B], index int64 [n]): the distinct values of `block` in ascending order and each
    fixture's position among them.  ValueError unless `block` holds one integer per fixture (integer-valued
    floats pass) and at most SEQ_MAX_BLOCKS distinct values."""
    b = np.asarray(list(block) if not isinstance(block, np.ndarray) else block)
    if b.shape != (n,):
        raise ValueError("block must have one value per fixture")
    if b.dtype.kind == "f":
        if not (np.all(np.isfinite(b)) and np.all(b == np.round(b)) and np.all(np.abs(b) < 2.0 ** 53)):
            raise ValueError("block must be integers")
    elif b.dtype.kind not in "iu":
        raise ValueError("block must be integers")
    values, index = np.unique(b.astype(np.int64), return_inverse=True)
    if values.size > SEQ_MAX_BLOCKS:
        raise ValueError(f"{values.size} blocks: sequential_scores takes at most {SEQ_MAX_BLOCKS}")
    return values, index.reshape(n).astype(np.int64)


def log_ratios(block_sums: np.ndarray) -> np.ndarray:
    """R[b, s] = the sum of A[b', s] over b' < b (R[0, .] = 0): block b is forecast with the results of the
    blocks before it.  -inf (a clipped tau) stays -inf; nothing is +inf, so nothing becomes NaN."""
    a = np.asarray(block_sums, dtype=np.float64)
    r = np.zeros_like(a)
    np.cumsum(a[:-1], axis=0, out=r[1:])
    return r


def _finite_number(value, name: str) -> float:
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name} must be a number")
    if not math.isfinite(float(value)):
        raise ValueError(f"{name} = {value} must be finite")
    return float(value)


def _block_means(pointwise: np.ndarray, index: np.ndarray, n_block: np.ndarray) -> np.ndarray:
    """Mean of `pointwise` over each block's fixtures (-inf stays -inf: nothing here is +inf)."""
    out = np.zeros(n_block.size, dtype=np.float64)
    np.add.at(out, index, pointwise)
    return out / n_block


class SequentialScores:
    """`sequential_scores` for a predictor class.  Uses the class's PointwiseLikelihood interface:
    `_loglik_groups(data)` (host checks, team lookups, one device query per group) and `_loglik_draws()`."""

    def sequential_scores(self, data, block, r_eff: float = 1.0, max_goals: int = 15, k_threshold: float = 0.7,
                          return_weights: bool = False) -> Dict:
        """Forecasts of the fixtures of `data` (the dict `log_likelihood` takes, at least one fixture), each
        made with the posterior re-weighted by the results of the EARLIER blocks, and the gameweek from
        which a refit is needed.  `block`: one integer per fixture (the gameweek, say); the distinct values
        in ascending order are the blocks 0..B-1 (at most 4096); the fixtures need be neither sorted nor
        contiguous.

        With ll the values of `log_likelihood` (unweighted, tau included): A[b, s] = sum of ll[s, n] over
        the fixtures of block b; R[b, s] = sum of A[b', s] over b' < b; R[b, .] is Pareto smoothed over the
        draws as `loo` smooths -ll (tail size from `r_eff`) and normalised to log weights lw[b, .].  Equal
        ratios (block 0, or one draw) give uniform weights with k = 0; a block whose every draw is ruled
        out by an earlier clipped tau is dead: k = +inf, ess = 0, elpd_i = -inf, probabilities 0.  Per
        fixture n of block b: elpd_i = lse_s(lw[b, s] + ll[s, n]) and the forecast P = sum_s exp(lw[b, s])
        p(s, n), p the per-draw outcome probabilities of `forecast_scores(max_goals=...)`.

        Returns a dict that `compare_scores` takes next to `forecast_scores(data)`: "kind" = "scores", "n",
        "outcome" uint8 [n], "outcome_proba" [n, 3]; "log_score_i", "brier_i", "rps_i" [n], their means
        "log_score", "brier", "rps" and "log_score_se", "brier_se", "rps_se"; "elpd_i" [n] and "elpd", its
        sum; "block" int64 [n], each fixture's block index, and "block_values" [B], the labels; per block
        [B]: "pareto_k", "ess" = exp(-lse(2 lw)), "tail_len" int32, "n_block", and the means over the
        block's fixtures "elpd_block", "rps_block", "brier_block", "log_score_block"; "reliable" [B] =
        (pareto_k <= k_threshold); "refit_from": the label of the first block with pareto_k > k_threshold,
        or None; with `return_weights` also "log_weights" [B, draws].  No result is NaN.  Every argument
        check runs on the host before any device call (ValueError)."""
        draws = self._loglik_draws()
        if r_eff is None:   # (check_draws reads None as "no PSIS")
            raise ValueError("r_eff must be a number")
        check_draws(draws, r_eff)
        G = _count(max_goals, "max_goals", 0, SCORE_MAX_GOALS)
        threshold = _finite_number(k_threshold, "k_threshold")
        groups, n = self._loglik_groups(data)
        if n == 0:
            raise ValueError("sequential_scores needs at least one fixture")
        values, index = relabel_blocks(block, n)
        B = values.size
        idx32 = index.astype(np.int32)
        sums = np.zeros((B, draws), dtype=np.float64)
        for positions, device, kw in groups:   # (group order; -inf stays -inf, nothing is +inf)
            at = slice(None) if positions is None else positions
            sums += device().block_loglik(**kw, block_idx=idx32[at], n_blocks=B)
        w = groups[0][1]().psis_weights(log_ratios(sums), float(r_eff))
        lw = w["log_weights"]
        proba = np.empty((n, 3), dtype=np.float64)
        elpd_i = np.empty(n, dtype=np.float64)
        outcome = np.empty(n, dtype=np.uint8)
        for positions, device, kw in groups:
            at = slice(None) if positions is None else positions
            part = device().weighted_scores(**kw, block_idx=idx32[at], log_weights=lw, max_goals=G)
            proba[at] = part["proba"]
            elpd_i[at] = part["elpd"]
            outcome[at] = outcomes(kw["home_goals"], kw["away_goals"])
        n_block = np.bincount(index, minlength=B).astype(np.int64)
        out = {"kind": "scores", "n": n, "outcome": outcome, "outcome_proba": proba}
        on_forecast = rules(proba, outcome)
        for name in ("log_score", "brier", "rps"):
            pointwise = on_forecast[name]
            out[f"{name}_i"] = pointwise
            out[name] = float(np.mean(pointwise))
            out[f"{name}_se"] = _se_mean(pointwise)
            out[f"{name}_block"] = _block_means(pointwise, index, n_block)
        k = w["pareto_k"]
        stale = np.nonzero(k > threshold)[0]
        out.update({"elpd_i": elpd_i, "elpd": float(np.sum(elpd_i)), "elpd_block": _block_means(elpd_i, index, n_block),
                    "block": index, "block_values": values, "n_block": n_block, "pareto_k": k, "ess": w["ess"],
                    "tail_len": w["tail_len"], "reliable": k <= threshold,
                    "refit_from": int(values[stale[0]]) if stale.size else None})
        if return_weights:
            out["log_weights"] = lw
        return out
