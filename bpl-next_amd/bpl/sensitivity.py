"""Power-scaling sensitivity: how much of each posterior quantity comes from the prior and how much from the
matches?  (Kallioinen, Paananen, Buerkner and Vehtari 2023; `priorsense` in R, `psens` in ArviZ; no reference
counterpart.)  The prior, or the likelihood, is raised to a power alpha slightly off 1; the existing draws are
re-weighted by the importance ratios (alpha - 1) * log density, Pareto smoothed as `psis_weights` smooths them,
and per quantity the distance between the weighted and the unweighted distribution of the draws is measured: the
symmetrised, normalised cumulative Jensen-Shannon distance `cjs`.  No refit.

`weighted_shift` is the generic half: any rows of log importance ratios, any draws.  Fed
`sequential_scores(return_weights=True)["log_weights"]` it says which quantities the later gameweeks moved.  The
sort, the weighted ECDF and the divergence run on the device, one workgroup per quantity
(csrc/dc_sensitivity.hip.h); the definitions are DESIGN.md section 33."""

from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np

from bpl.elpd import check_draws
from bpl.sequential import SEQ_MAX_BLOCKS

SHIFT_MAX_ROWS = 8          # include/bplhip.h BPLHIP_SHIFT_MAX_ROWS
SHIFT_MIN_DRAWS = 8
SHIFT_MAX_DRAWS = 65536     # include/bplhip.h BPLHIP_DIAG_MAX_DRAWS
THRESHOLD = 0.05            # priorsense's default
K_WARN = 0.7
ROWS = ("prior-", "prior+", "likelihood-", "likelihood+")
CONFLICT, DOMINATES = "prior-data conflict", "prior dominates"
_SHIFT_KEYS = ("cjs_sq", "mean", "sd")
_ROW_KEYS = ("log_weights", "pareto_k", "ess", "tail_len")

_context = None   # the HipContext of `_device_call`, created on first use
_backend = None   # callable(values [S, Q], log_ratios [R, S], r_eff, workspace_bytes) -> dict; None: the device


def _device_call(values, log_ratios, r_eff, workspace_bytes):
    global _context
    if _context is None:
        from bpl import _dist
        from bpl._ffi import HipContext

        _context = HipContext(_dist.local_device_index() if _dist.world()[1] > 1 else 0)
    return _context.weighted_shift(values, log_ratios, r_eff, workspace_bytes)


def _check_values(values):
    """float64 [S, Q] contiguous and the trailing shape; ValueError outside 8..65 536 draws."""
    v = np.asarray(values, dtype=np.float64)
    S = v.shape[0] if v.ndim else 0
    if S < SHIFT_MIN_DRAWS:
        raise ValueError(f"{S} draws; the shift needs at least {SHIFT_MIN_DRAWS}")
    if S > SHIFT_MAX_DRAWS:
        raise ValueError(f"{S} draws, at most {SHIFT_MAX_DRAWS}")
    return np.ascontiguousarray(v.reshape(S, -1)), v.shape[1:]


def _check_row(row, S: int, name: str) -> np.ndarray:
    try:
        r = np.asarray(row, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{name} must be numbers") from e
    if r.shape != (S,):
        raise ValueError(f"{name} has shape {r.shape}, not one value per draw ({S},)")
    if not np.all(np.isfinite(r)):
        raise ValueError(f"{name} has a non-finite value")
    return r


def weighted_shift(values, log_ratios, r_eff: float = 1.0, workspace_bytes: Optional[int] = None) -> Dict:
    """How far every quantity of `values`, float64 [S, ...] (every trailing entry is one scalar quantity), moves
    under each row of `log_ratios`, float64 [rows, S] (or [S]: one row), all finite, at most 8 rows.

    The rows are Pareto smoothed and normalised as `psis_weights` does it (tail size from `r_eff`).  Returns
    "cjs_sq", "cjs" = sqrt(cjs_sq), and the weighted "mean" and "sd", each [rows, ...]; and for the rows
    "log_weights" [rows, S], "pareto_k", "ess" [rows], "tail_len" int32 [rows].  A quantity with a non-finite
    draw, or whose draws are all equal, has NaN in cjs_sq and cjs; mean and sd are still formed.
    `workspace_bytes` caps the device memory of the sort beyond 12 288 draws (None: the library's default).

    ValueError, on the host before any device call: fewer than 8 or more than 65 536 draws, no row or more than
    8, a row whose length is not the number of draws, a non-finite ratio, a bad `r_eff`."""
    v, trailing = _check_values(values)
    S = v.shape[0]
    r = np.asarray(log_ratios, dtype=np.float64)
    if r.ndim == 1:
        r = r[None, :]
    if r.ndim != 2 or not 1 <= r.shape[0] <= SHIFT_MAX_ROWS:
        raise ValueError(f"log_ratios must be [rows, draws] with 1 to {SHIFT_MAX_ROWS} rows")
    r = np.ascontiguousarray(np.stack([_check_row(row, S, f"log_ratios[{i}]") for i, row in enumerate(r)]))
    if r_eff is None:
        raise ValueError("r_eff must be a number")
    check_draws(S, r_eff)
    ws = 0 if workspace_bytes is None else int(workspace_bytes)
    empty = v.shape[1] == 0
    raw = (_backend or _device_call)(np.zeros((S, 1)) if empty else v, r, float(r_eff), ws)
    out = {}
    for nm in _SHIFT_KEYS:
        a = np.asarray(raw[nm], dtype=np.float64)
        out[nm] = a[:, :0].reshape((r.shape[0],) + trailing) if empty else a.reshape((r.shape[0],) + trailing)
    with np.errstate(invalid="ignore"):
        out["cjs"] = np.sqrt(out["cjs_sq"])
    for nm in _ROW_KEYS:
        out[nm] = np.asarray(raw[nm])
    return out


def diagnose(prior, likelihood, threshold: float = THRESHOLD) -> np.ndarray:
    """The diagnosis strings of sensitivities (arrays of one shape): "prior-data conflict" where both reach
    `threshold`, "prior dominates" where the prior alone does, "" elsewhere (a NaN prior sensitivity included)."""
    p, l = np.asarray(prior, dtype=np.float64), np.asarray(likelihood, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        hot = p >= threshold
        both = hot & (l >= threshold)
    out = np.full(p.shape, "", dtype=f"<U{len(CONFLICT)}")
    out[hot] = DOMINATES
    out[both] = CONFLICT
    return out


def powerscale_sensitivity(values, log_prior, log_likelihood, delta: float = 0.01, r_eff: float = 1.0,
                           threshold: float = THRESHOLD, workspace_bytes: Optional[int] = None) -> Dict:
    """Prior and likelihood sensitivity of every quantity of `values`, float64 [S, ...], given the per-draw log
    densities `log_prior` and `log_likelihood` [S] of the two components.

    With alpha- = 1 / (1 + delta) and alpha+ = 1 + delta the four rows of log ratios (alpha - 1) * log density --
    prior-, prior+, likelihood-, likelihood+ -- go through `weighted_shift`, and
    sensitivity_c = (cjs_c- + cjs_c+) / (2 log2(1 + delta)).  Returns "prior" and "likelihood" (the trailing
    shape of `values`), "diagnosis" (an array of str: "prior-data conflict" where both reach `threshold`, "prior
    dominates" where the prior alone does, else ""), "cjs", "mean", "sd" [4, ...], "pareto_k", "ess" [4], "alpha"
    [2], "delta", "threshold" and "warnings" (one line per row with pareto_k > 0.7: its numbers are returned all
    the same).

    ValueError on the host: delta <= 0, a non-finite log density or one whose length is not the number of draws,
    fewer than 8 or more than 65 536 draws."""
    v, trailing = _check_values(values)
    S = v.shape[0]
    if isinstance(delta, (bool, np.bool_)) or not isinstance(delta, (int, float, np.integer, np.floating)) \
            or not (math.isfinite(float(delta)) and float(delta) > 0.0):
        raise ValueError(f"delta = {delta!r} must be a finite number > 0")
    if isinstance(threshold, (bool, np.bool_)) or not isinstance(threshold, (int, float, np.integer, np.floating)) \
            or math.isnan(float(threshold)):
        raise ValueError(f"threshold = {threshold!r} must be a number")
    delta = float(delta)
    lp = _check_row(log_prior, S, "log_prior")
    ll = _check_row(log_likelihood, S, "log_likelihood")
    lo, hi = 1.0 / (1.0 + delta), 1.0 + delta
    with np.errstate(over="ignore"):
        ratios = np.stack([(lo - 1.0) * lp, (hi - 1.0) * lp, (lo - 1.0) * ll, (hi - 1.0) * ll])
    if not np.all(np.isfinite(ratios)):
        raise ValueError("a log ratio (alpha - 1) * log density is not finite")
    w = weighted_shift(v, ratios, r_eff, workspace_bytes)
    cjs = w["cjs"].reshape((4,) + trailing)
    scale = 2.0 * math.log2(1.0 + delta)
    out = {"prior": (cjs[0] + cjs[1]) / scale, "likelihood": (cjs[2] + cjs[3]) / scale, "cjs": cjs,
           "mean": w["mean"].reshape((4,) + trailing), "sd": w["sd"].reshape((4,) + trailing),
           "pareto_k": w["pareto_k"], "ess": w["ess"], "alpha": np.array([lo, hi]), "delta": delta,
           "threshold": float(threshold)}
    out["diagnosis"] = diagnose(out["prior"], out["likelihood"], float(threshold))
    out["warnings"] = [f"{ROWS[i]} (alpha = {(lo, hi)[i & 1]:.6g}): pareto_k = {k:.3f} > {K_WARN}, the re-weighted "
                       f"draws are unreliable" for i, k in enumerate(w["pareto_k"]) if k > K_WARN]
    return out


def log_jacobian(sites, z) -> np.ndarray:
    """log |d constrained / d unconstrained| per draw of z [S, D], over the latent sites (name, size or shape) in
    flat order: z for an Exp site (`std_*`), -softplus(z) - softplus(-z) for a Sigmoid site (`corr_coef_raw`,
    `u`); every other site is unconstrained."""
    z = np.asarray(z, dtype=np.float64)
    out = np.zeros(z.shape[0], dtype=np.float64)
    at = 0
    for name, shape in sites:
        size = int(np.prod(shape))
        block = z[:, at:at + size]
        if name.startswith("std_"):
            out += block.sum(axis=1)
        elif name in ("corr_coef_raw", "u"):
            out -= (np.logaddexp(0.0, block) + np.logaddexp(0.0, -block)).sum(axis=1)
        at += size
    return out


class PowerscaleSensitivity:
    """`prior_sensitivity` for a predictor class.  Uses the class's McmcDiagnostics interface (`_diagnostic_arrays`,
    `_latent_sites`), its PointwiseLikelihood interface (`_loglik_groups`, `_loglik_draws`) and `_fit_weights`."""

    def _fit_weights(self, data) -> Optional[np.ndarray]:
        """The likelihood weights the fit's own keywords give on the fixtures of `data` (None: unweighted)."""
        return None

    def _loglik_draw_sums(self, data, weights) -> np.ndarray:
        """log_likelihood[s] = sum_i w_i ll_i[s], float64 [draws], without the [draws, fixtures] matrix: the
        fixtures are grouped by their distinct weight, `block_loglik` sums each group per draw (at most
        SEQ_MAX_BLOCKS - 1 weights per call, the rest of the fixtures parked in one block that is not read), and
        the sums are combined here in float64 in ascending order of the weight.  `weights`: None or [n]."""
        groups, n = self._loglik_groups(data)
        draws = self._loglik_draws()
        check_draws(draws)
        if weights is None:
            w = np.ones(n, dtype=np.float64)
        else:
            w = np.asarray(weights, dtype=np.float64)
            if w.shape != (n,) or not np.all(np.isfinite(w)):
                raise ValueError(f"weights must be {n} finite numbers, one per fixture")
        values, index = np.unique(w, return_inverse=True)
        index = index.reshape(n)
        total = np.zeros(draws, dtype=np.float64)
        step = SEQ_MAX_BLOCKS - 1
        for b0 in range(0, values.size, step):
            B = min(step, values.size - b0)
            local = index - b0
            idx32 = np.where((local >= 0) & (local < B), local, B).astype(np.int32)
            sums = np.zeros((B + 1, draws), dtype=np.float64)
            for positions, device, kw in groups:   # (group order)
                at = slice(None) if positions is None else positions
                sums += device().block_loglik(**kw, block_idx=idx32[at], n_blocks=B + 1)
            for b in range(B):
                if values[b0 + b] != 0.0:   # (a weight of 0 takes its fixtures out, whatever their likelihood)
                    total += values[b0 + b] * sums[b]
        return total

    def prior_sensitivity(self, data, weights=None, space: str = "constrained", delta: float = 0.01,
                          r_eff: float = 1.0, threshold: float = THRESHOLD) -> Dict:
        """Power-scaling sensitivity of the fitted model: per posterior quantity, how far it moves when the prior,
        or the likelihood, is raised to a power slightly off 1 (`bpl.powerscale_sensitivity`).

        `data` is the training data, as for `loo`.  The likelihood component is log_likelihood[s] = sum_i w_i
        ll_i[s] with ll the values of `log_likelihood(data)` and w the weights of the fit: `weights=None` takes
        the weights the fit's own keywords (time decay, game weights) give on `data`, an explicit [n] array
        overrides them.  The prior component is split off the sampler's own log joint,
        log_prior[s] = -potential_energy[s] - log_likelihood[s] - logJ[s], with logJ the log-Jacobian of the
        unconstraining transforms on `mcmc_info_["unconstrained"]`, so no class states its priors twice.
        `potential_energy` is the sampler kernel's value, which stays within 1e-3 of the float64 statement of
        the model: the log ratios carry at most delta * 1e-3 of that.  `space` picks the quantities as in
        `mcmc_diagnostics`.

        Returns {site: {"prior", "likelihood", "diagnosis"}} (arrays of the site's trailing shape) plus "pareto_k",
        "ess" [4] (prior-, prior+, likelihood-, likelihood+), "warnings", "log_prior", "log_likelihood" [draws],
        "delta" and "threshold".

        ValueError: `mcmc_info_` lacks "unconstrained" or "potential_energy" (a hand-built posterior: give the
        two log densities to `bpl.powerscale_sensitivity` yourself); the latent sites do not match the draws (after
        `add_new_team`, say); some log_likelihood[s] is not finite."""
        info = getattr(self, "mcmc_info_", None)
        if not info or info.get("unconstrained") is None or info.get("potential_energy") is None:
            raise ValueError("prior_sensitivity needs mcmc_info_['unconstrained'] and ['potential_energy'], which "
                             "fit() keeps; for a hand-built posterior give log_prior and log_likelihood to "
                             "bpl.powerscale_sensitivity")
        self._diagnostic_arrays("unconstrained")   # (ValueError unless the latent sites match the draws)
        z = np.asarray(info["unconstrained"], dtype=np.float64)
        sites = self._diagnostic_arrays(space)
        energy = np.asarray(info["potential_energy"], dtype=np.float64).reshape(-1)
        S = z.shape[0]
        if energy.shape != (S,) or any(a.shape[0] != S for a in sites.values()):
            raise ValueError(f"the posterior arrays and potential_energy disagree with the {S} unconstrained draws")
        ll = self._loglik_draw_sums(data, self._fit_weights(data) if weights is None else weights)
        if ll.shape != (S,) or not np.all(np.isfinite(ll)):
            raise ValueError("log_likelihood is not finite for every draw (a clipped tau on a training fixture?)")
        lp = -energy - ll - log_jacobian(self._latent_sites(), z)
        flat = np.concatenate([a.reshape(S, -1) for a in sites.values()], axis=1)
        res = powerscale_sensitivity(flat, lp, ll, delta, r_eff, threshold)
        out, at = {}, 0
        for name, a in sites.items():
            size = int(np.prod(a.shape[1:]))
            out[name] = {nm: res[nm][at:at + size].reshape(a.shape[1:]) for nm in ("prior", "likelihood", "diagnosis")}
            at += size
        out.update({nm: res[nm] for nm in ("pareto_k", "ess", "warnings", "delta", "threshold")})
        out.update(log_prior=lp, log_likelihood=ll)
        return out


def format_summary(result: Dict, worst: int = 10) -> str:
    """A text table of the `worst` quantities by prior sensitivity of a predictor's `prior_sensitivity()` result
    (NaN last), then the rows' Pareto k and effective sample sizes and the warnings."""
    rows = []
    for site, st in result.items():
        if not isinstance(st, dict) or "prior" not in st:
            continue
        prior = np.asarray(st["prior"])
        for index in np.ndindex(prior.shape):
            label = site + ("[" + ",".join(str(i) for i in index) + "]" if index else "")
            rows.append((label, float(prior[index]), float(np.asarray(st["likelihood"])[index]),
                         str(np.asarray(st["diagnosis"])[index])))
    order = sorted(rows, key=lambda r: (np.isnan(r[1]), -r[1] if not np.isnan(r[1]) else 0.0))[:max(int(worst), 0)]
    width = max([len(r[0]) for r in order] + [8])
    lines = [f"{'quantity':<{width}} {'prior':>10} {'likelihood':>10}  diagnosis"]
    for r in order:
        lines.append(f"{r[0]:<{width}} {r[1]:>10.4g} {r[2]:>10.4g}  {r[3]}".rstrip())
    flagged = sum(1 for r in rows if r[3])
    lines.append(f"{len(rows)} quantities; {flagged} at or above the threshold {result.get('threshold', THRESHOLD):.4g}")
    if "pareto_k" in result:
        lines.append("pareto_k: " + ", ".join(f"{nm} {k:.3f}" for nm, k in zip(ROWS, np.asarray(result["pareto_k"])))
                     + "; ess: " + ", ".join(f"{e:.0f}" for e in np.asarray(result["ess"])))
    lines += [f"warning: {w}" for w in result.get("warnings", [])]
    return "\n".join(lines)
