"""Model checking and comparison: pointwise log-likelihood, WAIC and PSIS-LOO of a fitted model on
held-in or held-out fixtures, and `compare_elpd` to rank several fits (no reference counterpart: the
reference leaves this to numpyro.infer.log_likelihood and ArviZ, which this package does not use).

ll[s, n] = log p(y_n | theta_s) includes the Dixon-Coles tau term (the reference adds tau through
numpyro.factor, so numpyro's log_likelihood would leave it out) and is UNWEIGHTED: time decay and game
weights shape the fit, not the pointwise likelihood (as numpyro's log_likelihood).  The device kernels
are csrc/dc_loglik.hip.h; WAIC uses the per-fixture lppd and variance, PSIS-LOO its elpd_loo and Pareto
k (definition: DESIGN.md section 12).  r_eff (relative efficiency of the draws) is an argument,
default 1, not estimated per chain.
"""

from __future__ import annotations

import math
from typing import Dict

import numpy as np

LOGLIK_MAX_DRAWS = 65536   # include/bplhip.h BPLHIP_LOGLIK_MAX_DRAWS
LOGLIK_MAX_TAIL = 1024     # include/bplhip.h BPLHIP_LOGLIK_MAX_TAIL
MAX_GOALS_DATA = 255


def tail_size(draws: int, r_eff: float) -> int:
    """PSIS tail length M = min(ceil(min(0.2 S, 3 sqrt(S / r_eff))), S - 1)."""
    return min(int(math.ceil(min(0.2 * draws, 3 * math.sqrt(draws / r_eff)))), draws - 1)


def check_draws(draws: int, r_eff=None) -> None:
    """The device limits, checked on the host: ValueError before any device call."""
    if draws > LOGLIK_MAX_DRAWS:
        raise ValueError(f"{draws} posterior draws: the log-likelihood path takes at most {LOGLIK_MAX_DRAWS}")
    if r_eff is None:
        return
    if isinstance(r_eff, (bool, np.bool_)) or not isinstance(r_eff, (int, float, np.integer, np.floating)):
        raise ValueError("r_eff must be a number")
    r = float(r_eff)
    if not (math.isfinite(r) and r > 0):
        raise ValueError(f"r_eff = {r_eff} must be finite and > 0")
    m = tail_size(draws, r)
    if m > LOGLIK_MAX_TAIL:
        raise ValueError(f"the PSIS tail of {m} draws (draws = {draws}, r_eff = {r}) exceeds {LOGLIK_MAX_TAIL}; "
                         "raise r_eff or use fewer draws")


def fixture_count(data, keys) -> int:
    """Length shared by data[k] for k in keys; ValueError if they differ or a key is missing."""
    lengths = {}
    for k in keys:
        if k not in data:
            raise ValueError(f"data has no {k!r}")
        v = data[k]
        lengths[k] = 1 if isinstance(v, str) else len(list(v) if not hasattr(v, "__len__") else v)
    if len(set(lengths.values())) > 1:
        raise ValueError(f"data columns have unequal lengths: {lengths}")
    return next(iter(lengths.values())) if lengths else 0


def goals(values, n: int) -> np.ndarray:
    """Integer goal counts in 0..255 as uint16 (ValueError otherwise)."""
    g = np.asarray(list(values) if not isinstance(values, np.ndarray) else values)
    if g.shape != (n,):
        raise ValueError("goals must be one value per fixture")
    if n and (g.dtype.kind not in "iuf" or not np.all(np.isfinite(g)) or not np.all(g == np.round(g))):
        raise ValueError("goals must be integers")
    if n and (g.min() < 0 or g.max() > MAX_GOALS_DATA):
        raise ValueError(f"goals must be in 0..{MAX_GOALS_DATA}")
    return g.astype(np.uint16)


def lookup(values, table: Dict, n: int, what: str = "team") -> np.ndarray:
    """Names (or ready indices below len(table)) -> uint16 indices; ValueError for an unknown one."""
    items = [values] if isinstance(values, str) else list(values)
    if len(items) != n:
        raise ValueError(f"{what} column must have one value per fixture")
    out = np.empty(n, dtype=np.uint16)
    for i, v in enumerate(items):
        if isinstance(v, (str, np.str_)):
            if v not in table:
                raise ValueError(f"unknown {what} {v!r}")
            out[i] = table[v]
        elif isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) and 0 <= int(v) < len(table):
            out[i] = int(v)
        else:
            raise ValueError(f"unknown {what} {v!r}")
    return out


def venue(values, n: int) -> np.ndarray:
    nv = np.asarray(list(values) if not isinstance(values, np.ndarray) else values)
    if nv.shape != (n,):
        raise ValueError("neutral_venue must be one value per fixture")
    if n and not np.all((nv == 0) | (nv == 1)):
        raise ValueError("neutral_venue must be 0 or 1")
    return nv.astype(np.uint8)


def _se(pointwise: np.ndarray) -> float:
    """sqrt(n) std(pointwise, ddof=1); 0 for one fixture, inf when a pointwise value is infinite."""
    n = pointwise.size
    if n < 2:
        return 0.0
    if not np.all(np.isfinite(pointwise)):
        return math.inf
    return float(math.sqrt(n) * np.std(pointwise, ddof=1))


class PointwiseLikelihood:
    """`log_likelihood`, `waic` and `loo` for a predictor class.  The class says how `data` becomes
    device queries (`_loglik_groups`: host checks, team lookups) and how many draws it has."""

    def _loglik_draws(self) -> int:
        return int(np.shape(self.corr_coef)[0])

    def _fixture_groups(self, data, with_goals: bool):
        """[(positions, device, kwargs)]: the fixtures at `positions` (an index array, or None for all)
        go to `device()` (a HipContext with the right posterior uploaded) with the query keyword
        arguments `kwargs` (with the actual goals, checked like the rest, when `with_goals`; without,
        data's goal columns are not looked at); and the number of fixtures."""
        raise NotImplementedError

    def _loglik_groups(self, data):
        """`_fixture_groups` with the actual goals: loglik_* keyword arguments."""
        return self._fixture_groups(data, with_goals=True)

    def _loglik_run(self, data, method: str, **extra):
        groups, n = self._loglik_groups(data)
        results = []
        for positions, device, kwargs in groups:
            results.append((positions, getattr(device(), method)(**kwargs, **extra)))
        return results, n

    def log_likelihood(self, data) -> np.ndarray:
        """ll[draw, fixture] = log p(home_goals, away_goals | draw), float64 [draws, fixtures], for the
        fixtures of `data` (a dict with the keys `fit` reads per fixture; others are ignored).  Includes
        the Dixon-Coles tau term; unweighted (fit-time time decay and game weights play no part)."""
        check_draws(self._loglik_draws())
        results, n = self._loglik_run(data, "loglik_matrix")
        out = np.empty((self._loglik_draws(), n), dtype=np.float64)
        for positions, ll in results:
            out[:, slice(None) if positions is None else positions] = ll
        return out

    def _loglik_summary(self, data, psis: bool, r_eff=None) -> Dict[str, np.ndarray]:
        check_draws(self._loglik_draws(), r_eff if psis else None)
        extra = {"psis": psis}
        if psis:
            extra["r_eff"] = float(r_eff)
        results, n = self._loglik_run(data, "loglik_summary", **extra)
        keys = ("lppd", "mean", "var") + (("elpd_loo", "pareto_k", "tail_len") if psis else ())
        out = {k: np.empty(n, dtype=np.int32 if k == "tail_len" else np.float64) for k in keys}
        for positions, part in results:
            for k in keys:
                out[k][slice(None) if positions is None else positions] = part[k]
        return out

    def waic(self, data) -> Dict:
        """Widely applicable information criterion on the fixtures of `data`: elpd_waic = sum over
        fixtures of lppd_i - p_waic_i, with lppd_i = log mean_s exp(ll) and p_waic_i the variance of ll
        over the draws (1/(S-1)).  Returns "elpd_waic", "p_waic", "se" (sqrt(n) std(elpd_waic_i,
        ddof=1)), "waic" = -2 elpd_waic, pointwise "elpd_waic_i", "p_waic_i", "lppd_i", and "warning"
        (some p_waic_i > 0.4)."""
        r = self._loglik_summary(data, psis=False)
        elpd_i = r["lppd"] - r["var"]
        elpd = float(np.sum(elpd_i))
        return {"kind": "waic", "n": elpd_i.size, "elpd_waic": elpd, "p_waic": float(np.sum(r["var"])),
                "se": _se(elpd_i), "waic": -2.0 * elpd, "elpd_waic_i": elpd_i, "p_waic_i": r["var"],
                "lppd_i": r["lppd"], "warning": bool(np.any(r["var"] > 0.4))}

    def loo(self, data, r_eff: float = 1.0) -> Dict:
        """Pareto-smoothed importance-sampling leave-one-out cross-validation on the fixtures of
        `data`.  r_eff: relative efficiency of the draws (default 1; not
        estimated per chain).  Returns "elpd_loo", "p_loo" = sum lppd_i - elpd_loo, "se", "looic" =
        -2 elpd_loo, pointwise "elpd_loo_i", "pareto_k", "lppd_i", and "warning" (some k > 0.7)."""
        r = self._loglik_summary(data, psis=True, r_eff=r_eff)
        elpd_i = r["elpd_loo"]
        elpd = float(np.sum(elpd_i))
        return {"kind": "loo", "n": elpd_i.size, "elpd_loo": elpd, "p_loo": float(np.sum(r["lppd"]) - elpd),
                "se": _se(elpd_i), "looic": -2.0 * elpd, "elpd_loo_i": elpd_i, "pareto_k": r["pareto_k"],
                "lppd_i": r["lppd"], "warning": bool(np.any(r["pareto_k"] > 0.7))}


def compare_elpd(results: Dict[str, Dict]) -> Dict[str, Dict]:
    """Rank `loo` (or `waic`) results of several models on the SAME fixtures, best first.  Per
    model: "rank" (0 = best), "elpd", "p", "se", "elpd_diff" (best's elpd minus this one's, >= 0)
    and "se_diff" = sqrt(n) std(pointwise difference to the best, ddof=1) (0 for the best),
    "warning".  ValueError for mixed kinds or different fixture counts."""
    if not results:
        raise ValueError("compare_elpd needs at least one result")
    kinds = {r.get("kind") for r in results.values()}
    if len(kinds) != 1 or not kinds <= {"loo", "waic"}:
        raise ValueError("compare_elpd takes results of one kind: all loo() or all waic()")
    kind = kinds.pop()
    sizes = {name: np.asarray(r[f"elpd_{kind}_i"]).size for name, r in results.items()}
    if len(set(sizes.values())) != 1:
        raise ValueError(f"results have different fixture counts: {sizes}")
    order = sorted(results, key=lambda name: -results[name][f"elpd_{kind}"])
    best = np.asarray(results[order[0]][f"elpd_{kind}_i"], dtype=np.float64)
    out = {}
    for rank, name in enumerate(order):
        r = results[name]
        diff = best - np.asarray(r[f"elpd_{kind}_i"], dtype=np.float64)
        out[name] = {"rank": rank, "elpd": r[f"elpd_{kind}"], "p": r[f"p_{kind}"], "se": r["se"],
                     "elpd_diff": results[order[0]][f"elpd_{kind}"] - r[f"elpd_{kind}"],
                     "se_diff": 0.0 if rank == 0 else _se(diff), "warning": r["warning"]}
    return out
