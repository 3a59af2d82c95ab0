"""MCMC convergence diagnostics: do the chains of a fit agree, and how many independent draws are they worth?
The rank-normalised split R-hat, the bulk / tail / mean effective sample sizes and the Monte Carlo standard error
of Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021), per scalar quantity (what numpyro's
`mcmc.print_summary()` gives the reference's users as `r_hat` and `n_eff`).

Per quantity, with C chains of N draws: every chain is split into its first and its last n = N // 2 draws (M = 2 C
chains, S = M n values).  `rhat` is the larger of the R-hats of the rank-normalised split draws and of the
rank-normalised |x - median|; `ess_bulk` is the effective sample size of the rank-normalised draws, `ess_tail` the
least one over the indicators x <= (a quantile), `ess_mean` that of the draws themselves and `mcse_mean` =
sd / sqrt(ess_mean).  Ranks, autocovariances and Geyer's truncation run on the device (csrc/dc_diagnostics.hip.h);
the definitions are DESIGN.md section 20."""

from __future__ import annotations

from typing import Dict, Optional

import numpy as np

DIAG_MAX_DRAWS = 65536      # include/bplhip.h BPLHIP_DIAG_MAX_DRAWS
DIAG_MAX_CHAINS = 256       # include/bplhip.h BPLHIP_DIAG_MAX_CHAINS
DIAG_MAX_QUANTILES = 16     # include/bplhip.h BPLHIP_DIAG_MAX_QUANTILES
STATISTICS = ("mean", "sd", "rhat", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean")
RHAT_WARN = 1.01
ESS_WARN_PER_CHAIN = 100.0

_context = None   # the HipContext of `_device_call`, created on first use
_backend = None   # callable(values [C N, Q], num_chains, quantiles, workspace_bytes) -> dict of [Q] arrays; None: the device


def _device_call(values, num_chains, quantiles, workspace_bytes):
    global _context
    if _context is None:
        from bpl import _dist
        from bpl._ffi import HipContext

        _context = HipContext(_dist.local_device_index() if _dist.world()[1] > 1 else 0)
    return _context.mcmc_diagnostics(values, num_chains, quantiles, workspace_bytes)


def _check(values, num_chains, quantiles):
    """The host checks: (float64 [C N, Q] contiguous, trailing shape, C, float64 quantiles)."""
    if isinstance(num_chains, (bool, np.bool_)) or int(num_chains) != num_chains or int(num_chains) < 1:
        raise ValueError(f"num_chains must be a positive integer, not {num_chains!r}")
    C = int(num_chains)
    v = np.asarray(values, dtype=np.float64)
    if v.ndim < 1 or v.shape[0] == 0 or v.shape[0] % C:
        raise ValueError(f"values has {v.shape[0] if v.ndim else 0} draws, not a multiple of num_chains={C}")
    if C > DIAG_MAX_CHAINS:
        raise ValueError(f"at most {DIAG_MAX_CHAINS} chains, not {C}")
    N = v.shape[0] // C
    if N < 8:
        raise ValueError(f"{N} draws per chain; the diagnostics need at least 8")
    S = 2 * C * (N // 2)
    if S > DIAG_MAX_DRAWS:
        raise ValueError(f"{S} split draws, at most {DIAG_MAX_DRAWS}")
    try:
        q = np.asarray(quantiles, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError("quantiles must be numbers") from e
    if q.ndim != 1 or q.size > DIAG_MAX_QUANTILES:
        raise ValueError(f"quantiles must be a sequence of at most {DIAG_MAX_QUANTILES} numbers")
    if not np.all((q > 0.0) & (q < 1.0)):
        raise ValueError("quantiles must lie strictly inside (0, 1)")
    trailing = v.shape[1:]
    return np.ascontiguousarray(v.reshape(v.shape[0], -1)), trailing, C, np.ascontiguousarray(q)


def mcmc_diagnostics(values, num_chains, quantiles=(0.05, 0.95), workspace_bytes=None) -> Dict[str, np.ndarray]:
    """Convergence diagnostics of `values`, float64 [num_chains * N, ...], chain-major (the order of every posterior
    array `fit` returns); every trailing entry is one scalar quantity.

    Returns a dict of float64 arrays of the trailing shape: "mean" and "sd" (ddof=1) over all draws, "rhat",
    "ess_bulk", "ess_tail" (the least over `quantiles`, each strictly inside (0, 1)), "ess_mean" and "mcse_mean".
    A quantity with a non-finite draw, or whose split draws are all equal, has NaN in everything but "mean" and
    "sd"; "rhat" is NaN when the within-chain variance is zero, an ess when its `var_plus` is zero.
    `workspace_bytes` caps the device memory beyond the draws (None: the library's default).

    ValueError, on the host before any device call: fewer than 8 draws per chain, more than 65 536 split draws,
    a number of draws that is no multiple of `num_chains`, more than 256 chains, a quantile outside (0, 1)."""
    v, trailing, C, q = _check(values, num_chains, quantiles)
    ws = 0 if workspace_bytes is None else int(workspace_bytes)
    if v.shape[1] == 0:
        return {nm: np.empty(trailing, dtype=np.float64) for nm in STATISTICS}
    raw = (_backend or _device_call)(v, C, q, ws)
    return {nm: np.asarray(raw[nm], dtype=np.float64).reshape(trailing) for nm in STATISTICS}


def split_draws(num_draws: int, num_chains: int) -> int:
    """S = 2 C (N // 2), the number of draws the effective sample sizes refer to."""
    return 2 * num_chains * ((num_draws // num_chains) // 2)


class McmcDiagnostics:
    """`mcmc_diagnostics` for a predictor class.  The class names its posterior arrays (`_DIAGNOSTIC_SITES`, attribute
    names; None entries are skipped) and its latent sites (`_latent_sites()`, (name, size or shape) in the flat
    order of `mcmc_info_["unconstrained"]`)."""

    _DIAGNOSTIC_SITES = ("attack", "defence", "home_advantage", "corr_coef")

    def _latent_sites(self):
        raise NotImplementedError

    def _diagnostic_arrays(self, space: str) -> Dict[str, np.ndarray]:
        info = getattr(self, "mcmc_info_", None)
        if space == "constrained":
            out = {}
            for name in self._DIAGNOSTIC_SITES:
                a = getattr(self, name, None)
                if a is not None:
                    out[name] = np.asarray(a, dtype=np.float64)
            if not out:
                raise ValueError("the model has no posterior draws: fit it first")
            return out
        if space != "unconstrained":
            raise ValueError(f"space must be 'constrained' or 'unconstrained', not {space!r}")
        if not info or info.get("unconstrained") is None:
            raise ValueError("the unconstrained draws are kept by fit() only (mcmc_info_ is missing)")
        z = np.asarray(info["unconstrained"], dtype=np.float64)
        sites = self._latent_sites()
        total = sum(int(np.prod(shape)) for _, shape in sites)
        if z.ndim != 2 or total != z.shape[1]:
            raise ValueError(f"the latent sites hold {total} entries, the unconstrained draws have shape {z.shape}")
        out, at = {}, 0
        for name, shape in sites:
            size = int(np.prod(shape))
            out[name] = z[:, at:at + size].reshape((z.shape[0],) + (shape if isinstance(shape, tuple) else (size,)))
            at += size
        return out

    def mcmc_diagnostics(self, space: str = "constrained", num_chains: Optional[int] = None,
                         quantiles=(0.05, 0.95)) -> Dict:
        """Convergence diagnostics of the fitted model (`bpl.mcmc_diagnostics` on every site).

        `space`: "constrained" diagnoses every posterior array the class keeps after `fit`; "unconstrained"
        diagnoses `mcmc_info_["unconstrained"]`, split by the class's latent sites.  `num_chains` defaults to
        `mcmc_info_["num_chains"]`; a hand-built posterior has no `mcmc_info_` and must give it (ValueError).

        Returns {site: {statistic: array of the site's trailing shape}} plus "sampler" (per chain: "divergences",
        "mean_accept_prob", "step_size" of the last draw; absent without `mcmc_info_`), "r_eff" (the mean over
        all diagnosed quantities of ess_mean / S, NaN entries left out: the scalar `loo(data, r_eff=...)` takes)
        and "warnings" (a list of strings: sites with rhat > 1.01, with ess_bulk or ess_tail below 100 per
        chain, and divergences)."""
        info = getattr(self, "mcmc_info_", None)
        if num_chains is None:
            if not info:
                raise ValueError("num_chains must be given for a posterior without mcmc_info_")
            num_chains = info["num_chains"]
        sites = self._diagnostic_arrays(space)
        draws = {a.shape[0] for a in sites.values()}
        if len(draws) != 1:
            raise ValueError(f"the posterior arrays disagree on the number of draws: {sorted(draws)}")
        S_all = draws.pop()
        flat = np.concatenate([a.reshape(S_all, -1) for a in sites.values()], axis=1)
        stats = mcmc_diagnostics(flat, num_chains, quantiles)
        out, at = {}, 0
        for name, a in sites.items():
            size = int(np.prod(a.shape[1:]))
            out[name] = {nm: stats[nm][at:at + size].reshape(a.shape[1:]) for nm in STATISTICS}
            at += size
        C = int(num_chains)
        S = split_draws(S_all, C)
        eff = stats["ess_mean"] / S
        out["r_eff"] = float(np.mean(eff[~np.isnan(eff)])) if np.any(~np.isnan(eff)) else float("nan")
        warn = site_warnings({k: out[k] for k in sites}, C)
        if info and info.get("diverging") is not None:
            kept = lambda key: np.asarray(info[key], dtype=np.float64).reshape(C, -1)
            out["sampler"] = {"divergences": kept("diverging").sum(axis=1).astype(np.int64),
                              "mean_accept_prob": kept("accept_prob").mean(axis=1),
                              "step_size": kept("step_size")[:, -1]}
            total = int(out["sampler"]["divergences"].sum())
            if total:
                warn.append(f"{total} divergent transitions (per chain: {out['sampler']['divergences'].tolist()})")
        out["warnings"] = warn
        return out


def site_warnings(sites: Dict[str, Dict[str, np.ndarray]], num_chains: int):
    """One line per site whose worst quantity misses a threshold (NaN entries do not count)."""
    warn = []
    floor = ESS_WARN_PER_CHAIN * num_chains
    with np.errstate(invalid="ignore"):
        for name, st in sites.items():
            rhat = np.asarray(st["rhat"])
            if np.any(rhat > RHAT_WARN):
                warn.append(f"{name}: rhat up to {np.nanmax(rhat):.3f} (> {RHAT_WARN}) in {int(np.sum(rhat > RHAT_WARN))} "
                            f"of {rhat.size} quantities")
            for key in ("ess_bulk", "ess_tail"):
                ess = np.asarray(st[key])
                if np.any(ess < floor):
                    warn.append(f"{name}: {key} down to {np.nanmin(ess):.0f} (< {ESS_WARN_PER_CHAIN:.0f} per chain) in "
                                f"{int(np.sum(ess < floor))} of {ess.size} quantities")
    return warn


def format_summary(result: Dict, worst: int = 10) -> str:
    """A text table of the `worst` quantities by rhat of a predictor's `mcmc_diagnostics()` result (NaN rhat last),
    then r_eff, the sampler's per-chain statistics and the warnings."""
    rows = []
    for site, st in result.items():
        if not isinstance(st, dict) or "rhat" not in st:
            continue
        rhat = np.asarray(st["rhat"])
        for index in np.ndindex(rhat.shape):
            label = site + ("[" + ",".join(str(i) for i in index) + "]" if index else "")
            rows.append((label,) + tuple(float(np.asarray(st[nm])[index]) for nm in STATISTICS))
    order = sorted(rows, key=lambda r: (np.isnan(r[3]), -r[3] if not np.isnan(r[3]) else 0.0))[:max(int(worst), 0)]
    width = max([len(r[0]) for r in order] + [8])
    lines = [f"{'quantity':<{width}} " + " ".join(f"{nm:>10}" for nm in STATISTICS)]
    for r in order:
        lines.append(f"{r[0]:<{width}} " + " ".join(f"{v:>10.4g}" for v in r[1:]))
    lines.append(f"{len(rows)} quantities; r_eff = {result.get('r_eff', float('nan')):.4g}")
    sampler = result.get("sampler")
    if sampler:
        lines.append("divergences per chain: " + str(np.asarray(sampler["divergences"]).tolist())
                     + "; mean accept_prob: " + ", ".join(f"{v:.3f}" for v in sampler["mean_accept_prob"])
                     + "; step size: " + ", ".join(f"{v:.4g}" for v in sampler["step_size"]))
    lines += [f"warning: {w}" for w in result.get("warnings", [])]
    return "\n".join(lines)
