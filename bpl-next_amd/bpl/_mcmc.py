"""The `NUTS(model)` + `MCMC(...).run(...)` + `get_samples()` sequence of the reference
(bpl/dixon_coles.py:100-122, bpl/extended_dixon_coles.py:293-331), driven through
libbplhip.so.  Host Python only orchestrates: fixture upload / broadcast, one
`bplhip_nuts_run` per chain, gather, and the constrained/deterministic site map.
"""

from __future__ import annotations

from typing import Any, Callable, Dict, Optional

import numpy as np

from bpl import _dist
from bpl._ffi import (BPLHIP_EUNSUPPORTED, MODEL_BASIC, MODEL_EXTENDED, BplHipError, default_nuts_cfg, prng_key,
                      threefry_split)

_MCMC_KEYS = {"num_chains", "thinning", "progress_bar", "chain_method", "jit_model_args",
              "postprocess_fn"}
_RUN_KEYS = {"init_params", "extra_fields"}
# the sites of the league and the neutral layouts (sizes, not shapes) that are scalars per draw
SCALAR_SITES = frozenset(
    ["corr_coef_raw", "u", "home_advantage", "mean_defence", "mean_home_advantage", "std_attack", "std_defence",
     "std_home_advantage"]
    + [f"{kind}_{side}_{what}" for kind in ("mean", "std") for side in ("home", "away") for what in ("attack", "defence")])
STAT_NAMES = ("potential_energy", "accept_prob", "step_size", "num_steps", "diverging", "corr_coef")


def latent_sites(model: int, T: int, K: int):
    """(name, size) of every latent site in flat (sorted-name) order."""
    if model == MODEL_BASIC:
        return [("attack_decentered", T), ("corr_coef_raw", 1), ("defence_decentered", T),
                ("home_advantage", 1), ("mean_defence", 1), ("std_attack", 1),
                ("std_defence", 1)]
    s = []
    if K:
        s.append(("attack_coefficients", K))
    s.append(("corr_coef_raw", 1))
    if K:
        s.append(("defence_coefficients", K))
    s += [("home_advantage_decentered", T), ("mean_defence", 1), ("mean_home_advantage", 1),
          ("standardised_attack", T), ("standardised_defence", T), ("std_attack", 1),
          ("std_defence", 1), ("std_home_advantage", 1), ("u", 1)]
    return s


def _flatten_init(init_params, model, T, K):
    if init_params is None:
        return None
    if isinstance(init_params, dict):
        parts = []
        for name, size in latent_sites(model, T, K):
            if name not in init_params:
                raise KeyError(f"init_params is missing site '{name}'")
            v = np.asarray(init_params[name], dtype=np.float64).reshape(-1)
            if v.size != size:
                raise ValueError(f"init_params['{name}'] has size {v.size}, expected {size}")
            parts.append(v)
        return np.concatenate(parts)
    return np.asarray(init_params, dtype=np.float64).reshape(-1)


def concat_init(init_params, sites):
    """A dict of start values concatenated in site order, unchecked (the neutral and the dynamic
    classes' rule; the league classes validate site by site, `_flatten_init`); else as given."""
    if isinstance(init_params, dict):
        return np.concatenate([np.asarray(init_params[n], dtype=np.float64).reshape(-1) for n, _ in sites])
    return init_params


def same_start(z0, num_chains: int) -> np.ndarray:
    """One start point handed to every chain: [num_chains] + z0's own shape."""
    return np.stack([np.asarray(z0, np.float64)] * num_chains)


def constrain_sites(sites, z) -> Dict[str, np.ndarray]:
    """numpyro `get_samples()` of the latent sites: the columns of the unconstrained draws z
    [draws, D] cut by `sites` ((name, size or shape) in flat order) and mapped to constrained space.
    A shape gives [draws] + shape; a size gives [draws, size], or [draws] for a site of SCALAR_SITES."""
    out, o = {}, 0
    for name, shape in sites:
        size = int(np.prod(shape))
        v = z[:, o:o + size]
        o += size
        if name.startswith("std_"):
            v = np.exp(v)  # HalfNormal sites: ExpTransform
        elif name in ("corr_coef_raw", "u"):  # Beta sites: SigmoidTransform
            v = np.clip(1.0 / (1.0 + np.exp(-v)), np.finfo(np.float32).tiny, 1.0 - np.finfo(np.float32).eps)
        if isinstance(shape, tuple):
            v = v.reshape((z.shape[0],) + shape)
        elif name in SCALAR_SITES:
            v = v[:, 0]
        out[name] = v
    return out


def neutral_sites(sites, z, cov_std=None, C: int = 0) -> Dict[str, Any]:
    """Every posterior attribute of the neutral-venue classes that is a function of the draws alone (corr_coef is
    not: it is a sampler statistic), as {attribute: array}.  `sites`: the neutral layout's (name, size) list, z
    [draws, D], `cov_std` the standardised covariates [T, K] or None, C the confederation count (0: the attribute
    is None)."""
    lat = constrain_sites(sites, z)  # numpyro get_samples(): constrained latent sites; deterministic ones below
    att_mean, def_mean = 0.0, lat["mean_defence"][:, None]
    if cov_std is not None:
        att_mean = lat["attack_coefficients"] @ cov_std.T
        def_mean = def_mean + lat["defence_coefficients"] @ cov_std.T
    out = {"attack": att_mean + lat["standardised_attack"] * lat["std_attack"][:, None],
           "defence": def_mean + lat["standardised_defence"] * lat["std_defence"][:, None]}
    for nm in ("home_attack", "away_attack", "home_defence", "away_defence"):
        out[nm] = lat["mean_" + nm][:, None] + lat["std_" + nm][:, None] * lat[nm + "_decentered"]
    # LocScaleReparam(centered=0) of Normal(0, 1): the value is the decentered site
    out["confederation_strength"] = lat["confederation_strength_decentered"] if C else None
    out["u"] = lat["u"]
    out["rho"] = 2.0 * lat["u"] - 1.0
    out["attack_coefficients"] = lat.get("attack_coefficients", None)
    out["defence_coefficients"] = lat.get("defence_coefficients", None)
    for nm in ("mean_defence", "std_attack", "std_defence", "mean_home_attack", "mean_away_attack",
               "mean_home_defence", "mean_away_defence", "std_home_attack", "std_home_defence", "std_away_attack",
               "std_away_defence", "standardised_attack", "standardised_defence"):
        out[nm] = lat[nm]
    return out


def dynamic_sites(sites, z) -> Dict[str, Any]:
    """The dynamic class's posterior attributes that are constrained latent sites, as {attribute: array}; the six
    [draws, G, T] tables come from bplhip_constrain_dynamic, corr_coef from the sampler statistics.  `sites`: the
    dynamic layout's (name, shape) list, z [draws, D]."""
    lat = constrain_sites(sites, z)  # constrained latent sites (numpyro get_samples)
    out = {"u": lat["u"], "rho": 2.0 * lat["u"] - 1.0, "attack_coefficients": lat.get("attack_coefficients"),
           "defence_coefficients": lat.get("defence_coefficients")}
    for nm in ("mean_defence", "std_attack", "std_defence", "mean_home_attack", "mean_away_attack",
               "mean_home_defence", "mean_away_defence", "std_home_attack", "std_away_attack", "std_home_defence",
               "std_away_defence", "standardised_attack", "standardised_defence"):
        out[nm] = lat[nm]
    return out


def standardise_covariates(by_team: Optional[dict], teams):
    """([teams, K] table in `teams` order, centred and scaled by the population std; its mean; its
    std), or (None, None, None) without covariates."""
    if not by_team:
        return None, None, None
    if set(by_team) != set(teams):
        raise ValueError("team_covariates must contain all the teams in the data.")
    table = np.array([by_team[name] for name in teams], dtype=np.float64)
    mean, std = table.mean(axis=0), table.std(axis=0)
    return (table - mean) / std, mean, std


def check_goals(home_goals, away_goals):
    hg, ag = np.asarray(home_goals), np.asarray(away_goals)
    if hg.size and (hg.min() < 0 or ag.min() < 0 or hg.max() > 255 or ag.max() > 255):
        raise ValueError("goals must be integers in [0, 255]")
    return hg, ag


def chain_kwargs(mcmc_kwargs, run_kwargs):
    """The keyword checks the league and the neutral classes share: unknown keys, num_chains and
    thinning, chain_method.  Returns the two dicts (copies) and a dict of the three for `sample_chains`."""
    mcmc_kwargs = dict(mcmc_kwargs or {})
    run_kwargs = dict(run_kwargs or {})
    bad = set(mcmc_kwargs) - _MCMC_KEYS
    if bad:
        raise TypeError(f"MCMC got unexpected keyword argument(s) {sorted(bad)}")
    bad = set(run_kwargs) - _RUN_KEYS
    if bad:
        raise TypeError(f"MCMC.run got unexpected keyword argument(s) {sorted(bad)}")
    chains = {"num_chains": int(mcmc_kwargs.get("num_chains", 1)), "thinning": int(mcmc_kwargs.get("thinning", 1)),
              "chain_method": mcmc_kwargs.get("chain_method", "parallel")}
    if chains["num_chains"] < 1 or chains["thinning"] < 1:
        raise ValueError("num_chains and thinning must be >= 1")
    if chains["chain_method"] not in ("parallel", "sequential", "vectorized"):
        raise ValueError("Only supporting the following methods to draw chains: "
                         '"sequential", "parallel", or "vectorized"')
    return mcmc_kwargs, run_kwargs, chains


def mcmc_info(z, num_chains, stats, scal) -> Dict[str, Any]:
    """`mcmc_info_`: stats [chains, kept, STAT_NAMES] (flattened chain-major per name), scal [chains,
    (leapfrogs, seconds, divergences, final step size)].  "step_size" is the per-draw array (the step each kept
    transition used); the adapted step size each chain ended its warm-up with is "final_step_size" [chains]."""
    info = {
        "num_chains": num_chains,
        "unconstrained": z,
        "total_leapfrogs": int(scal[:, 0].sum()),
        "wall_seconds": float(scal[:, 1].max()),
        "divergences": int(scal[:, 2].sum()),
        "final_step_size": scal[:, 3].copy(),
    }
    for i, nm in enumerate(STAT_NAMES):
        info[nm] = stats[:, :, i].reshape(-1)
    return info


def running_mean_accept_prob(accept_prob, num_chains: int) -> np.ndarray:
    """numpyro's HMCState.mean_accept_prob as an extra field: entry i of a chain is the mean of `accept_prob` over
    its post-warmup iterations 0..i (hmc.py: mean_accept_prob += (accept_prob - mean_accept_prob) / n, with n
    counted from the end of the warm-up).  accept_prob [chains * kept] chain-major, every iteration kept
    (thinning == 1); returns the same shape.  A chain's last entry is the library's `mean_accept_prob` scalar
    (nuts.hpp ChainDriver::end: the same recurrence)."""
    a = np.asarray(accept_prob, np.float64).reshape(num_chains, -1)
    return (np.cumsum(a, axis=1) / np.arange(1, a.shape[1] + 1)).reshape(-1)


def sample_chains(bind, *, num_chains=1, thinning=1, chain_method="parallel", random_state=42, num_warmup=500,
                  num_samples=1000, init=None, finish=None, lockstep=True, context_factory=None):
    """The MCMC mechanics of every model class.  `bind(ctx)` binds the fixtures (the one
    model-specific step before sampling); `init(num_chains, D)` returns the start points, row c for
    chain c, or None; `finish(ctx, z)` is the device-side constrain step, run while the context is
    open.  Chain c runs on rank c % world with key split(PRNGKey(random_state), num_chains)[c] (one
    chain: the key itself).  Returns (z [num_chains * kept, D] chain-major, the `mcmc_info` dict,
    what `finish` returned)."""
    rank, ws = _dist.world()
    if context_factory is None:
        from bpl import _ffi

        context_factory = _ffi.HipContext  # (looked up per call: tests swap it)
    ctx = context_factory(_dist.local_device_index() if ws > 1 else 0)
    try:
        bind(ctx)
        D = ctx.dim
        cfg = default_nuts_cfg()
        cfg.num_warmup, cfg.num_samples, cfg.thinning = int(num_warmup), int(num_samples), thinning
        key = prng_key(random_state)
        keys = [key] if num_chains == 1 else threefry_split(key, num_chains)
        z0 = None if init is None else init(num_chains, D)

        mine = _dist.chains_of_rank(num_chains, rank, ws)
        kept = cfg.num_samples // thinning
        draws = np.empty((len(mine), kept, D))
        stats = np.empty((len(mine), kept, len(STAT_NAMES)))
        scal = np.zeros((len(mine), 4))
        # chains that share this GPU run in lock step (numpyro chain_method="vectorized": one
        # chain-vectorised evaluation per leapfrog of all of them) unless chain_method="sequential"
        # or the bound model does not support it
        results = None
        if lockstep and len(mine) > 1 and chain_method != "sequential" and hasattr(ctx, "nuts_run_chains"):
            try:
                results = ctx.nuts_run_chains(cfg, [keys[c] for c in mine], None if z0 is None else z0[list(mine)])
            except BplHipError as e:
                if e.code != BPLHIP_EUNSUPPORTED:
                    raise
        for j, c in enumerate(mine):
            d, st = results[j] if results is not None else ctx.nuts_run(cfg, keys[c], None if z0 is None else z0[c])
            draws[j] = d
            for i, nm in enumerate(STAT_NAMES):
                stats[j, :, i] = st[nm]
            scal[j] = (st["total_leapfrogs"], st["wall_seconds"], st["total_divergences"], st["final_step_size"])
        draws, stats, scal = (_dist.gather_chains(a, num_chains, device=ctx.device) for a in (draws, stats, scal))
        z = draws.reshape(num_chains * kept, D)  # chain-major, numpyro get_samples order
        return z, mcmc_info(z, num_chains, stats, scal), finish(ctx, z) if finish else None
    finally:
        close = getattr(ctx, "close", None)
        if close:
            close()


def run_mcmc(
    model: int,
    home_ind: np.ndarray,
    away_ind: np.ndarray,
    home_goals,
    away_goals,
    n_teams: int,
    *,
    weights: Optional[np.ndarray] = None,
    covariates_std: Optional[np.ndarray] = None,
    random_state: int = 42,
    num_warmup: int = 500,
    num_samples: int = 1000,
    mcmc_kwargs: Optional[Dict[str, Any]] = None,
    run_kwargs: Optional[Dict[str, Any]] = None,
    context_factory: Optional[Callable[[int], Any]] = None,
):
    """The league classes' fit.  Returns (samples: dict of [chains*S, ...] arrays, info: dict)."""
    mcmc_kwargs, run_kwargs, chains = chain_kwargs(mcmc_kwargs, run_kwargs)
    # numpyro's MCMC takes these too; none is silently ignored here (round 3 accepted and dropped them):
    #   postprocess_fn  the map from unconstrained draws to the sites of `get_samples()`: the library's own
    #                   (bplhip_constrain + the closed-form transforms of `constrain_sites`) is the only one there is
    #   jit_model_args  a compilation knob of the JAX path; nothing is traced here, either value is a no-op
    #   extra_fields    (MCMC.run) per-draw sampler statistics: every one this sampler keeps is returned in
    #                   `info` anyway; the names asked for are checked against them and echoed back
    if mcmc_kwargs.get("postprocess_fn") is not None:
        raise NotImplementedError("postprocess_fn: the device sampler constrains its draws itself "
                                  "(bplhip_constrain); transform the returned samples instead")
    extra = tuple(run_kwargs.get("extra_fields") or ())
    known = {"potential_energy", "accept_prob", "mean_accept_prob", "adapt_state.step_size", "step_size",
             "num_steps", "diverging", "energy"}
    bad = [f for f in extra if f not in known]
    if bad:
        raise ValueError(f"extra_fields {bad} are not collected by this sampler; available: {sorted(known - {'energy'})}")
    if "energy" in extra:
        raise ValueError("extra_fields 'energy' (the Hamiltonian of the proposal) is not kept per draw; "
                         "'potential_energy' is")
    if "mean_accept_prob" in extra and chains["thinning"] > 1:
        raise ValueError("extra_fields 'mean_accept_prob' is the running mean of accept_prob over EVERY post-warmup "
                         "iteration; with thinning > 1 the dropped iterations are not kept. Ask for 'accept_prob'")

    hg, ag = check_goals(home_goals, away_goals)
    arrays = {
        "home_idx": np.asarray(home_ind, dtype=np.uint16),
        "away_idx": np.asarray(away_ind, dtype=np.uint16),
        "home_goals": hg.astype(np.uint8),
        "away_goals": ag.astype(np.uint8),
        "weights": None if weights is None else np.asarray(weights, dtype=np.float32),
        "covariates": None if covariates_std is None else np.asarray(covariates_std, np.float64),
    }
    K = 0  # columns of rank 0's covariates, known once they are broadcast

    def bind(ctx):
        nonlocal K
        bc = _dist.broadcast_fixtures(arrays, device=ctx.device)
        cov = None if bc["covariates"] is None else bc["covariates"].cpu().numpy()
        ctx.set_fixtures(model, bc["home_idx"], bc["away_idx"], bc["home_goals"],
                         bc["away_goals"], n_teams, weights=bc["weights"], covariates_std=cov)
        K = 0 if cov is None else cov.shape[1]

    def init(num_chains, D):  # [D] for every chain, or num_chains * D values
        z0 = _flatten_init(run_kwargs.get("init_params"), model, n_teams, K)
        if z0 is None:
            return None
        return z0.reshape(num_chains, D) if z0.size == num_chains * D and num_chains > 1 else same_start(z0, num_chains)

    z, info, site = sample_chains(bind, random_state=random_state, num_warmup=num_warmup, num_samples=num_samples,
                                  init=init, finish=lambda ctx, z: ctx.constrain(z),
                                  context_factory=context_factory, **chains)
    # numpyro `get_samples()`: the deterministic sites of bplhip_constrain + the constrained latent sites
    samples = dict(site)
    for name, v in constrain_sites(latent_sites(model, n_teams, K), z).items():
        samples.setdefault(name, v)
    if model == MODEL_EXTENDED:
        samples["rho"] = 2.0 * samples["u"] - 1.0
    alias = {"adapt_state.step_size": "step_size"}
    info["extra_fields"] = {f: info[alias.get(f, f)] for f in extra if f != "mean_accept_prob"}
    if "mean_accept_prob" in extra:
        info["extra_fields"]["mean_accept_prob"] = running_mean_accept_prob(info["accept_prob"], info["num_chains"])
    return samples, info
