"""float64 numpy restatement of the MCMC convergence diagnostics (csrc/dc_diagnostics.hip.h, bpl/diagnostics.py), one
quantity at a time, as DESIGN.md section 20 defines them: split chains, average ranks, Phi^-1 from
`statistics.NormalDist`, direct autocovariance sums, Geyer's initial positive and monotone sequences written out.
Every ess also reports its smallest decision margin: the least absolute value over every pair sum compared with 0,
every monotone-sequence comparison and tau minus its floor."""
import math
from statistics import NormalDist

import numpy as np

STATS = ("mean", "sd", "rhat", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean")
_INV = NormalDist().inv_cdf


def split_chains(x, num_chains):
    """[C * N] chain-major -> [2 C, N // 2]: each chain's first and last N // 2 draws."""
    x = np.asarray(x, dtype=np.float64).reshape(num_chains, -1)
    n = x.shape[1] // 2
    return np.stack([x[:, :n], x[:, x.shape[1] - n:]], axis=1).reshape(2 * num_chains, n)


def average_ranks(v):
    """1-based ranks of a flat array; tied values share the mean of their ranks."""
    v = np.asarray(v, dtype=np.float64).ravel() + 0.0
    order = np.argsort(v, kind="stable")
    s = v[order]
    ranks = np.empty(v.size)
    i = 0
    while i < v.size:
        j = i + 1
        while j < v.size and s[j] == s[i]:
            j += 1
        ranks[order[i:j]] = 0.5 * ((i + 1) + j)
        i = j
    return ranks


def z_scale(m):
    """Rank normalisation of the pooled values of an M x n matrix."""
    r = average_ranks(m)
    S = r.size
    return np.array([_INV((ri - 0.375) / (S + 0.25)) for ri in r]).reshape(m.shape)


def rhat_of(m):
    n = m.shape[1]
    W = np.mean(np.var(m, axis=1, ddof=1))
    Bn = np.var(np.mean(m, axis=1), ddof=1)
    if W == 0.0:
        return math.nan
    return math.sqrt(((n - 1) / n * W + Bn) / W)


def ess_of(m, with_last_lag=False, facts=None):
    """(ess, smallest decision margin) of an M x n matrix; with_last_lag: also the largest lag whose autocovariance
    the walk needed.  facts: a dict that receives what the walk did -- "stop_lag" (t when the positive sequence
    ended), "stop_reason" ("bound": t < n - 3 failed, "pair": a pair sum was not above 0, "constant": var_plus = 0),
    "replacements" (pairs the monotone step replaced), "floor" (tau was below 1 / log10 S), "tau" and "rho" (the
    autocorrelations the walk computed, lags 0 .. stop_lag)."""
    M, n = m.shape
    S = M * n
    d = m - m.mean(axis=1, keepdims=True)

    def acov(t):   # mean over the chains of acov_c(t)
        return float(np.mean(np.sum(d[:, :n - t] * d[:, t:], axis=1) / n))

    mean_var = acov(0) * n / (n - 1.0)
    var_plus = mean_var * (n - 1.0) / n
    if M > 1:
        var_plus += float(np.var(m.mean(axis=1), ddof=1))
    if var_plus == 0.0:
        if facts is not None:
            facts.update(stop_lag=0, stop_reason="constant", replacements=0, floor=False, tau=math.nan, rho=[])
        return (math.nan, math.inf, 0) if with_last_lag else (math.nan, math.inf)
    rho = np.zeros(n + 2)
    rho_of = lambda t: 1.0 - (mean_var - acov(t)) / var_plus
    margin = math.inf
    even, odd = 1.0, rho_of(1)
    rho[0], rho[1] = even, odd
    computed = [even, odd]
    reason = "bound"
    t = 1
    while t < n - 3:
        margin = min(margin, abs(even + odd))
        if not even + odd > 0.0:
            reason = "pair"
            break
        even, odd = rho_of(t + 1), rho_of(t + 2)
        computed += [even, odd]
        if even + odd >= 0.0:
            rho[t + 1], rho[t + 2] = even, odd
        t += 2
    if t > 1:
        margin = min(margin, abs(even + odd))   # (the last pair's own test against 0)
    last_lag = t
    max_t = t - 2
    if even > 0.0:
        rho[max_t + 1] = even
    replaced = 0
    t = 1
    while t <= max_t - 2:
        margin = min(margin, abs((rho[t + 1] + rho[t + 2]) - (rho[t - 1] + rho[t])))
        if rho[t + 1] + rho[t + 2] > rho[t - 1] + rho[t]:
            rho[t + 1] = (rho[t - 1] + rho[t]) / 2.0
            rho[t + 2] = rho[t + 1]
            replaced += 1
        t += 2
    tau = -1.0 + 2.0 * float(np.sum(rho[:max_t + 1])) + rho[max_t + 1]
    floor = 1.0 / math.log10(S)
    margin = min(margin, abs(tau - floor))
    ess = S / max(tau, floor)
    if facts is not None:
        facts.update(stop_lag=last_lag, stop_reason=reason, replacements=replaced, floor=tau < floor, tau=tau,
                     rho=computed)
    return (ess, margin, last_lag) if with_last_lag else (ess, margin)


def diagnose_one(x, num_chains, quantiles=(0.05, 0.95)):
    """Every statistic of one quantity's [C * N] chain-major draws, plus "margin" and the two R-hats."""
    x = np.asarray(x, dtype=np.float64).ravel()
    out = {nm: math.nan for nm in STATS}
    out.update(margin=math.inf, rhat_bulk=math.nan, rhat_folded=math.nan)
    with np.errstate(all="ignore"):
        out["mean"] = float(np.mean(x))
        out["sd"] = float(np.std(x, ddof=1))
    if not np.all(np.isfinite(x)):
        return out
    s = split_chains(x, num_chains)
    if s.min() == s.max():   # constant: W = 0 and every var_plus = 0
        return out
    zb = z_scale(s)
    zf = z_scale(np.abs(s - np.median(s)))
    out["rhat_bulk"], out["rhat_folded"] = rhat_of(zb), rhat_of(zf)
    out["rhat"] = float(np.maximum(out["rhat_bulk"], out["rhat_folded"]))
    out["ess_bulk"], m1 = ess_of(zb)
    out["ess_mean"], m2 = ess_of(s)
    tails, m3 = [], math.inf
    for q in quantiles:
        e, mq = ess_of((s <= np.quantile(s, q)).astype(np.float64))
        tails.append(e)
        m3 = min(m3, mq)
    out["ess_tail"] = float(np.min(tails)) if tails else math.nan
    out["mcse_mean"] = out["sd"] / math.sqrt(out["ess_mean"]) if out["ess_mean"] == out["ess_mean"] else math.nan
    out["margin"] = min(m1, m2, m3)
    return out


def diagnose(values, num_chains, quantiles=(0.05, 0.95)):
    """`values` [C * N, Q] -> dict of [Q] arrays (the statistics and "margin")."""
    values = np.asarray(values, dtype=np.float64)
    rows = [diagnose_one(values[:, j], num_chains, quantiles) for j in range(values.shape[1])]
    return {nm: np.array([r[nm] for r in rows]) for nm in STATS + ("margin",)}


def backend(values, num_chains, quantiles, workspace_bytes=0):
    """A stand-in for the device call of bpl.diagnostics (same signature, same keys)."""
    full = diagnose(values, num_chains, tuple(quantiles))
    return {nm: full[nm] for nm in STATS}


def ar1(rs, C, N, phi, Q=1):
    """[C * N, Q] stationary AR(1) chains with unit innovations."""
    out = np.empty((C, N, Q))
    out[:, 0] = rs.normal(size=(C, Q)) / math.sqrt(1.0 - phi * phi)
    for i in range(1, N):
        out[:, i] = phi * out[:, i - 1] + rs.normal(size=(C, Q))
    return out.reshape(C * N, Q)
