"""float64 numpy restatement of the log-likelihood path (csrc/dc_loglik.hip.h, bpl/elpd.py): the ll
matrix from each class's own `_calculate_expected_goals`, the per-fixture summaries, and PSIS-LOO step by
step as DESIGN.md section 12 defines it (ArviZ's _psislw / _gpdfit written out, with the tail sorted
stably by (x, draw)).  Also hand-built posteriors and data for the five predictor classes."""
import math

import numpy as np
from scipy.special import gammaln, logsumexp

from bpl import (DixonColesMatchPredictor, ExtendedDixonColesMatchPredictor, NeutralDixonColesMatchPredictor,
                 NeutralDixonColesMatchPredictorWC)
from bpl.base import BaseMatchPredictor
from bpl.dynamic_dixon_coles import DynamicNeutralDixonColesMatchPredictor
from bpl.elpd import tail_size

LOG_DBL_MIN = float(np.log(np.finfo(float).tiny))
EPS = float(np.finfo(float).eps)
KINDS = ("basic", "extended", "neutral", "wc", "dynamic")


# ---- posteriors and data
def hand_model(kind, S=64, T=8, seed=0, C=3, G=3):
    rs = np.random.RandomState(seed)
    names = [f"t{i:02d}" for i in range(T)]
    if kind in ("basic", "extended"):
        m = DixonColesMatchPredictor() if kind == "basic" else ExtendedDixonColesMatchPredictor()
        m.teams = np.array(names)
        m._teams_dict = {t: i for i, t in enumerate(names)}
        m.attack, m.defence = rs.normal(0, 0.3, (S, T)), rs.normal(0, 0.3, (S, T))
        m.home_advantage = rs.normal(0.25, 0.05, S) if kind == "basic" else rs.normal(0.25, 0.1, (S, T))
        m.corr_coef = rs.uniform(-0.1, 0.1, S)
        return m
    if kind == "dynamic":
        m = DynamicNeutralDixonColesMatchPredictor()
        m.teams = list(names)
        m.num_gameweeks = G
        for nm in ("attack", "defence", "home_attack", "away_attack", "home_defence", "away_defence"):
            setattr(m, nm, rs.normal(0, 0.3 if nm in ("attack", "defence") else 0.1, (S, G, T)))
        m.corr_coef = rs.uniform(-0.1, 0.1, S)
        return m
    m = NeutralDixonColesMatchPredictor() if kind == "neutral" else NeutralDixonColesMatchPredictorWC()
    m.teams = np.array(names)
    m._teams_dict = {t: i for i, t in enumerate(names)}
    for nm in ("attack", "defence"):
        setattr(m, nm, rs.normal(0, 0.3, (S, T)))
    for nm in ("home_attack", "away_attack", "home_defence", "away_defence"):
        setattr(m, nm, rs.normal(0, 0.1, (S, T)))
    m.corr_coef = rs.uniform(-0.1, 0.1, S)
    if kind == "wc":
        m.conferences = np.array([f"c{i}" for i in range(C)])
        m._conferences_dict = {c: i for i, c in enumerate(m.conferences)}
        m.confederation_strength = rs.normal(0, 0.2, (S, C))
    return m


def hand_data(m, n=50, seed=1, max_goals=6):
    rs = np.random.RandomState(seed)
    teams = list(m.teams)
    h = rs.randint(0, len(teams), n)
    a = (h + 1 + rs.randint(0, len(teams) - 1, n)) % len(teams)
    d = {"home_team": [teams[i] for i in h], "away_team": [teams[i] for i in a],
         "home_goals": rs.randint(0, max_goals + 1, n), "away_goals": rs.randint(0, max_goals + 1, n)}
    if not isinstance(m, BaseMatchPredictor):
        d["neutral_venue"] = rs.randint(0, 2, n)
    if isinstance(m, NeutralDixonColesMatchPredictorWC):
        conf = list(m.conferences)
        d["home_conf"] = [conf[i] for i in rs.randint(0, len(conf), n)]
        d["away_conf"] = [conf[i] for i in rs.randint(0, len(conf), n)]
    if isinstance(m, DynamicNeutralDixonColesMatchPredictor):
        d["gameweek"] = rs.randint(0, m.num_gameweeks, n)
    return d


# ---- the matrix
def ll_from_rates(lh, la, x, y, rho):
    """[S, n] log of tau * Poisson(x; lh) * Poisson(y; la), tau clipped at 0 (-inf)."""
    x = np.asarray(x, dtype=np.float64)[None, :]
    y = np.asarray(y, dtype=np.float64)[None, :]
    with np.errstate(all="ignore"):
        v = x * np.log(lh) - lh - gammaln(x + 1) + y * np.log(la) - la - gammaln(y + 1)
        c = np.where(x == 0, np.where(y == 0, -(lh * la), lh), np.where(y == 0, la, -1.0))
        tau = np.log(np.maximum(1.0 + rho[:, None] * c, 0.0))
    return np.where((x <= 1) & (y <= 1), v + tau, v)


def ll_matrix(m, data):
    h, a = list(data["home_team"]), list(data["away_team"])
    x, y = np.asarray(data["home_goals"]), np.asarray(data["away_goals"])
    rho = np.asarray(m.corr_coef, dtype=np.float64)
    if isinstance(m, BaseMatchPredictor):
        lh, la = m._calculate_expected_goals(h, a)
    elif isinstance(m, NeutralDixonColesMatchPredictorWC):
        lh, la = m._calculate_expected_goals(h, a, list(data["home_conf"]), list(data["away_conf"]),
                                             np.asarray(data["neutral_venue"]))
    elif isinstance(m, NeutralDixonColesMatchPredictor):
        lh, la = m._calculate_expected_goals(h, a, np.asarray(data["neutral_venue"]))
    else:
        gw, nv = np.asarray(data["gameweek"]), np.asarray(data["neutral_venue"])
        out = np.empty((rho.size, len(h)))
        for g in np.unique(gw):
            pos = np.nonzero(gw == g)[0]
            lh, la = m._calculate_expected_goals([h[i] for i in pos], [a[i] for i in pos], nv[pos], gameweek=int(g))
            out[:, pos] = ll_from_rates(lh, la, x[pos], y[pos], rho)
        return out
    return ll_from_rates(lh, la, x, y, rho)


# ---- PSIS
def gpdfit(z):
    """Zhang-Stephens fit of a generalised Pareto distribution to sorted exceedances z (> 0), with the
    weak prior on k; returns (k, sigma)."""
    n = z.size
    m = 30 + int(n ** 0.5)
    b = 1 - np.sqrt(m / (np.arange(1, m + 1, dtype=np.float64) - 0.5))
    b /= 3 * z[int(n / 4 + 0.5) - 1]
    b += 1 / z[-1]
    with np.errstate(all="ignore"):
        kj = np.log1p(-b[:, None] * z).mean(axis=1)
        lj = n * (np.log(-(b / kj)) - kj - 1)
        w = 1 / np.exp(lj - lj[:, None]).sum(axis=1)
        keep = w >= 10 * EPS
        w, b = w[keep], b[keep]
        w = w / w.sum()
        bh = np.sum(b * w)
        kh = np.log1p(-bh * z).mean()
        sigma = -kh / bh
    return (n * kh + 5.0) / (n + 10), sigma


def psis(ll, r_eff=1.0, return_lw=False):
    """One fixture's draws -> (elpd_loo, k, L[, lw])."""
    ll = np.asarray(ll, dtype=np.float64)
    S = ll.size
    if not np.all(ll > -np.inf):
        return (-np.inf, np.inf, 0) + ((None,) if return_lw else ())
    M = tail_size(S, r_eff)
    r = -ll
    x = (r - r.max()) + 0.0
    order = np.argsort(x, kind="stable")
    cutoff = max(x[order[S - M - 1]], LOG_DBL_MIN)
    tail = np.nonzero(x > cutoff)[0]
    L = tail.size
    k = np.inf
    if L > 4:
        ti = tail[np.argsort(x[tail], kind="stable")]
        z = np.exp(x[ti]) - np.exp(cutoff)
        k, sigma = gpdfit(z)
        if not (np.isfinite(k) and sigma > 0 and np.isfinite(sigma)):
            k = np.inf
        else:
            p = np.arange(0.5, L) / L
            q = -np.log1p(-p) if abs(k) < EPS else np.expm1(-k * np.log1p(-p)) / k
            x = x.copy()
            x[ti] = np.log(q * sigma + np.exp(cutoff))
            x[x > 0] = 0
    lw = x - logsumexp(x)
    out = (float(logsumexp(lw + ll)), float(k), int(L))
    return out + ((lw,) if return_lw else ())


def summary(ll, r_eff=1.0, psis_on=True):
    ll = np.asarray(ll, dtype=np.float64)
    S, n = ll.shape
    bad = ~np.all(ll > -np.inf, axis=0)
    with np.errstate(all="ignore"):
        out = {"lppd": logsumexp(ll, axis=0) - math.log(S), "mean": ll.mean(axis=0),
               "var": ll.var(axis=0, ddof=1) if S > 1 else np.zeros(n)}
    out["var"] = np.where(bad, np.inf, out["var"])
    out["mean"] = np.where(bad, -np.inf, out["mean"])
    if psis_on:
        res = [psis(ll[:, i], r_eff) for i in range(n)]
        out["elpd_loo"] = np.array([r[0] for r in res])
        out["pareto_k"] = np.array([r[1] for r in res])
        out["tail_len"] = np.array([r[2] for r in res], dtype=np.int32)
    return out


def waic(ll):
    s = summary(ll, psis_on=False)
    elpd_i = s["lppd"] - s["var"]
    return {"elpd_waic": elpd_i.sum(), "p_waic": s["var"].sum(), "elpd_waic_i": elpd_i, "lppd_i": s["lppd"]}


def loo(ll, r_eff=1.0):
    s = summary(ll, r_eff)
    return {"elpd_loo": s["elpd_loo"].sum(), "p_loo": s["lppd"].sum() - s["elpd_loo"].sum(),
            "elpd_loo_i": s["elpd_loo"], "pareto_k": s["pareto_k"]}
