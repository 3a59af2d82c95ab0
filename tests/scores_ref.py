"""float64 numpy restatement of forecast_scores (bpl/scoring.py, csrc/dc_score.hip.h) by a deliberately
different route from the kernel's O(G) walk: the FULL (G+1) x (G+1) scoreline grid of every (draw,
fixture), each cell from its own closed form exp(k log rate - rate - lgamma(k+1)), the tau factor on the
four low cells, then the three triangles, the mean over the draws and the rules.  The rates are those
tests/loglik_ref.py::ll_matrix forms: each class's own `_calculate_expected_goals`."""
import numpy as np
from scipy.special import gammaln

from bpl import NeutralDixonColesMatchPredictor, NeutralDixonColesMatchPredictorWC
from bpl.base import BaseMatchPredictor

CELLS = 1 << 24   # grid cells held at once


def rates(m, data):
    """(lh, la) [S, n] of the fixtures of `data` (the rate calls of loglik_ref.ll_matrix)."""
    h, a = list(data["home_team"]), list(data["away_team"])
    if isinstance(m, BaseMatchPredictor):
        return m._calculate_expected_goals(h, a)
    if isinstance(m, NeutralDixonColesMatchPredictorWC):
        return m._calculate_expected_goals(h, a, list(data["home_conf"]), list(data["away_conf"]),
                                           np.asarray(data["neutral_venue"]))
    if isinstance(m, NeutralDixonColesMatchPredictor):
        return m._calculate_expected_goals(h, a, np.asarray(data["neutral_venue"]))
    gw, nv = np.asarray(data["gameweek"]), np.asarray(data["neutral_venue"])
    S = np.shape(m.corr_coef)[0]
    lh, la = np.empty((S, len(h))), np.empty((S, len(h)))
    for g in np.unique(gw):
        pos = np.nonzero(gw == g)[0]
        lh[:, pos], la[:, pos] = m._calculate_expected_goals([h[i] for i in pos], [a[i] for i in pos], nv[pos],
                                                             gameweek=int(g))
    return lh, la


def grid(lh, la, rho, G):
    """[S, n, G+1, G+1] q(x, y) = max(1 + rho c, 0) Pois(x; lh) Pois(y; la), axis 2 the home goals."""
    k = np.arange(G + 1, dtype=np.float64)
    lg = gammaln(k + 1.0)
    with np.errstate(all="ignore"):
        ph = np.exp(k * np.log(lh)[..., None] - lh[..., None] - lg)
        pa = np.exp(k * np.log(la)[..., None] - la[..., None] - lg)
    q = ph[..., :, None] * pa[..., None, :]
    r = np.asarray(rho, dtype=np.float64)[:, None]
    q[..., 0, 0] *= np.maximum(1.0 - r * lh * la, 0.0)
    if G >= 1:
        q[..., 0, 1] *= np.maximum(1.0 + r * lh, 0.0)
        q[..., 1, 0] *= np.maximum(1.0 + r * la, 0.0)
        q[..., 1, 1] *= np.maximum(1.0 - r + 0.0 * lh, 0.0)
    return q


def draw_probs(lh, la, rho, G):
    """p [S, n, 3]: per draw and fixture the sums of the grid over x > y, x = y, x < y."""
    S, n = lh.shape
    x, y = np.meshgrid(np.arange(G + 1), np.arange(G + 1), indexing="ij")
    masks = [(x > y).astype(np.float64), (x == y).astype(np.float64), (x < y).astype(np.float64)]
    out = np.empty((S, n, 3))
    step = max(1, CELLS // (S * (G + 1) * (G + 1)))
    for i in range(0, n, step):
        q = grid(lh[:, i:i + step], la[:, i:i + step], rho, G)
        for c, mask in enumerate(masks):
            out[:, i:i + step, c] = (q * mask).sum(axis=(-2, -1))
    return out


def outcome_of(home_goals, away_goals):
    x, y = np.asarray(home_goals, dtype=np.int64), np.asarray(away_goals, dtype=np.int64)
    return np.where(x > y, 0, np.where(x == y, 1, 2)).astype(np.uint8)


def rules(p, o):
    """(log, brier, rps) of triples p [..., n, 3] against classes o [n]."""
    hit = np.zeros(p.shape[-2:])
    hit[np.arange(o.size), o] = 1.0
    with np.errstate(divide="ignore"):
        log = np.log((p * hit).sum(axis=-1))
    brier = ((p - hit) ** 2).sum(axis=-1)
    cp, ch = np.cumsum(p, axis=-1), np.cumsum(hit, axis=-1)
    rps = 0.5 * ((cp[..., 0] - ch[:, 0]) ** 2 + (cp[..., 1] - ch[:, 1]) ** 2)
    return log, brier, rps


def device_part(lh, la, rho, home_goals, away_goals, G):
    """What HipContext.outcome_scores returns for these rates: "proba" [n, 3] and "draw_sums" [S, 3]."""
    p = draw_probs(lh, la, rho, G)
    o = outcome_of(home_goals, away_goals)
    with np.errstate(invalid="ignore"):
        sums = np.stack([r.sum(axis=1) for r in rules(p, o)], axis=1)
    return {"proba": p.mean(axis=0), "draw_sums": sums}


def scores(m, data, G):
    """The restatement of forecast_scores (without "calibration"), plus "p_draws" [S, n, 3]."""
    lh, la = rates(m, data)
    p = draw_probs(lh, la, np.asarray(m.corr_coef, dtype=np.float64), G)
    o = outcome_of(data["home_goals"], data["away_goals"])
    P = p.mean(axis=0)
    out = {"n": o.size, "outcome": o, "outcome_proba": P, "p_draws": p}
    on_mean, per_draw = rules(P, o), rules(p, o)
    for i, name in enumerate(("log_score", "brier", "rps")):
        v = on_mean[i]
        out[f"{name}_i"] = v
        out[name] = float(v.mean())
        out[f"{name}_se"] = (0.0 if v.size < 2 else
                             float(np.std(v, ddof=1) / np.sqrt(v.size)) if np.isfinite(v).all() else np.inf)
        out[f"{name}_draws"] = per_draw[i].mean(axis=1)
    return out
