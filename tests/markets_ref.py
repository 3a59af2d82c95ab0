"""float64 numpy restatement of predict_markets (bpl/markets.py, csrc/dc_market.hip.h) by a different route
from the kernel's recurrences: the FULL (G+1) x (G+1) scoreline grid of every (draw, fixture) from closed-form
pmfs (scores_ref.rates, scores_ref.grid), an einsum with the market weights, then per (market, fixture) a sort
of the per-draw values and the interpolation formula written out (not np.quantile)."""
import numpy as np

import scores_ref as SR
from bpl import markets as MK

CELLS = 1 << 23   # grid cells held at once


def all_builders(G=None):
    """One market from every builder."""
    return {"home_win": MK.home_win(), "draw": MK.draw(), "away_win": MK.away_win(), "over_2.5": MK.total_over(2.5),
            "under_2": MK.total_under(2), "handicap_home_-1": MK.handicap(-1, "home"),
            "handicap_away_+1.5": MK.handicap(1.5, "away"), "btts": MK.btts(), "clean_sheet_home": MK.clean_sheet("home"),
            "clean_sheet_away": MK.clean_sheet("away"), "score_1_0": MK.correct_score(1, 0),
            "goals_home": MK.goals("home"), "goals_away": MK.goals("away"), "total_goals": MK.total_goals()}


def weights_of(markets, G):
    """[K, G+1, G+1] of a dict name -> Market or array."""
    return np.stack([m.weights(G) if isinstance(m, MK.Market) else np.asarray(m, dtype=np.float64)
                     for m in markets.values()])


def values_from_rates(lh, la, rho, W, G):
    """v [S, K, n]: per draw and fixture the grid contracted with every market's weights."""
    S, n = lh.shape
    out = np.empty((S, W.shape[0], n))
    step = max(1, CELLS // (S * (G + 1) * (G + 1)))
    for i in range(0, n, step):
        q = SR.grid(lh[:, i:i + step], la[:, i:i + step], rho, G)
        out[:, :, i:i + step] = np.einsum("kxy,snxy->skn", W, q, optimize=True)
    return out


def values(m, data, markets, G):
    lh, la = SR.rates(m, data)
    return values_from_rates(lh, la, np.asarray(m.corr_coef, dtype=np.float64), weights_of(markets, G), G)


def summarise(v, quantiles):
    """mean, sd [K, n] and quantile [K, Q, n] of values v [S, K, n]."""
    S = v.shape[0]
    srt = np.sort(v, axis=0)
    q = np.asarray(quantiles, dtype=np.float64).reshape(-1)
    quant = np.empty((v.shape[1], q.size, v.shape[2]))
    for i, qi in enumerate(q):
        h = qi * (S - 1)
        lo = int(np.floor(h))
        hi = min(lo + 1, S - 1)
        quant[:, i, :] = srt[lo] + (h - lo) * (srt[hi] - srt[lo])
    sd = v.std(axis=0, ddof=1) if S > 1 else np.zeros(v.shape[1:])
    return {"mean": v.mean(axis=0), "sd": sd, "quantile": quant}


def predict_markets(m, data, markets, G, quantiles):
    v = values(m, data, markets, G)
    out = summarise(v, quantiles)
    out["draws"] = v
    return out


def device_part(lh, la, rho, weights, quantiles, G, return_draws):
    """What HipContext.market_summary returns for these rates."""
    v = values_from_rates(lh, la, rho, np.asarray(weights, dtype=np.float64), G)
    out = summarise(v, quantiles)
    if return_draws:
        out["draws"] = v
    return out
