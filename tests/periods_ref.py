"""float64 numpy restatement of predict_periods (bpl/periods.py, csrc/dc_period.hip.h) by a different route from
the kernel's recurrences: the FULL [G+1]^4 array p(a, b, x, y) of every (draw, fixture) from closed-form pmfs
(exp(k log rate - rate - lgamma(k + 1)), the rate-0 cases of split 0 and 1 written out), the tau factor on the
four low FINAL cells, a contraction with the market weights, then markets_ref.summarise."""
import numpy as np
from scipy.special import gammaln

import markets_ref as MR
import scores_ref as SR
from bpl import markets as MK
from bpl import periods as PD

CELLS = 1 << 20   # cells of p held at once


def all_builders():
    """One period market from every builder."""
    return {"ht_over_0.5": PD.first_period(MK.total_over(0.5)), "second_draw": PD.second_period("draw"),
            "ft_home": PD.full_time("home"),
            "lead_and_not_win": PD.all_of(PD.first_period("home"), PD.full_time(MK.handicap(0.5, "away"))),
            "draw_home": PD.ht_ft("draw", "home"), "both_home": PD.win_both_periods("home"),
            "either_away": PD.win_either_period("away"), "score_both_home": PD.score_in_both_periods("home"),
            "second_highest": PD.highest_scoring_period("second"), "comeback_away": PD.comeback("away")}


def weights_of(markets, G):
    """[K, G+1, G+1, G+1, G+1] of a dict name -> PeriodMarket or array."""
    return np.stack([m.weights(G) if isinstance(m, PD.PeriodMarket) else np.asarray(m, dtype=np.float64)
                     for m in markets.values()])


def readable(G):
    """[G+1]^4 bool: a <= x and b <= y."""
    a, b, x, y = np.ix_(*(np.arange(G + 1),) * 4)
    return (a <= x) & (b <= y)


def pois(k, rate):
    """Pois(k; rate), rate [...] against counts k [G+1] -> [..., G+1]; Pois(0; 0) = 1, Pois(k > 0; 0) = 0."""
    rate = np.asarray(rate, dtype=np.float64)[..., None]
    with np.errstate(all="ignore"):
        p = np.exp(k * np.log(rate) - rate - gammaln(k + 1.0))
    return np.where(rate == 0.0, (k == 0).astype(np.float64), p)


def side_law(rate, f, G):
    """[..., a, x]: Pois(a; f rate) Pois(x - a; (1 - f) rate), 0 where a > x."""
    k = np.arange(G + 1, dtype=np.float64)
    first, second = pois(k, f * rate), pois(k, (1.0 - f) * rate)   # [..., G+1]
    a, x = np.meshgrid(np.arange(G + 1), np.arange(G + 1), indexing="ij")
    return np.where(a <= x, first[..., a] * second[..., np.maximum(x - a, 0)], 0.0)


def joint(lh, la, rho, f, G):
    """p [S, n, a, b, x, y] for rates [S, n], rho [S] and splits f [n]."""
    r = np.asarray(rho, dtype=np.float64)[:, None]
    F = np.ones(lh.shape + (G + 1, G + 1))
    F[..., 0, 0] = np.maximum(1.0 - r * lh * la, 0.0)
    if G >= 1:
        F[..., 0, 1] = np.maximum(1.0 + r * lh, 0.0)
        F[..., 1, 0] = np.maximum(1.0 + r * la, 0.0)
        F[..., 1, 1] = np.maximum(1.0 - r + 0.0 * lh, 0.0)
    ph, pa = side_law(lh, f[None, :], G), side_law(la, f[None, :], G)   # [S, n, a, x], [S, n, b, y]
    p = ph[:, :, :, None, :, None] * pa[:, :, None, :, None, :]
    p *= F[:, :, None, None, :, :]
    return p


def values_from_rates(lh, la, rho, split, W, G):
    """v [S, K, n]: per draw and fixture the joint law contracted with every market's weights."""
    S, n = lh.shape
    f = np.broadcast_to(np.asarray(split, dtype=np.float64), (n,))
    W = np.where(readable(G), np.asarray(W, dtype=np.float64), 0.0).reshape(len(W), -1)
    out = np.empty((S, W.shape[0], n))
    rows = min(S, max(1, CELLS // (G + 1) ** 4))          # draws at once (one fixture can be more than CELLS)
    step = max(1, CELLS // (rows * (G + 1) ** 4))         # fixtures at once
    for i in range(0, n, step):
        for s0 in range(0, S, rows):
            p = joint(lh[s0:s0 + rows, i:i + step], la[s0:s0 + rows, i:i + step], rho[s0:s0 + rows], f[i:i + step], G)
            out[s0:s0 + rows, :, i:i + step] = np.einsum("kc,snc->skn", W, p.reshape(p.shape[0], p.shape[1], -1),
                                                         optimize=True)
    return out


def values(m, data, markets, split, G):
    lh, la = SR.rates(m, data)
    return values_from_rates(lh, la, np.asarray(m.corr_coef, dtype=np.float64), split, weights_of(markets, G), G)


def predict_periods(m, data, markets, split, G, quantiles):
    v = values(m, data, markets, split, G)
    out = MR.summarise(v, quantiles)
    out["draws"] = v
    return out


def device_part(lh, la, rho, split, weights, quantiles, G, return_draws):
    """What HipContext.period_summary returns for these rates."""
    v = values_from_rates(lh, la, np.asarray(rho, dtype=np.float64), split, np.asarray(weights, dtype=np.float64), G)
    out = MR.summarise(v, quantiles)
    if return_draws:
        out["draws"] = v
    return out
