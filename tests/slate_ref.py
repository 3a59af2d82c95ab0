"""float64 numpy restatement of predict_slate (bpl/slate.py, csrc/dc_slate.hip.h) by a different route from the
kernel's: the FULL scoreline grid of every (draw, fixture) from closed-form pmfs (scores_ref.rates,
scores_ref.grid), np.bincount of the grid by leg value for a leg's value law, np.convolve in list order for a
draw's law of the total, markets_ref.summarise for the summaries.  A second, independent route for small slates:
enumerate all prod(m_i + 1) value combinations and add the products, with no convolution."""
import itertools

import numpy as np

import markets_ref as MR
import scores_ref as SR
from bpl import markets as MK

CELLS = 1 << 23   # grid cells held at once


def table_of(leg, G):
    """int64 [G+1, G+1] of a Market or an array."""
    w = leg.weights(G) if isinstance(leg, MK.Market) else np.asarray(leg, dtype=np.float64)
    t = w.astype(np.int64)
    assert t.shape == (G + 1, G + 1) and (t == w).all() and t.min() >= 0 and t.max() <= 7
    return t


def leg_laws_from_rates(lh, la, rho, tables, G):
    """r [S, n, 8]: per draw and fixture the grid's mass on each leg value (np.bincount per grid)."""
    S, n = lh.shape
    out = np.empty((S, n, 8))
    step = max(1, CELLS // (S * (G + 1) * (G + 1)))
    for i0 in range(0, n, step):
        q = SR.grid(lh[:, i0:i0 + step], la[:, i0:i0 + step], rho, G)
        for i in range(q.shape[1]):
            flat = tables[i0 + i].reshape(-1)
            for s in range(S):
                out[s, i0 + i] = np.bincount(flat, weights=q[s, i].reshape(-1), minlength=8)
    return out


def slate_stats(r, tops, index, J):
    """Per draw and slate from the leg laws r [S, n, 8] (leg i with the values 0..tops[i]): pmf, at_least
    [S, J, P+1], expected, mass [S, J], with np.convolve in list order."""
    S = r.shape[0]
    max_total = np.bincount(index, weights=tops, minlength=J).astype(np.int64)
    P = int(max_total.max())
    pmf = np.zeros((S, J, P + 1))
    for j in range(J):
        for s in range(S):
            p = np.ones(1)
            for i in np.nonzero(index == j)[0]:
                p = np.convolve(p, r[s, i, :tops[i] + 1])
            pmf[s, j, :p.size] = p
    at_least = np.cumsum(pmf[:, :, ::-1], axis=2)[:, :, ::-1]
    return {"pmf": pmf, "at_least": at_least, "expected": pmf @ np.arange(P + 1.0), "mass": at_least[:, :, 0],
            "max_total": max_total}


def enumerate_pmf(r, tops, rows):
    """pmf [S, rows] of one slate with the leg laws r [S, N, 8]: the sum over every combination of leg values of
    the product of their probabilities, math.fsum-free and convolution-free (small N only)."""
    S, N = r.shape[:2]
    out = np.zeros((S, rows))
    for combo in itertools.product(*[range(int(t) + 1) for t in tops]):
        prod = np.ones(S)
        for i, v in enumerate(combo):
            prod = prod * r[:, i, v]
        out[:, sum(combo)] += prod
    return out


def device_part(lh, la, rho, tables, leg_table, start, quantiles, G, return_draws):
    """What HipContext.slate_summary returns for these rates (the fixtures already grouped by slate)."""
    tables = np.asarray(tables).astype(np.int64)
    leg_table, start = np.asarray(leg_table), np.asarray(start)
    J = start.size - 1
    index = np.repeat(np.arange(J), np.diff(start))
    tops = tables.reshape(tables.shape[0], -1).max(axis=1)[leg_table]
    r = leg_laws_from_rates(lh, la, rho, tables[leg_table], G)
    st = slate_stats(r, tops, index, J)
    # [S, K, J]: pmf, at_least, expected, mass
    v = np.concatenate([st["pmf"].transpose(0, 2, 1), st["at_least"].transpose(0, 2, 1), st["expected"][:, None, :],
                        st["mass"][:, None, :]], axis=1)
    out = MR.summarise(v, quantiles)
    out["leg_proba"] = r.mean(axis=0)
    if return_draws:
        out["draws"] = st["pmf"]
    return out


def predict_slate(m, data, legs, slate, G, quantiles):
    """The restatement of predict_slate (every array of its result), plus "leg_draws" [S, n, 8]."""
    lh, la = SR.rates(m, data)
    n = lh.shape[1]
    legs = [legs] * n if isinstance(legs, MK.Market) or (isinstance(legs, np.ndarray) and legs.ndim == 2) else list(legs)
    tables = np.stack([table_of(leg, G) for leg in legs])
    tops = tables.reshape(n, -1).max(axis=1)
    labels, index = (np.zeros(1, dtype=np.int64), np.zeros(n, dtype=np.int64)) if slate is None else \
        np.unique(np.asarray(slate, dtype=np.int64), return_inverse=True)
    index = index.reshape(n)
    J = labels.size
    r = leg_laws_from_rates(lh, la, np.asarray(m.corr_coef, dtype=np.float64), tables, G)
    st = slate_stats(r, tops, index, J)
    P = st["pmf"].shape[2] - 1
    out = {"n": n, "slates": labels, "size": np.bincount(index, minlength=J), "max_total": st["max_total"],
           "totals": np.arange(P + 1), "pmf_draws": st["pmf"], "leg_draws": r, "leg_proba": r.mean(axis=0)}
    for name in ("pmf", "at_least"):
        sm = MR.summarise(st[name], quantiles)   # [S, J, P+1] -> [J, P+1], [J, Q, P+1]
        out[name], out[f"{name}_sd"], out[f"{name}_quantile"] = sm["mean"], sm["sd"], sm["quantile"]
    sm = MR.summarise(st["expected"][:, :, None], quantiles)
    out["expected"], out["expected_sd"], out["expected_quantile"] = sm["mean"][:, 0], sm["sd"][:, 0], sm["quantile"][:, :, 0]
    out["mass"] = st["mass"].mean(axis=0)
    out["top_proba"] = out["pmf"][np.arange(J), st["max_total"]]
    ind = slate_stats(out["leg_proba"][None], tops, index, J)
    out["independent_pmf"], out["independent_at_least"] = ind["pmf"][0], ind["at_least"][0]
    return out
