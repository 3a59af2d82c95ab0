"""float64 numpy restatement of predict_in_play (bpl/inplay.py, csrc/dc_inplay.hip.h) by a
different route from the kernel: closed-form pmfs exp(k log mu - mu - lgamma(k+1)) (math.lgamma, no scipy) on the
FULL shifted grid of every (draw, fixture); Z by summing max(tau, 0) pmf pmf over a grid so wide that the dropped
tail is below 1e-18 (not the closed form 1 + sum (f - 1) u v); np.argsort(kind="stable"), np.cumsum and the
crossing rule written out.  It also returns the FLAG of every (market, quantile, fixture) cell: a cell is flagged
when some C_i lies within 1e-9 W of q W (the weights carry about 1e-13 relative error and a scan of S terms at
most S 2^-53: 1e-9 is wide of both), and then either neighbouring order statistic is accepted.  The gates of
section 25 are computed here too, from the restatement's own Z."""
import math

import numpy as np

import markets_ref as MR
import scores_ref as SR

EPS = 2.0 ** -53
FLAG_REL = 1e-9
TAIL = 1e-18


def lgf(k):
    """lgamma(k + 1) of integer counts (array or scalar)."""
    return np.vectorize(lambda v: math.lgamma(v + 1.0), otypes=[np.float64])(np.asarray(k))


def width(mu_max):
    """N such that the Poisson(mu_max) mass beyond N is below TAIL (geometric bound on the tail from N + 1 on)."""
    n = int(math.ceil(2.0 * mu_max)) + 2
    while True:
        logp = (n + 1) * math.log(max(mu_max, 1e-300)) - mu_max - math.lgamma(n + 2.0)
        if math.exp(logp) / (1.0 - mu_max / (n + 2.0)) < TAIL:
            return n
        n += 1


def pmf(mu, n):
    """[..., n + 1]: Pois(k; mu), k = 0..n, each from its closed form (mu > 0)."""
    k = np.arange(n + 1, dtype=np.float64)
    return np.exp(k * np.log(mu)[..., None] - mu[..., None] - lgf(k))


def tau_grid(lh, la, rho, nx, ny):
    """[S, nx + 1, ny + 1] the clipped tau factor of FINAL scores (x, y) from (0, 0), 1 off the four low cells."""
    f = np.ones(lh.shape + (nx + 1, ny + 1))
    f[:, 0, 0] = np.maximum(1.0 - rho * lh * la, 0.0)
    if ny >= 1:
        f[:, 0, 1] = np.maximum(1.0 + rho * lh, 0.0)
    if nx >= 1:
        f[:, 1, 0] = np.maximum(1.0 + rho * la, 0.0)
    if nx >= 1 and ny >= 1:
        f[:, 1, 1] = np.maximum(1.0 - rho, 0.0)
    return f


def one_fixture(lh, la, rho, a, b, t, W, G):
    """One fixture's draws: (val [S, K], lev [S], Z [S], A [S]) with A = sum |f - 1| u v over the reachable tau cells
    (what the closed form of Z adds up, for its rounding bound)."""
    r = 1.0 - t
    N = max(width(float(max(lh.max(), la.max()) * r)), G - a, G - b)   # (and every cell of the grid 0..G)
    u, v = pmf(lh * r, N), pmf(la * r, N)                      # remaining goals 0..N
    f = tau_grid(lh, la, rho, a + N, b + N)[:, a:, b:]          # final scores a..a+N, b..b+N
    p = f * u[:, :, None] * v[:, None, :]
    Z = p.sum(axis=(1, 2))
    A = (np.abs(f - 1.0) * u[:, :, None] * v[:, None, :])[:, :2, :2].sum(axis=(1, 2))
    nx, ny = G - a + 1, G - b + 1                               # cells on the grid 0..G
    val = np.einsum("kxy,sxy->sk", W[:, a:, b:], p[:, :nx, :ny]) / Z[:, None]
    with np.errstate(all="ignore"):
        pa = (a * np.log(lh * t) if a > 0 else 0.0) - lh * t - math.lgamma(a + 1.0)
        pb = (b * np.log(la * t) if b > 0 else 0.0) - la * t - math.lgamma(b + 1.0)
    return val, pa + pb + np.log(Z), Z, A


def closed_form_Z(lh, la, rho, a, b, t):
    """Z [S] as the kernel forms it: 1 + sum over the reachable tau cells of (f - 1) u_(x-a) v_(y-b)."""
    r = 1.0 - t
    u, v = pmf(lh * r, 1), pmf(la * r, 1)
    f = tau_grid(lh, la, rho, 1, 1)
    Z = np.ones_like(lh)
    for x in range(a, 2):
        for y in range(b, 2):
            Z = Z + (f[:, x, y] - 1.0) * u[:, x - a] * v[:, y - b]
    return Z


def weighted_quantiles(val, om, quantiles):
    """One (market, fixture): (quantile [Q], flag [Q], neighbours [Q, 2]) of values val [S] under weights om [S]."""
    S = val.size
    order = np.argsort(val, kind="stable")        # ties by draw index
    srt, C = val[order], np.cumsum(om[order])
    Wt = C[-1]
    q = np.asarray(quantiles, dtype=np.float64)
    out, flag, nb = np.empty(q.size), np.zeros(q.size, dtype=bool), np.empty((q.size, 2))
    for i, qi in enumerate(q):
        if qi >= 1.0:
            at = S - 1                             # the maximum, whatever the last weights are
        else:
            at = int(np.nonzero(C >= qi * Wt)[0][0])
            flag[i] = bool(np.any(np.abs(C - qi * Wt) <= FLAG_REL * Wt)) and qi > 0.0
        out[i] = srt[at]
        nb[i] = srt[max(at - 1, 0)], srt[min(at + 1, S - 1)]
    return out, flag, nb


def summarise(val, lev, quantiles, reweight=True, log_weights=None):
    """val [S, K, n], lev [S, n] -> the summaries, flags and the weights om [S, n]."""
    S, K, n = val.shape
    L = (lev if reweight else np.zeros_like(lev)) + (0.0 if log_weights is None else np.asarray(log_weights)[:, None])
    om = np.exp(L - L.max(axis=0))
    sw = om.sum(axis=0)
    mean = (om[:, None, :] * val).sum(axis=0) / sw
    sd = np.sqrt((om[:, None, :] * (val - mean) ** 2).sum(axis=0) / sw)
    q = np.asarray(quantiles, dtype=np.float64).reshape(-1)
    quant, flag, nb = np.empty((K, q.size, n)), np.zeros((K, q.size, n), dtype=bool), np.empty((K, q.size, n, 2))
    for k in range(K):
        for i in range(n):
            quant[k, :, i], flag[k, :, i], nb[k, :, i] = weighted_quantiles(val[:, k, i], om[:, i], q)
    mx = lev.max(axis=0)
    return {"mean": mean, "sd": sd, "quantile": quant, "flag": flag, "neighbours": nb, "weights": om, "L": L,
            "ess": sw ** 2 / (om ** 2).sum(axis=0), "log_evidence": mx + np.log(np.exp(lev - mx).mean(axis=0))}


def from_rates(lh, la, rho, a, b, t, W, G, quantiles, reweight=True, log_weights=None):
    S, n = lh.shape
    val, lev, Z, A = np.empty((S, W.shape[0], n)), np.empty((S, n)), np.empty((S, n)), np.empty((S, n))
    for i in range(n):
        val[:, :, i], lev[:, i], Z[:, i], A[:, i] = one_fixture(lh[:, i], la[:, i], rho, int(a[i]), int(b[i]),
                                                                  float(t[i]), W, G)
    out = summarise(val, lev, quantiles, reweight, log_weights)
    out.update(draws=val, draw_log_evidence=lev, Z=Z, A=A, lh=lh, la=la)
    return out


def predict_in_play(m, data, markets, G, quantiles, reweight=True, log_weights=None):
    lh, la = SR.rates(m, data)
    out = from_rates(lh, la, np.asarray(m.corr_coef, dtype=np.float64), np.asarray(data["home_goals"]),
                     np.asarray(data["away_goals"]), np.asarray(data["elapsed"], dtype=np.float64),
                     MR.weights_of(markets, G), G, quantiles, reweight, log_weights)
    out.update(a=np.asarray(data["home_goals"]), b=np.asarray(data["away_goals"]),
               t=np.asarray(data["elapsed"], dtype=np.float64), wmax=np.abs(MR.weights_of(markets, G)).reshape(
                   len(markets), -1).max(axis=1))
    return out


def device_part(lh, la, rho, home_goals, away_goals, elapsed, weights, quantiles, G, reweight, log_weights,
                return_draws):
    """What HipContext.inplay_summary returns for these rates."""
    r = from_rates(lh, la, rho, np.asarray(home_goals), np.asarray(away_goals), np.asarray(elapsed, dtype=np.float64),
                   np.asarray(weights, dtype=np.float64), G, quantiles, reweight, log_weights)
    keys = ("mean", "sd", "quantile", "ess", "log_evidence") + (("draws", "draw_log_evidence") if return_draws else ())
    return {k: r[k] for k in keys}


# ---- states for the tests
QS = (0.0, 0.05, 0.5, 0.95, 1.0)   # with S = 257 no q S is within 1e-6 of an integer but q = 0 and q = 1, which are exact


def with_states(data, G, seed, elapsed=None):
    """`data` with a state per fixture: the score drawn from {0, 1, 2, 3} (capped at G) and elapsed from (0, 1)."""
    rs = np.random.RandomState(seed)
    n = len(data["home_team"])
    d = dict(data)
    d["home_goals"] = np.minimum(rs.randint(0, 4, n), G)
    d["away_goals"] = np.minimum(rs.randint(0, 4, n), G)
    d["elapsed"] = rs.uniform(0.02, 0.98, n) if elapsed is None else np.full(n, float(elapsed))
    return d


def with_state_list(data, states):
    """`data` (at least len(states) fixtures) cut to one fixture per (a, b, t) of `states`."""
    n = len(states)
    d = {k: (v[:n] if isinstance(v, np.ndarray) else list(v)[:n]) for k, v in data.items()}
    d["home_goals"] = np.array([s[0] for s in states])
    d["away_goals"] = np.array([s[1] for s in states])
    d["elapsed"] = np.array([s[2] for s in states], dtype=np.float64)
    return d


# ---- the gates of DESIGN.md section 25, all from the restatement's own quantities
def gates(ref):
    """value [S, K, n], lev [S, n], mean / sd / quantile [K, n], ess / log_evidence [n]."""
    Z, A, val = ref["Z"], ref["A"], ref["draws"]
    S = val.shape[0]
    g = 1e-12 * np.maximum(1.0, ref["wmax"])                      # section 16's g, per market
    e_Z = EPS * (4.0 + 204.0 * A)                                 # the four-term closed form
    # the restatement's own Z, relative: per cell two closed-form pmfs (exponents of size <= 8 where the mass is, three
    # roundings each: a dozen relative roundings per pmf), two products, numpy's pairwise sum over <= 2^12 cells
    e_ref = 40.0 * EPS
    value = (g[None, :, None] * np.maximum(1.0, 1.0 / Z)[:, None, :]
             + np.abs(val) * (e_Z / Z + e_ref + 3.0 * EPS)[:, None, :])
    a, b, t, lh, la = ref["a"][None, :], ref["b"][None, :], ref["t"][None, :], ref["lh"], ref["la"]
    with np.errstate(all="ignore"):
        lt = np.where(t > 0.0, np.abs(np.log(np.where(t > 0.0, t, 1.0))), 0.0)
        scale = (lh * t + la * t + a * (np.abs(np.log(lh)) + lt) + b * (np.abs(np.log(la)) + lt) + lgf(a) + lgf(b)
                 + np.abs(np.log(Z)))
    lev = 48.0 * EPS * scale + 12.0 * EPS * (a + b) + e_Z / Z + e_ref
    # the weights: relative error delta from two log evidences (a draw's and the maximum's), the sum with the
    # log weight and the exp
    delta = 2.0 * (lev.max(axis=0) + EPS * np.abs(ref["L"]).max(axis=0)) + 4.0 * EPS      # [n]
    vmax = value.max(axis=0)                                                               # [K, n]
    R = val.max(axis=0) - val.min(axis=0)
    big = np.abs(val).max(axis=0)
    mean = vmax + 2.0 * delta * R + S * EPS * big
    with np.errstate(all="ignore"):
        by_sd = np.where(ref["sd"] > 0.0, 6.0 * delta * R * R / np.where(ref["sd"] > 0.0, ref["sd"], 1.0), np.inf)
    sd = 10.0 * vmax + np.minimum(np.sqrt(6.0 * delta) * R, by_sd) + S * EPS * R
    # ess = (sum w)^2 / sum w^2 <= S: three sums of S positive terms and the weights' delta, relative
    ess = ref["ess"] * (4.0 * delta + 3.0 * S * EPS)
    logev = lev.max(axis=0) + (S + 8.0) * EPS * (1.0 + np.abs(ref["log_evidence"]))
    return {"draws": value, "draw_log_evidence": lev, "mean": mean, "sd": sd, "quantile": vmax, "ess": ess,
            "log_evidence": logev}


def compare(got, ref, tag="", draws=True, flag_share=0.01):
    """`got` against the restatement within the gates; prints measured error over gate; returns the maxima."""
    G = gates(ref)
    keys = ["mean", "sd", "ess", "log_evidence"] + (["draws", "draw_log_evidence"] if draws else [])
    worst = {}
    for key in keys:
        assert got[key].shape == ref[key].shape, (key, got[key].shape, ref[key].shape)
        assert not np.isnan(got[key]).any(), key
        worst[key] = float((np.abs(got[key] - ref[key]) / G[key]).max())
    q, rq = got["quantile"], ref["quantile"]
    assert q.shape == rq.shape and not np.isnan(q).any()
    gate = G["quantile"][:, None, :] * np.ones_like(rq)
    err = np.abs(q - rq)
    near = np.minimum(err, np.abs(q[..., None] - ref["neighbours"]).min(axis=-1))
    err = np.where(ref["flag"], near, err)
    worst["quantile"] = float((err / gate).max(initial=0.0))
    flagged = int(ref["flag"].sum())
    for key, w in worst.items():
        print(f"{tag}: {key} error / gate {w:.3e}")
    print(f"{tag}: flagged cells {flagged} of {ref['flag'].size}")
    assert flagged <= flag_share * ref["flag"].size, (flagged, ref["flag"].size)
    for key, w in worst.items():
        assert w <= 1.0, (key, w)
    return worst
