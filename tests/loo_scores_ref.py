"""float64 numpy restatement of loo_scores (bpl/loo_scores.py, csrc/dc_loo.hip.h) by a different route from the
kernel's: the log-likelihood matrix of tests/loglik_ref.py, PSIS of each column with its normalised log weights
(loglik_ref.psis(..., return_lw=True)), the FULL scoreline grid of every (draw, fixture) from tests/scores_ref.py
(outcome triangles by scores_ref.draw_probs, marginals by summing the grid along one axis), and the -inf limit
spelled out: uniform weights over the draws with ll = -inf."""
import numpy as np

import loglik_ref as LR
import scores_ref as SR


def narrow(m, sd=0.05):
    """`m` with attack and defence rescaled from hand_model's sd 0.3 to `sd`: Pareto k well below 0.7, where the
    default spread reaches about 1.6."""
    m.attack = np.asarray(m.attack) * (sd / 0.3)
    m.defence = np.asarray(m.defence) * (sd / 0.3)
    return m


def weights(ll_i, r_eff=1.0):
    """One fixture's draws -> (w [S] summing to 1, elpd_loo, k, L)."""
    ll_i = np.asarray(ll_i, dtype=np.float64)
    elpd, k, L, lw = LR.psis(ll_i, r_eff, return_lw=True)
    if lw is None:   # some draw is -inf: the limit of the definition
        dead = ~(ll_i > -np.inf)
        return dead / dead.sum(), elpd, k, L
    return np.exp(lw), elpd, k, L


def pit_pair(marginal, count):
    """(lower, upper) of a weighted marginal [G+1] at an actual count (which may exceed G)."""
    c = np.concatenate([[0.0], np.cumsum(marginal)])
    g1 = marginal.size
    return c[min(int(count), g1)], c[min(int(count) + 1, g1)]


def device_part(ll, lh, la, rho, home_goals, away_goals, G, r_eff=1.0):
    """What HipContext.loo_scores returns for this log-likelihood matrix [S, n] and these rates."""
    S, n = ll.shape
    rho = np.asarray(rho, dtype=np.float64)
    p = SR.draw_probs(lh, la, rho, G)
    out = {"elpd_loo": np.empty(n), "pareto_k": np.empty(n), "ess": np.empty(n), "tail_len": np.empty(n, dtype=np.int32),
           "proba": np.empty((n, 3)), "proba_in_sample": p.mean(axis=0), "pit": np.empty((n, 4))}
    for i in range(n):
        w, out["elpd_loo"][i], out["pareto_k"][i], out["tail_len"][i] = weights(ll[:, i], r_eff)
        out["ess"][i] = 1.0 / np.sum(w * w)
        out["proba"][i] = w @ p[:, i]
        q = SR.grid(lh[:, i:i + 1], la[:, i:i + 1], rho, G)[:, 0]      # [S, G+1, G+1], axis 1 the home goals
        out["pit"][i, :2] = pit_pair(w @ q.sum(axis=2), home_goals[i])
        out["pit"][i, 2:] = pit_pair(w @ q.sum(axis=1), away_goals[i])
    return out


def scores(m, data, G, r_eff=1.0):
    """The restatement of loo_scores' device outputs for a model and its data, in fixture order."""
    lh, la = SR.rates(m, data)
    return device_part(LR.ll_matrix(m, data), lh, la, np.asarray(m.corr_coef, dtype=np.float64),
                       np.asarray(data["home_goals"]), np.asarray(data["away_goals"]), G, r_eff)
