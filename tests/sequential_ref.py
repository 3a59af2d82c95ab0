"""float64 numpy restatement of sequential_scores (bpl/sequential.py, csrc/dc_sequential.hip.h; DESIGN.md
section 17) by a different route from the kernels: the FULL log-likelihood matrix (loglik_ref.ll_matrix),
PSIS with a full sort (loglik_ref.psis / gpdfit) and the full scoreline grids (scores_ref.draw_probs).  Also
`narrowed`, which makes a loglik_ref.hand_model posterior informative enough for the weights to be worth
testing: the raw hand models are prior-wide, and their weights collapse onto one draw after the first block."""
import copy

import numpy as np
from scipy.special import logsumexp

import loglik_ref as LR
import scores_ref as SR


def narrowed(m, f):
    """A copy of the hand model `m` whose draws are pulled towards their mean over the draws by the factor
    f: every float array whose first axis is the draws."""
    out = copy.copy(m)
    S = np.shape(m.corr_coef)[0]
    for name, v in vars(m).items():
        if isinstance(v, np.ndarray) and v.dtype.kind == "f" and v.ndim >= 1 and v.shape[0] == S:
            mean = v.mean(axis=0, keepdims=True)
            setattr(out, name, mean + f * (v - mean))
    return out


def relabel(block):
    values, index = np.unique(np.asarray(block).astype(np.int64), return_inverse=True)
    return values, index.reshape(-1).astype(np.int64)


def psis_row(r, r_eff=1.0):
    """One block's log ratios over the draws -> (lw, k, ess, L)."""
    r = np.asarray(r, dtype=np.float64)
    S = r.size
    if not r.max() > -np.inf:                       # a dead block
        return np.full(S, -np.inf), np.inf, 0.0, 0
    if r.max() == r.min():                          # constant ratios have no tail
        lw = np.full(S, -np.log(S) + 0.0)
        return lw, 0.0, float(np.exp(-logsumexp(2 * lw))), 0
    with np.errstate(all="ignore"):                 # (its own elpd, of ll = -r, is not used)
        _, k, L, lw = LR.psis(-r, r_eff, return_lw=True)
    return lw, k, float(np.exp(-logsumexp(2 * lw))), L


def block_sums(ll, index, B):
    """A[b, s] = the sum of ll[s, n] over the fixtures of block b."""
    A = np.zeros((B, ll.shape[0]))
    for b in range(B):
        A[b] = ll[:, index == b].sum(axis=1)
    return A


def log_ratios(A):
    R = np.zeros_like(A)
    for b in range(1, A.shape[0]):
        R[b] = R[b - 1] + A[b - 1]
    return R


def weights(R, r_eff=1.0):
    rows = [psis_row(R[b], r_eff) for b in range(R.shape[0])]
    return {"log_weights": np.stack([r[0] for r in rows]), "pareto_k": np.array([r[1] for r in rows]),
            "ess": np.array([r[2] for r in rows]), "tail_len": np.array([r[3] for r in rows], dtype=np.int32)}


def weighted(ll, p, lw, index):
    """(elpd_i [n], P [n, 3]) of fixtures with ll [S, n] and per-draw probabilities p [S, n, 3]."""
    with np.errstate(all="ignore"):
        elpd = logsumexp(lw[index].T + ll, axis=0)
        P = np.einsum("ns,snk->nk", np.exp(lw[index]), p)
    return elpd, P


def _se_mean(v):
    if v.size < 2:
        return 0.0
    return float(np.std(v, ddof=1) / np.sqrt(v.size)) if np.isfinite(v).all() else np.inf


def scores(m, data, block, r_eff=1.0, G=15, k_threshold=0.7):
    """The restatement of sequential_scores(return_weights=True), plus "block_sums" [B, S], "ll" [S, n] and
    "p_draws" [S, n, 3]."""
    ll = LR.ll_matrix(m, data)
    values, index = relabel(block)
    B = values.size
    A = block_sums(ll, index, B)
    w = weights(log_ratios(A), r_eff)
    lh, la = SR.rates(m, data)
    p = SR.draw_probs(lh, la, np.asarray(m.corr_coef, dtype=np.float64), G)
    elpd_i, P = weighted(ll, p, w["log_weights"], index)
    o = SR.outcome_of(data["home_goals"], data["away_goals"])
    n_block = np.bincount(index, minlength=B)
    out = {"n": o.size, "outcome": o, "outcome_proba": P, "elpd_i": elpd_i, "elpd": float(elpd_i.sum()),
           "block": index, "block_values": values, "n_block": n_block, "block_sums": A, "ll": ll, "p_draws": p, **w}
    per_block = {"elpd": elpd_i}
    for name, v in zip(("log_score", "brier", "rps"), SR.rules(P, o)):
        out[f"{name}_i"], out[name], out[f"{name}_se"] = v, float(v.mean()), _se_mean(v)
        per_block[name] = v
    for name, v in per_block.items():
        out[f"{name}_block"] = np.array([v[index == b].mean() for b in range(B)])
    out["reliable"] = out["pareto_k"] <= k_threshold
    stale = np.nonzero(out["pareto_k"] > k_threshold)[0]
    out["refit_from"] = int(values[stale[0]]) if stale.size else None
    return out

