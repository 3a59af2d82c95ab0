"""float64 numpy restatement of power-scaling sensitivity (csrc/dc_sensitivity.hip.h, bpl/sensitivity.py), one
quantity and one weight row at a time, with plain loops, as DESIGN.md section 33 defines it: the stable sort, the
running sum of the weights in sorted order, the two passes of the cumulative Jensen-Shannon divergence written out
interval by interval.  The rows are smoothed by `sequential_ref.psis_row`."""
import math

import numpy as np

import sequential_ref as QR

KEYS = ("cjs_sq", "mean", "sd")


def shift_parts(x, w):
    """(B, F, R) of draws x under weights w (any positive scale): the forward pass's normaliser, and the
    normalised divergences of the forward and of the survival pass."""
    x = np.asarray(x, dtype=np.float64) + 0.0
    w = np.asarray(w, dtype=np.float64)
    S = x.size
    order = np.argsort(x, kind="stable")
    xs, ws = x[order], w[order]
    W = 0.0
    for i in range(S):
        W += ws[i]
    js_f = b_f = js_r = b_r = 0.0
    run = 0.0
    for i in range(1, S):
        run += ws[i - 1]
        d = xs[i] - xs[i - 1]
        p, q = i / S, run / W
        for survival in (False, True):
            if survival:
                p, q = 1.0 - p, max(1.0 - q, 0.0)
            m = (p + q) / 2.0
            t = (p * math.log2(p / m) if p > 0.0 else 0.0) + (q * math.log2(q / m) if q > 0.0 else 0.0)
            if survival:
                js_r += d * t
                b_r += d * (p + q)
            else:
                js_f += d * t
                b_f += d * (p + q)
    return b_f, max(js_f, 0.0) / b_f, max(js_r, 0.0) / b_r


def cjs_sq(x, w):
    """max(F, R); NaN for a non-finite draw or for draws that are all equal."""
    x = np.asarray(x, dtype=np.float64)
    if not np.all(np.isfinite(x)) or x.min() == x.max():
        return math.nan
    _, f, r = shift_parts(x, w)
    return max(f, r)


def weighted_moments(x, w):
    """(mean, sd) under weights w: sd = sqrt(sum w (x - mean)^2 / sum w)."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    with np.errstate(all="ignore"):
        sw = float(np.sum(w))
        mean = float(np.sum(w * x)) / sw
        return mean, math.sqrt(float(np.sum(w * (x - mean) ** 2)) / sw)


def weighted_shift(values, log_ratios, r_eff=1.0):
    """`values` [S, Q], `log_ratios` [R, S] -> the dict of the device call: cjs_sq, mean, sd [R, Q] and the rows'
    log_weights [R, S], pareto_k, ess [R], tail_len int32 [R]."""
    values = np.asarray(values, dtype=np.float64)
    log_ratios = np.asarray(log_ratios, dtype=np.float64)
    out = QR.weights(log_ratios, r_eff)
    R, Q = log_ratios.shape[0], values.shape[1]
    for nm in KEYS:
        out[nm] = np.empty((R, Q))
    for r in range(R):
        w = np.exp(out["log_weights"][r])
        for j in range(Q):
            out["cjs_sq"][r, j] = cjs_sq(values[:, j], w)
            out["mean"][r, j], out["sd"][r, j] = weighted_moments(values[:, j], w)
    return out


def backend(values, log_ratios, r_eff=1.0, workspace_bytes=0):
    """A stand-in for the device call of bpl.sensitivity (same signature, same keys)."""
    return weighted_shift(values, log_ratios, r_eff)


def power_ratios(log_prior, log_likelihood, delta):
    """[4, S]: prior-, prior+, likelihood-, likelihood+ for alpha- = 1 / (1 + delta), alpha+ = 1 + delta."""
    lo, hi = 1.0 / (1.0 + delta), 1.0 + delta
    lp, ll = np.asarray(log_prior, dtype=np.float64), np.asarray(log_likelihood, dtype=np.float64)
    return np.stack([(lo - 1.0) * lp, (hi - 1.0) * lp, (lo - 1.0) * ll, (hi - 1.0) * ll])


def powerscale(values, log_prior, log_likelihood, delta=0.01, r_eff=1.0):
    """{"prior", "likelihood"} [Q] plus the weighted_shift dict of the four rows."""
    out = weighted_shift(values, power_ratios(log_prior, log_likelihood, delta), r_eff)
    cjs = np.sqrt(out["cjs_sq"])
    out["cjs"] = cjs
    out["prior"] = (cjs[0] + cjs[1]) / (2.0 * math.log2(1.0 + delta))
    out["likelihood"] = (cjs[2] + cjs[3]) / (2.0 * math.log2(1.0 + delta))
    return out


def gaussian_case(S, seed=0, Q_extra=1):
    """Draws x ~ N(0, 1) with l = -x^2 / 2 and `Q_extra` independent columns: values [S, 1 + Q_extra], l [S]."""
    rs = np.random.RandomState(seed)
    x = rs.normal(size=S)
    return np.column_stack([x] + [rs.normal(size=S) for _ in range(Q_extra)]), -0.5 * x * x


def log_jacobian(sites, z):
    """The log-Jacobian of the unconstraining transforms over draws z [S, D]: z itself for an Exp site (std_*),
    -softplus(z) - softplus(-z) for a Sigmoid site (corr_coef_raw, u); `sites` as `_latent_sites()` gives them."""
    z = np.asarray(z, dtype=np.float64)
    out = np.zeros(z.shape[0])
    at = 0
    for name, shape in sites:
        size = int(np.prod(shape))
        for j in range(at, at + size):
            if name.startswith("std_"):
                out += z[:, j]
            elif name in ("corr_coef_raw", "u"):
                out += -np.logaddexp(0.0, z[:, j]) - np.logaddexp(0.0, -z[:, j])
        at += size
    return out
