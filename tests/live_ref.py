"""numpy float64 restatement of `simulate_season` with matches in progress and weighted draws (bpl/base.py,
csrc/dc_live.hip.h), operation for operation, for the tests: the states' log likelihood per
draw, the weights and their fixed-association scan, systematic resampling, the conditional two-walk sampler and the
ranked table.  It reuses season_ref's threefry blocks and walks and h2h_ref's rankings (neither is changed).  Only
`exp` and `log` may differ from the device in their last bit: a simulation is flagged when a walk comparison came
within season_ref.FLAG_TOL of its boundary, or when its resampling target lies within inplay_ref.FLAG_REL W of some
C[s] (the scan moves by far less than that)."""
import math

import numpy as np

import h2h_ref as HR
import inplay_ref as IR
import season_ref as SR

RESAMPLE_COUNTER = 0x20000000
THREADS = 256          # live_weights' workgroup: the scan's segments
LIVE_MAX_GOALS = 63
_LGF = np.array([math.lgamma(k + 1.0) for k in range(LIVE_MAX_GOALS + 1)])


def rates(attack, defence, home_advantage, s, h, a):
    """Full-match rates of draws s for fixtures (h, a) (broadcast index arrays), formed as dc_season forms them."""
    edge = home_advantage[s] if home_advantage.ndim == 1 else home_advantage[s, h]
    return np.exp((attack[s, h] - defence[s, a]) + edge), np.exp(attack[s, a] - defence[s, h])


def state_loglik(attack, defence, home_advantage, rho, h, a, x, y, t):
    """l [S, L]: log Pois(x; lh t) + log Pois(y; la t) + log Z per draw and state, as live_loglik forms it."""
    S = attack.shape[0]
    h, a, x, y = (np.asarray(v, np.int64) for v in (h, a, x, y))
    t = np.asarray(t, np.float64)
    out = np.zeros((S, h.size))
    for m in range(h.size):
        ha = home_advantage if home_advantage.ndim == 1 else home_advantage[:, h[m]]
        eh = attack[:, h[m]] - defence[:, a[m]] + ha
        ea = attack[:, a[m]] - defence[:, h[m]]
        lh, la = np.exp(eh), np.exp(ea)
        r = 1.0 - t[m]
        lhr, lar = lh * r, la * r
        u0, v0 = np.exp(-lhr), np.exp(-lar)
        c00, c01, c10, c11 = rho * -(lh * la), rho * lh, rho * la, rho * -1.0
        u1, v1 = u0 * lhr, v0 * lar
        zero = np.zeros(S)
        hx0 = u0 if x[m] == 0 else zero
        hx1 = u1 if x[m] == 0 else (u0 if x[m] == 1 else zero)
        hy0 = v0 if y[m] == 0 else zero
        hy1 = v1 if y[m] == 0 else (v0 if y[m] == 1 else zero)
        Z = 1.0 + (((np.maximum(c00, -1.0) * (hx0 * hy0) + np.maximum(c01, -1.0) * (hx0 * hy1)) +
                    np.maximum(c10, -1.0) * (hx1 * hy0)) + np.maximum(c11, -1.0) * (hx1 * hy1))
        with np.errstate(all="ignore"):
            lt = np.log(t[m])
            pa = (float(x[m]) * (eh + lt) if x[m] > 0 else 0.0) - lh * t[m] - _LGF[x[m]]
            pb = (float(y[m]) * (ea + lt) if y[m] > 0 else 0.0) - la * t[m] - _LGF[y[m]]
        out[:, m] = (pa + pb) + np.log(Z)
    return out


def log_weights(l, reweight, lw):
    """(L [S], L0 [S]): L0 the states' part summed in m order, L = (L0 if reweight) + (lw if given)."""
    L0 = np.zeros(l.shape[0])
    for m in range(l.shape[1]):
        L0 = L0 + l[:, m]
    L = (L0 if reweight else np.zeros_like(L0)) + (0.0 if lw is None else np.asarray(lw, np.float64))
    return L, L0


def _segments(S):
    per = (S + THREADS - 1) // THREADS
    return [(min(i * per, S), min(min(i * per, S) + per, S)) for i in range(THREADS)]


def _ordered_total(parts):
    """(total, before [THREADS]): the parts added left to right from 0.0, and what stands before each."""
    run = np.cumsum(np.concatenate([[0.0], parts]))   # (np.cumsum adds sequentially; 0.0 + x = x)
    return run[-1], run[:-1]


def weights(L, L0):
    """live_weights: {"omega", "C", "W", "ess", "log_evidence"} with the kernel's association -- thread-owned
    contiguous segments summed sequentially, segment totals left to right, C = segment start + own partial sum."""
    S = L.size
    om = np.exp(L - L.max())
    m0 = L0.max()
    e = np.exp(L0 - m0)
    seg = _segments(S)
    part = np.array([np.cumsum(om[lo:hi])[-1] if hi > lo else 0.0 for lo, hi in seg])
    sq = np.array([np.cumsum(om[lo:hi] * om[lo:hi])[-1] if hi > lo else 0.0 for lo, hi in seg])
    ev = np.array([np.cumsum(e[lo:hi])[-1] if hi > lo else 0.0 for lo, hi in seg])
    W, before = _ordered_total(part)
    sww, _ = _ordered_total(sq)
    et, _ = _ordered_total(ev)
    C = np.empty(S)
    for (lo, hi), b in zip(seg, before):
        if hi > lo:
            C[lo:hi] = b + np.cumsum(om[lo:hi])
    assert C[-1] == W
    return {"omega": om, "C": C, "W": W, "ess": W * W / sww, "log_evidence": m0 + np.log(et / S)}


def resample(C, N, key):
    """(s [N], flagged [N]): systematic resampling on the scan C under the call's key."""
    o0, _ = SR.threefry_block(key, np.zeros(1, np.uint32), np.full(1, RESAMPLE_COUNTER, np.uint32))
    U = SR.unit_open(o0)[0]
    W = C[-1]
    step = W / float(N)
    target = np.minimum((np.arange(N, dtype=np.float64) + U) * step, W)
    count = np.searchsorted(C, target, side="left")          # #{s : C[s] < target}
    s = np.minimum(count, C.size - 1)
    near = np.minimum(np.abs(C[s] - target), np.abs(C[np.maximum(count - 1, 0)] - target))
    return s, near <= IR.FLAG_REL * W


def _tau(lh, la, rho):
    return (np.maximum(1.0 - lh * la * rho, 0.0), np.maximum(1.0 + lh * rho, 0.0),
            np.maximum(1.0 + la * rho, 0.0), np.maximum(1.0 - rho, 0.0))


def _head(lh, la, rho, a, b, r):
    """The conditional sampler's constants, term for term as sample_conditional writes them."""
    t00, t01, t10, t11 = _tau(lh, la, rho)
    lhr, lar = lh * r, la * r
    q0 = np.exp(-lar)
    q1 = q0 * lar
    one = np.ones_like(lh)
    c0 = np.where(b == 0, 1.0 + (t00 - 1.0) * q0 + (t01 - 1.0) * q1, np.where(b == 1, 1.0 + (t01 - 1.0) * q0, one))
    c1 = np.where(b == 0, 1.0 + (t10 - 1.0) * q0 + (t11 - 1.0) * q1, np.where(b == 1, 1.0 + (t11 - 1.0) * q0, one))
    p0 = np.exp(-lhr)
    p1 = p0 * lhr
    Z = np.where(a == 0, 1.0 + p0 * (c0 - 1.0) + p1 * (c1 - 1.0), np.where(a == 1, 1.0 + p0 * (c1 - 1.0), one))
    return (t00, t01, t10, t11), lhr, lar, q0, c0, c1, p0, Z


def sample_conditional(lh, la, rho, a, b, r, u1, u2):
    """FINAL scorelines of matches standing a : b with the fraction r to play (1-d arrays): (x, y, flagged)."""
    lh, la, rho, r, u1, u2 = (np.asarray(v, np.float64).ravel() for v in (lh, la, rho, r, u1, u2))
    a, b = np.asarray(a, np.int64).ravel(), np.asarray(b, np.int64).ravel()
    (t00, t01, t10, t11), lhr, lar, q0, c0, c1, p0, Z = _head(lh, la, rho, a, b, r)
    one = np.ones_like(lh)
    flag = np.zeros(lh.shape, dtype=bool)
    # home: the weight c1 falls on the step that reaches x = 1 (a = 0, k = 1); p * 1.0 = p elsewhere
    k = SR._walk(u1 * Z, p0.copy(), np.where(a == 0, p0 * c0, np.where(a == 1, p0 * c1, p0)), lhr,
                 np.where(a == 0, c1, one), flag)
    x = np.minimum(a + k, 255)
    cx = np.where(x == 0, c0, np.where(x == 1, c1, 1.0))
    f0 = np.where(x == 0, t00, np.where(x == 1, t10, 1.0))
    f1 = np.where(x == 0, t01, np.where(x == 1, t11, 1.0))
    tau0 = np.where(b == 0, f0, np.where(b == 1, f1, one))
    tau1 = np.where(b == 0, f1, one)
    k = SR._walk(u2 * cx, q0.copy(), q0 * tau0, lar, tau1, flag)
    return x, np.minimum(b + k, 255), flag


def conditional_pmf(lh, la, rho, a, b, t, G):
    """[G + 1, G + 1] exact conditional probabilities of the FINAL score (zero below the current score) for scalar
    rates, from the sampler's own constants: tau(x, y) u_(x-a) v_(y-b) / Z."""
    arr = lambda v: np.array([v], dtype=np.float64)   # noqa: E731
    r = 1.0 - t
    (t00, t01, t10, t11), lhr, lar, q0, _, _, p0, Z = _head(arr(lh), arr(la), arr(rho), np.array([a]), np.array([b]), arr(r))
    tau = np.ones((G + 1, G + 1))
    tau[0, 0], tau[1, 0] = t00[0], t10[0]
    if G >= 1:
        tau[0, 1], tau[1, 1] = t01[0], t11[0]
    out = np.zeros((G + 1, G + 1))
    u = p0[0]
    for x in range(a, G + 1):
        if x > a:
            u = u * lhr[0] / (x - a)
        v = q0[0]
        for y in range(b, G + 1):
            if y > b:
                v = v * lar[0] / (y - b)
            out[x, y] = tau[x, y] * u * v / Z[0]
    return out


def simulate_season_live(attack, defence, home_advantage, corr_coef, home_idx, away_idx, in_play, table_idx, table,
                         points, num_simulations, key, reweight=True, log_weights_in=None, head_to_head=False,
                         pair_init=None):
    """What `simulate_season(..., in_play=..., log_weights=...)` returns (without "teams"), with every optional
    output, plus "flagged" [num_simulations], "L", "L0" [S] and "weights" (the dict of `weights`, or None without
    weights in force).  in_play: (home idx, away idx, home goals, away goals, elapsed) arrays [L]."""
    attack, defence = np.asarray(attack, np.float64), np.asarray(defence, np.float64)
    ha, rho_s = np.asarray(home_advantage, np.float64), np.asarray(corr_coef, np.float64)
    ih, ia, ix, iy = (np.asarray(v, np.int64) for v in in_play[:4])
    it = np.asarray(in_play[4], np.float64)
    F, Lm = np.asarray(home_idx).size, ih.size
    h = np.concatenate([np.asarray(home_idx, np.int64), ih])
    a = np.concatenate([np.asarray(away_idx, np.int64), ia])
    table_idx = np.asarray(table_idx, np.int64)
    table = np.asarray(table, np.int64).reshape(table_idx.size, 3)
    n, nf, N, S = table_idx.size, h.size, int(num_simulations), attack.shape[0]
    slot = np.full(attack.shape[1], -1)
    slot[table_idx] = np.arange(n)
    hs, as_ = slot[h], slot[a]
    j = np.arange(N, dtype=np.int64)
    flagged = np.zeros(N, dtype=bool)
    in_force = log_weights_in is not None or (reweight and Lm > 0)
    wt, L, L0 = None, np.zeros(S), np.zeros(S)
    if in_force:
        L, L0 = log_weights(state_loglik(attack, defence, ha, rho_s, ih, ia, ix, iy, it), reweight, log_weights_in)
        wt = weights(L, L0)
        s, flagged = resample(wt["C"], N, key)
    else:
        s = j % S
    x = np.zeros((N, nf), dtype=np.int64)
    y = np.zeros((N, nf), dtype=np.int64)
    if nf:
        S2, F2 = np.meshgrid(s, np.arange(nf), indexing="ij")
        lh, la = rates(attack, defence, ha, S2, h[F2], a[F2])
        o0, o1 = SR.threefry_block(key, j[:, None].astype(np.uint32), np.arange(nf, dtype=np.uint32)[None, :])
        u1, u2 = SR.unit_open(o0), SR.unit_open(o1)
        rho = rho_s[S2]
        if F:
            xs, ys, fl = SR.sample_scorelines(lh[:, :F], la[:, :F], rho[:, :F], u1[:, :F], u2[:, :F])
            x[:, :F], y[:, :F] = xs.reshape(N, F), ys.reshape(N, F)
            flagged = flagged | fl.reshape(N, F).any(axis=1)
        if Lm:
            A2, B2, R2 = (np.broadcast_to(v, (N, Lm)) for v in (ix, iy, 1.0 - it))
            xs, ys, fl = sample_conditional(lh[:, F:], la[:, F:], rho[:, F:], A2, B2, R2, u1[:, F:], u2[:, F:])
            x[:, F:], y[:, F:] = xs.reshape(N, Lm), ys.reshape(N, Lm)
            flagged = flagged | fl.reshape(N, Lm).any(axis=1)
    win, draw, loss = points
    tp, gf, ga = (np.tile(table[:, c], (N, 1)) for c in range(3))
    if nf:
        rows = np.broadcast_to(j[:, None], x.shape)
        H, A = np.broadcast_to(hs, x.shape), np.broadcast_to(as_, x.shape)
        ph = np.where(x > y, win, np.where(x == y, draw, loss))
        pa = np.where(y > x, win, np.where(x == y, draw, loss))
        for acc, sl, v in ((tp, H, ph), (tp, A, pa), (gf, H, x), (gf, A, y), (ga, H, y), (ga, A, x)):
            np.add.at(acc, (rows, sl), v)
    gd = gf - ga
    if head_to_head:
        position, _ = HR.season_positions(hs, as_, x, y, table, points, key, pair_init)
    else:
        position = HR.overall_ahead(tp, gf, ga, HR.words(key, N, n)).sum(axis=1)
    keep = ~flagged
    counts = np.zeros((n, n), dtype=np.int64)
    np.add.at(counts, (np.broadcast_to(np.arange(n), (N, n))[keep], position[keep]), 1)
    return {
        "points": tp.astype(np.int32), "position": position.astype(np.uint8), "draw": s.astype(np.int32),
        "home_goals": x[:, :F].astype(np.uint8), "away_goals": y[:, :F].astype(np.uint8),
        "in_play_home_goals": x[:, F:].astype(np.uint8), "in_play_away_goals": y[:, F:].astype(np.uint8),
        "flagged": flagged, "unflagged_counts": counts, "points_sum": tp[keep].sum(axis=0),
        "gd_sum": gd[keep].sum(axis=0), "L": L, "L0": L0, "weights": wt,
        "ess": float(S) if wt is None else float(wt["ess"]),
        "log_evidence": (float("nan") if Lm else 0.0) if wt is None else float(wt["log_evidence"]),
    }
