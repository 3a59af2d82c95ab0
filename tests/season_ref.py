"""numpy float64 restatement of `simulate_season` (bpl/base.py, csrc/dc_season.hip.h), operation for
operation, for the tests: threefry-2x32-20 blocks, the exact two-walk scoreline sampler and the ranked
table.  Only `exp` may differ from the device in its last bit; every simulation in which some
comparison of the walks came within FLAG_TOL of its boundary is flagged, as the only place where
that difference can change a draw."""
import numpy as np

FLAG_TOL = 1e-12
TIEBREAK_COUNTER = 0x80000000
_R0, _R1 = (13, 15, 26, 6), (17, 29, 16, 24)


def threefry_block(key, c0, c1):
    """Threefry-2x32-20 of the counter pairs (c0, c1) (broadcast arrays) under key = (hi, lo)."""
    c0, c1 = np.broadcast_arrays(np.asarray(c0, dtype=np.uint32), np.asarray(c1, dtype=np.uint32))
    k = (int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF)
    ks = (k[0], k[1], k[0] ^ k[1] ^ 0x1BD11BDA)
    x0 = c0 + np.uint32(ks[0])
    x1 = c1 + np.uint32(ks[1])
    for g in range(5):
        for r in (_R1 if g & 1 else _R0):
            x0 = x0 + x1
            x1 = (x1 << np.uint32(r)) | (x1 >> np.uint32(32 - r))
            x1 = x1 ^ x0
        x0 = x0 + np.uint32(ks[(g + 1) % 3])
        x1 = x1 + np.uint32((ks[(g + 2) % 3] + g + 1) & 0xFFFFFFFF)
    return x0, x1


def unit_open(o):
    """u = (o + 0.5) 2^-32: exact in float64, inside (0, 1)."""
    return (o.astype(np.float64) + 0.5) * 2.0 ** -32


def _walk(th, p, acc, rate, w1, flag):
    """First k with th < sum_{i<=k} p_i w_i (w_1 = w1, w_k = 1 for k >= 2, p_k = p_{k-1} rate / k),
    capped at 255; flags comparisons within FLAG_TOL."""
    k = np.zeros(th.shape, dtype=np.int64)
    flag |= np.abs(th - acc) < FLAG_TOL
    active = ~(th < acc)
    step = 0
    while active.any():
        step += 1
        i = np.nonzero(active)[0]
        p[i] = p[i] * rate[i] / float(step)
        acc[i] = acc[i] + (p[i] * w1[i] if step == 1 else p[i])
        k[i] = step
        flag[i] |= np.abs(th[i] - acc[i]) < FLAG_TOL
        active[i] = ~(th[i] < acc[i]) & (step < 255)
    return k


def sample_scorelines(lh, la, rho, u1, u2):
    """Scorelines drawn exactly from max(tau, 0) Pois(x; lh) Pois(y; la) / Z (1-d arrays).
    Returns (x, y, flagged)."""
    lh, la, rho, u1, u2 = (np.asarray(v, dtype=np.float64).ravel() for v in (lh, la, rho, u1, u2))
    t00 = np.maximum(1.0 - lh * la * rho, 0.0)
    t01 = np.maximum(1.0 + lh * rho, 0.0)
    t10 = np.maximum(1.0 + la * rho, 0.0)
    t11 = np.maximum(1.0 - rho, 0.0)
    q0 = np.exp(-la)
    q1 = q0 * la
    c0 = 1.0 + (t00 - 1.0) * q0 + (t01 - 1.0) * q1
    c1 = 1.0 + (t10 - 1.0) * q0 + (t11 - 1.0) * q1
    p0 = np.exp(-lh)
    p1 = p0 * lh
    Z = 1.0 + p0 * (c0 - 1.0) + p1 * (c1 - 1.0)
    flag = np.zeros(lh.shape, dtype=bool)
    x = _walk(u1 * Z, p0.copy(), p0 * c0, lh, c1, flag)
    cx = np.where(x == 0, c0, np.where(x == 1, c1, 1.0))
    tau0 = np.where(x == 0, t00, np.where(x == 1, t10, 1.0))
    tau1 = np.where(x == 0, t01, np.where(x == 1, t11, 1.0))
    y = _walk(u2 * cx, q0.copy(), q0 * tau0, la, tau1, flag)
    return x, y, flag


def scoreline_edges(lh, la, rho, max_goals):
    """The sampler's inverse-CDF boundaries for scalar rates, from the walks' own cumulative sums:
    home [max_goals + 2] (x is drawn when home[x] <= u1 < home[x + 1]) and away [max_goals + 1,
    max_goals + 2] (y given x when away[x, y] <= u2 < away[x, y + 1])."""
    t = {(0, 0): max(1.0 - lh * la * rho, 0.0), (0, 1): max(1.0 + lh * rho, 0.0),
         (1, 0): max(1.0 + la * rho, 0.0), (1, 1): max(1.0 - rho, 0.0)}
    q0 = np.exp(-la)
    q1 = q0 * la
    c = [1.0 + (t[0, 0] - 1.0) * q0 + (t[0, 1] - 1.0) * q1, 1.0 + (t[1, 0] - 1.0) * q0 + (t[1, 1] - 1.0) * q1]
    p0 = np.exp(-lh)
    Z = 1.0 + p0 * (c[0] - 1.0) + p0 * lh * (c[1] - 1.0)
    G = max_goals
    home = np.zeros(G + 2)
    away = np.zeros((G + 1, G + 2))
    p, acc = p0, 0.0
    for x in range(G + 1):
        if x:
            p = p * lh / x
        acc = acc + p * (c[x] if x <= 1 else 1.0)
        home[x + 1] = acc / Z
        cx = c[x] if x <= 1 else 1.0
        q, acc_y = q0, 0.0
        for y in range(G + 1):
            if y:
                q = q * la / y
            acc_y = acc_y + q * (t[x, y] if x <= 1 and y <= 1 else 1.0)
            away[x, y + 1] = acc_y / cx
    return home, away


def simulate_season(attack, defence, home_advantage, corr_coef, home_idx, away_idx, table_idx, table,
                    points, num_simulations, key):
    """The dict `simulate_season` returns (without "teams"), with every optional output, plus
    "flagged" [num_simulations]: simulations with a comparison within FLAG_TOL of its boundary.
    table_idx: the table's model indices in slot order; table: [n, 3] (points, GF, GA)."""
    attack, defence = np.asarray(attack, np.float64), np.asarray(defence, np.float64)
    ha, rho_s = np.asarray(home_advantage, np.float64), np.asarray(corr_coef, np.float64)
    h, a = np.asarray(home_idx, np.int64), np.asarray(away_idx, np.int64)
    table_idx = np.asarray(table_idx, np.int64)
    table = np.asarray(table, np.int64).reshape(table_idx.size, 3)
    n, nf, N, S = table_idx.size, h.size, int(num_simulations), attack.shape[0]
    slot = np.full(attack.shape[1], -1)
    slot[table_idx] = np.arange(n)
    hs, as_ = slot[h], slot[a]
    j = np.arange(N, dtype=np.int64)
    s = j % S
    pts = np.tile(table[:, 0], (N, 1))
    gf = np.tile(table[:, 1], (N, 1))
    ga = np.tile(table[:, 2], (N, 1))
    x = np.zeros((N, nf), dtype=np.int64)
    y = np.zeros((N, nf), dtype=np.int64)
    flagged = np.zeros(N, dtype=bool)
    if nf:
        S2, F2 = np.meshgrid(s, np.arange(nf), indexing="ij")
        H2, A2 = h[F2], a[F2]
        edge = ha[S2] if ha.ndim == 1 else ha[S2, H2]
        lh = np.exp((attack[S2, H2] - defence[S2, A2]) + edge)
        la = np.exp(attack[S2, A2] - defence[S2, H2])
        o0, o1 = threefry_block(key, j[:, None].astype(np.uint32), np.arange(nf, dtype=np.uint32)[None, :])
        xs, ys, fl = sample_scorelines(lh, la, rho_s[S2], unit_open(o0), unit_open(o1))
        x, y = xs.reshape(N, nf), ys.reshape(N, nf)
        flagged = fl.reshape(N, nf).any(axis=1)
        win, draw, loss = points
        ph = np.where(x > y, win, np.where(x == y, draw, loss))
        pa = np.where(y > x, win, np.where(x == y, draw, loss))
        rows = np.repeat(j, nf).reshape(N, nf)
        for acc, sl, v in ((pts, hs, ph), (pts, as_, pa), (gf, hs, x), (gf, as_, y), (ga, hs, y), (ga, as_, x)):
            np.add.at(acc, (rows, np.broadcast_to(sl, (N, nf))), v)
    gd = gf - ga
    r, _ = threefry_block(key, j[:, None].astype(np.uint32), (TIEBREAK_COUNTER | np.arange(n)).astype(np.uint32)[None, :])
    r = r.astype(np.int64)
    idx = np.arange(n)
    # better[j, k, i]: slot k is ahead of slot i
    P, G, F, R = (v[:, :, None] for v in (pts, gd, gf, r))
    Pi, Gi, Fi, Ri = (v[:, None, :] for v in (pts, gd, gf, r))
    better = (P > Pi) | ((P == Pi) & ((G > Gi) | ((G == Gi) & ((F > Fi) | ((F == Fi) & (
        (R > Ri) | ((R == Ri) & (idx[:, None] < idx[None, :]))))))))
    position = better.sum(axis=1)
    counts = np.zeros((n, n), dtype=np.int64)
    np.add.at(counts, (np.broadcast_to(idx, (N, n)), position), 1)
    return {
        "position_proba": counts / N,
        "expected_points": pts.sum(axis=0) / N,
        "expected_goal_difference": gd.sum(axis=0) / N,
        "points": pts.astype(np.int32),
        "position": position.astype(np.uint8),
        "home_goals": x.astype(np.uint8),
        "away_goals": y.astype(np.uint8),
        "flagged": flagged,
    }
