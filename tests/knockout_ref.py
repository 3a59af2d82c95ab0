"""numpy float64 restatement of `simulate_tournament(knockout_rule="extra_time")` (bpl/neutral_dixon_coles.py,
csrc/dc_knockout.hip.h), operation for operation, for the tests: the group stage and its first-round bracket
(restated here from tournament_ref / h2h_ref's helpers, which do not expose the bracket), then every knockout tie
by the new rule -- one or two legs, away goals, extra time at scaled rates, the shoot-out.  A simulation is
flagged when a walk of a block that was actually played came within season_ref.FLAG_TOL of its boundary, or a
shoot-out between unequal strengths had |u - P| < SHOOTOUT_TOL: the two places where exp's last bit can change a
result."""
import numpy as np

import h2h_ref as H
from season_ref import sample_scorelines, threefry_block, unit_open
from tournament_ref import KNOCKOUT_COUNTER, MAX_GROUP, rates, venue

SHOOTOUT_TOL = 1e-12
LEG1, LEG2, EXTRA_TIME, SHOOTOUT = 0, 1, 2, 3            # the block t of counter 0x40000000 | k << 5 | t
NORMAL, AWAY_GOALS, IN_EXTRA_TIME, BY_SHOOTOUT = 0, 1, 2, 3   # how a tie was decided


def play(tables, inp, key, j, s, hs, as_, on, ctr, scale, flagged):
    """Scorelines (x home, y away) of matches of simulations j on draws s (1-d arrays): slot hs at home against
    slot as_, on-venue or neutral, both rates times `scale`, on block (j, ctr)."""
    ti = inp["team_idx"].astype(np.int64)
    conf = inp["conf"]
    ch = ca = None
    if conf is not None:
        ch, ca = conf.astype(np.int64)[hs], conf.astype(np.int64)[as_]
    lh, la = rates(tables, s, ti[hs], ti[as_], on, ch, ca)
    lh, la = lh * scale, la * scale
    o0, o1 = threefry_block(key, j.astype(np.uint32), np.asarray(ctr, dtype=np.int64).astype(np.uint32))
    x, y, fl = sample_scorelines(lh, la, tables["corr_coef"][s], unit_open(o0), unit_open(o1))
    np.logical_or.at(flagged, j, fl)
    return x, y


def first_round(tables, inp, key, flagged, head_to_head=False, pair_init=None):
    """The group stage: (bracket [N, 2^R] slots, stage [N, n] 0 / 1, position [N, n] or -1 without groups)."""
    N, n = inp["num_simulations"], len(inp["team_idx"])
    nb = 1 << inp["rounds"]
    j = np.arange(N, dtype=np.int64)
    s = j % tables["attack"].shape[0]
    if inp["group"] is None:
        return (np.tile(inp["bracket"].astype(np.int64), (N, 1)), np.ones((N, n), dtype=np.int64),
                np.full((N, n), -1, dtype=np.int64))
    group = inp["group"].astype(np.int64)
    table = inp["table"]
    pts, gf, ga = (np.tile(table[:, c], (N, 1)) for c in range(3))
    init = np.zeros((n, n), dtype=np.int64) if pair_init is None else np.asarray(pair_init).astype(np.int64)
    pp, pg = np.tile(init >> 16, (N, 1, 1)), np.tile(init & 0xFFFF, (N, 1, 1))
    fp, fq = inp["fix_p"].astype(np.int64), inp["fix_q"].astype(np.int64)
    if fp.size:
        J2, F2 = np.meshgrid(j, np.arange(fp.size), indexing="ij")
        rows, f = J2.ravel(), F2.ravel()
        hs, as_, on = venue(fp[f], fq[f], inp["host"])
        x, y = play(tables, inp, key, rows, s[rows], hs, as_, on, f, 1.0, flagged)
        win, draw, loss = inp["points"]
        ph = np.where(x > y, win, np.where(x == y, draw, loss))
        pa = np.where(y > x, win, np.where(x == y, draw, loss))
        for acc, sl, v in ((pts, hs, ph), (pts, as_, pa), (gf, hs, x), (gf, as_, y), (ga, hs, y), (ga, as_, x)):
            np.add.at(acc, (rows, sl), v)
        if head_to_head:
            np.add.at(pp, (rows, hs, as_), ph)
            np.add.at(pp, (rows, as_, hs), pa)
            np.add.at(pg, (rows, hs, as_), x)
            np.add.at(pg, (rows, as_, hs), y)
    r = H.words(key, N, n)
    better = H.overall_ahead(pts, gf, ga, r)
    if head_to_head:
        position = H.rank(pts, gf, ga, (pp << 16) | pg, r, group)
    else:
        position = (better & (group[:, None] == group[None, :])[None]).sum(axis=1)
    adv, bor = inp["advance"], inp["best_of_rest"]
    rest = position == adv
    rest_rank = (better & rest[:, :, None]).sum(axis=1)
    code = np.where(position < adv, MAX_GROUP * group[None, :] + position,
                    np.where(rest & (rest_rank < bor), 128 + rest_rank, -1))
    code_pos = np.full(193, -1, dtype=np.int64)   # index 192: "no code"
    for b, c in enumerate(inp["bracket"].astype(np.int64)):
        hi, lo = c >> 8, c & 0xFF
        code_pos[128 + lo - 1 if hi == 0xFF else MAX_GROUP * hi + lo - 1] = b
    bpos = code_pos[np.where(code >= 0, code, 192)]
    jj, ii = np.nonzero(bpos >= 0)
    br = np.full((N, nb), -1, dtype=np.int64)
    br[jj, bpos[jj, ii]] = ii
    assert (br >= 0).all()
    return br, (bpos >= 0).astype(np.int64), position


def simulate_tournament(tables, inp, key, head_to_head=False, pair_init=None):
    """The raw results of `simulate_tournament(knockout_rule="extra_time")` for the checked inputs `inp` (the dict
    of _tournament_inputs): "stage_counts" [n, R + 2], "position_counts" [n, 8] (with groups), "decided_counts"
    [R, 4], "stage" and "position" [N, n], "decided" [N, 2^R - 1], "flagged" [N]; and for the tests' own checks
    "level" [N, 2^R - 1] (the aggregate was level after the legs) and "away" [N, 2^R - 1, 2] (the away goals of
    the first- / second-listed side in a two-legged tie, else 0)."""
    N, n, R = inp["num_simulations"], len(inp["team_idx"]), inp["rounds"]
    nb = 1 << R
    j = np.arange(N, dtype=np.int64)
    s = j % tables["attack"].shape[0]
    flagged = np.zeros(N, dtype=bool)
    br, stage, position = first_round(tables, inp, key, flagged, head_to_head, pair_init)
    legs, scale, strength = inp["legs"], inp["extra_time_scale"], inp["strength"]
    decided_all = np.zeros((N, nb - 1), dtype=np.uint8)
    level_all = np.zeros((N, nb - 1), dtype=bool)
    away_all = np.zeros((N, nb - 1, 2), dtype=np.int64)
    k0 = 0
    for rnd in range(R):
        M = nb >> (rnd + 1)
        J = np.repeat(j, M)
        P, Q = br[:, 0::2].ravel(), br[:, 1::2].ravel()
        ctr = np.tile(KNOCKOUT_COUNTER | ((k0 + np.arange(M)) << 5), N)
        away = np.zeros((N * M, 2), dtype=np.int64)
        if legs[rnd] == 2:
            on = np.ones(N * M, dtype=bool)
            x1, y1 = play(tables, inp, key, J, s[J], P, Q, on, ctr | LEG1, 1.0, flagged)
            x2, y2 = play(tables, inp, key, J, s[J], Q, P, on, ctr | LEG2, 1.0, flagged)
            gp, gq = x1 + y2, y1 + x2
            q_home = np.ones(N * M, dtype=bool)
            away[:, 0], away[:, 1] = y2, y1
        else:
            hs, as_, on = venue(P, Q, inp["host"])
            x, y = play(tables, inp, key, J, s[J], hs, as_, on, ctr | LEG1, 1.0, flagged)
            q_home = hs == Q
            gp, gq = np.where(q_home, y, x), np.where(q_home, x, y)
        level = gp == gq
        decided = np.where(level, -1, NORMAL)
        win = np.where(gp > gq, P, Q)
        if legs[rnd] == 2 and inp["away_goals"]:
            ag = level & (away[:, 0] != away[:, 1])
            decided[ag] = AWAY_GOALS
            win[ag] = np.where(away[:, 0] > away[:, 1], P, Q)[ag]
        i = np.nonzero(decided < 0)[0]
        if i.size:
            xe, ye = play(tables, inp, key, J[i], s[J[i]], np.where(q_home[i], Q[i], P[i]),
                          np.where(q_home[i], P[i], Q[i]), on[i], ctr[i] | EXTRA_TIME, scale, flagged)
            tp, tq = gp[i] + np.where(q_home[i], ye, xe), gq[i] + np.where(q_home[i], xe, ye)
            d = tp != tq
            decided[i[d]] = IN_EXTRA_TIME
            win[i[d]] = np.where(tp > tq, P[i], Q[i])[d]
        i = np.nonzero(decided < 0)[0]
        if i.size:
            o0, _ = threefry_block(key, J[i].astype(np.uint32), (ctr[i] | SHOOTOUT).astype(np.uint32))
            u = unit_open(o0)
            sp, sq = strength[P[i]], strength[Q[i]]
            prob = 1.0 / (1.0 + np.exp(-(sp - sq)))
            decided[i] = BY_SHOOTOUT
            win[i] = np.where(u < prob, P[i], Q[i])
            np.logical_or.at(flagged, J[i], (sp != sq) & (np.abs(u - prob) < SHOOTOUT_TOL))
        assert (decided >= 0).all()
        win = win.reshape(N, M)
        stage[np.repeat(j, M).reshape(N, M), win] = rnd + 2
        decided_all[:, k0:k0 + M] = decided.reshape(N, M)
        level_all[:, k0:k0 + M] = level.reshape(N, M)
        away_all[:, k0:k0 + M] = away.reshape(N, M, 2)
        br = win
        k0 += M
    idx = np.arange(n)
    stage_counts = np.zeros((n, R + 2), dtype=np.int64)
    np.add.at(stage_counts, (np.broadcast_to(idx, (N, n)), stage), 1)
    decided_counts = np.zeros((R, 4), dtype=np.int64)
    k0 = 0
    for rnd in range(R):
        M = nb >> (rnd + 1)
        decided_counts[rnd] = np.bincount(decided_all[:, k0:k0 + M].ravel(), minlength=4)
        k0 += M
    out = {"stage_counts": stage_counts, "decided_counts": decided_counts, "stage": stage.astype(np.uint8),
           "position": position, "decided": decided_all, "flagged": flagged, "level": level_all, "away": away_all}
    if inp["group"] is not None:
        pc = np.zeros((n, MAX_GROUP), dtype=np.int64)
        np.add.at(pc, (np.broadcast_to(idx, (N, n)), position), 1)
        out["position_counts"] = pc
    return out
