"""numpy float64 restatement of `simulate_season(..., playoffs=...)` (bpl/base.py, csrc/dc_playoff.hip.h),
operation for operation, for the tests: the league from season_ref (threefry blocks, `unit_open`, the exact
sampler and its flag) and h2h_ref (both rankings), then the bracket by knockout_ref's ladder with the base
classes' team-level rates and the seed-driven orientation.  A simulation is flagged exactly as knockout_ref
flags one: a walk of a block that was actually played (league fixture or play-off leg) came within
season_ref.FLAG_TOL of its boundary, or a shoot-out between unequal strengths had |u - P| < SHOOTOUT_TOL."""
import numpy as np

import h2h_ref as H
import season_ref as SR
from knockout_ref import (AWAY_GOALS, BY_SHOOTOUT, EXTRA_TIME, IN_EXTRA_TIME, LEG1, LEG2, NORMAL, SHOOTOUT,  # noqa: F401
                          SHOOTOUT_TOL)
from season_ref import sample_scorelines, threefry_block, unit_open

KNOCKOUT_COUNTER = 0x40000000
GUEST, BYE = 0x8000, 0xFFFF      # bracket codes
NO_SLOT = -1
DECIDED_BYE = 255


def leg(model, key, j, s, h, a, on, ctr, scale, flagged):
    """Scorelines (x home, y away) of legs of simulations j on draws s (1-d arrays): model team h at home against
    a, with (on) or without the home-advantage term, both rates times `scale`, on block (j, ctr)."""
    att, dfn, ha, rho = (np.asarray(v, np.float64) for v in model)
    eh = att[s, h] - dfn[s, a]
    edge = ha[s] if ha.ndim == 1 else ha[s, h]
    eh = np.where(on, eh + edge, eh)
    lh = np.exp(eh) * scale
    la = np.exp(att[s, a] - dfn[s, h]) * scale
    o0, o1 = threefry_block(key, j.astype(np.uint32), np.asarray(ctr, dtype=np.int64).astype(np.uint32))
    x, y, fl = sample_scorelines(lh, la, rho[s], unit_open(o0), unit_open(o1))
    np.logical_or.at(flagged, j, fl)
    return x, y


def resolve(codes, position, n):
    """The first round's slots [N, 2^R] from the bracket codes and the positions [N, n] (NO_SLOT: a bye)."""
    N = position.shape[0]
    pos_slot = np.argsort(position, axis=1)          # the positions are a permutation: slot at each position
    br = np.full((N, len(codes)), NO_SLOT, dtype=np.int64)
    for b, c in enumerate(int(v) for v in codes):
        if c == BYE:
            continue
        br[:, b] = n + (c & 0x7FFF) if c & GUEST else pos_slot[:, c]
    return br


def play_bracket(model, po, key, slot_model, position, flagged):
    """The bracket after the rankings `position` [N, n]: ("stage" [N, n + g], "decided" [N, 2^R - 1])."""
    N, n = position.shape
    R, nt = po["rounds"], len(slot_model)
    nb = 1 << R
    S = np.asarray(model[0]).shape[0]
    j = np.arange(N, dtype=np.int64)
    s = j % S
    slot_model = np.asarray(slot_model, dtype=np.int64)
    seed = np.concatenate([position.astype(np.int64), np.tile(np.arange(n, nt), (N, 1))], axis=1)
    br = resolve(po["bracket"], position, n)
    stage = np.zeros((N, nt), dtype=np.int64)
    jj, bb = np.nonzero(br != NO_SLOT)
    stage[jj, br[jj, bb]] = 1
    legs, scale, strength = po["legs"], po["extra_time_scale"], po["strength"]
    decided_all = np.full((N, nb - 1), DECIDED_BYE, dtype=np.uint8)
    k0 = 0
    for rnd in range(R):
        M = nb >> (rnd + 1)
        e0, e1 = br[:, 0::2], br[:, 1::2]
        win_all = np.where(e0 == NO_SLOT, e1, e0)            # a bye: the other entry (or NO_SLOT) goes through
        jm, mm = np.nonzero((e0 != NO_SLOT) & (e1 != NO_SLOT))
        if jm.size:
            a0, a1 = e0[jm, mm], e1[jm, mm]
            first_better = seed[jm, a0] < seed[jm, a1]
            Q, P = np.where(first_better, a0, a1), np.where(first_better, a1, a0)
            J, sj = jm, s[jm]
            mP, mQ = slot_model[P], slot_model[Q]
            ctr = KNOCKOUT_COUNTER | ((k0 + mm) << 5)
            two = legs[rnd] == 2
            neutral = bool((po["neutral_mask"] >> rnd) & 1)
            if two:
                on = np.ones(J.size, dtype=bool)
                x1, y1 = leg(model, key, J, sj, mP, mQ, on, ctr | LEG1, 1.0, flagged)
                x2, y2 = leg(model, key, J, sj, mQ, mP, on, ctr | LEG2, 1.0, flagged)
                gp, gq = x1 + y2, y1 + x2
                q_home = np.ones(J.size, dtype=bool)
                away_p, away_q = y2, y1
            else:
                q_home = np.full(J.size, not neutral)
                on = np.full(J.size, not neutral)
                x, y = leg(model, key, J, sj, np.where(q_home, mQ, mP), np.where(q_home, mP, mQ), on, ctr | LEG1, 1.0,
                           flagged)
                gp, gq = np.where(q_home, y, x), np.where(q_home, x, y)
            level = gp == gq
            decided = np.where(level, -1, NORMAL)
            win = np.where(gp > gq, P, Q)
            if two and po["away_goals"]:
                ag = level & (away_p != away_q)
                decided[ag] = AWAY_GOALS
                win[ag] = np.where(away_p > away_q, P, Q)[ag]
            i = np.nonzero(decided < 0)[0]
            if i.size:
                xe, ye = leg(model, key, J[i], sj[i], np.where(q_home[i], mQ[i], mP[i]), np.where(q_home[i], mP[i], mQ[i]),
                             on[i], ctr[i] | EXTRA_TIME, scale, flagged)
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
            win_all[jm, mm] = win
            decided_all[jm, k0 + mm] = decided
        jj, mm2 = np.nonzero(win_all != NO_SLOT)
        stage[jj, win_all[jj, mm2]] = rnd + 2
        br = win_all
        k0 += M
    return stage.astype(np.uint8), decided_all


def simulate_season(m, season_inputs, po, key, head_to_head=False, pair_init=None):
    """The league of season_ref.simulate_season (its dict, "position" replaced by the head-to-head order when
    asked) plus the play-off's raw results: "stage_counts" [n + g, R + 2], "decided_counts" [R, 4],
    "playoff_stage" [N, n + g], "playoff_decided" [N, 2^R - 1]; "flagged" covers league and bracket.
    season_inputs: (home, away, table_idx, table, points, N) of `_season_inputs`; po: `playoff_inputs`' dict."""
    h, a, table_idx, table, points, N = season_inputs
    model = (m.attack, m.defence, m.home_advantage, m.corr_coef)
    out = SR.simulate_season(*model, h, a, table_idx, table, points, N, key)
    n = len(table_idx)
    if head_to_head:
        slot = np.full(np.asarray(m.attack).shape[1], -1, dtype=np.int64)
        slot[np.asarray(table_idx, np.int64)] = np.arange(n)
        position, _ = H.season_positions(slot[np.asarray(h, np.int64)], slot[np.asarray(a, np.int64)], out["home_goals"],
                                         out["away_goals"], table, points, key, pair_init)
        out["position"] = position.astype(np.uint8)
        counts = np.zeros((n, n), dtype=np.int64)
        np.add.at(counts, (np.broadcast_to(np.arange(n), (N, n)), position), 1)
        out["position_proba"] = counts / N
    flagged = out["flagged"].copy()
    slot_model = np.concatenate([np.asarray(table_idx, np.int64), po["guests"].astype(np.int64)])
    stage, decided = play_bracket(model, po, key, slot_model, out["position"].astype(np.int64), flagged)
    R, nt = po["rounds"], len(slot_model)
    stage_counts = np.zeros((nt, R + 2), dtype=np.int64)
    np.add.at(stage_counts, (np.broadcast_to(np.arange(nt), (N, nt)), stage.astype(np.int64)), 1)
    decided_counts = np.zeros((R, 4), dtype=np.int64)
    k0 = 0
    for rnd in range(R):
        M = (1 << R) >> (rnd + 1)
        decided_counts[rnd] = np.bincount(decided[:, k0:k0 + M].ravel(), minlength=256)[:4]
        k0 += M
    out.update(stage_counts=stage_counts, decided_counts=decided_counts, playoff_stage=stage,
               playoff_decided=decided, flagged=flagged)
    return out
