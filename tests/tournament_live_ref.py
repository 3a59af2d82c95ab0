"""numpy float64 restatement of `simulate_tournament` with group matches in progress and weighted draws
(bpl/neutral_dixon_coles.py, csrc/dc_tournament_live.hip.h), operation for operation, for the
tests.  It is composed from the restatements already here, none of which is changed: tournament_ref's venue, rates
and redraw attempts, live_ref's weights, scan, resampling and conditional sampler, h2h_ref's rankings, knockout_ref's
extra-time ladder and allocation_ref's reading of the table.

Those restatements play simulation j on draw j mod S.  Here the draw of a simulation is whatever the resampling
selected, so they are handed the posterior tables GATHERED by simulation -- row j is the selected draw of simulation j,
N rows, j mod N = j -- and play every match on the right draw without knowing of it.  The group stage is restated here
(the others do not expose theirs): the ordinary fixtures as knockout_ref.first_round plays them, then the matches in
play from their states, the ranking, and the bracket by rank or through the table.  The knockout rounds are
knockout_ref.simulate_tournament's on that first round (its `first_round` is replaced for the call, the way
allocation_cases does it) or tournament_ref's redraw attempts.

Flags as in live_ref: a simulation is flagged when a walk comparison came within season_ref.FLAG_TOL of its boundary
(a shoot-out within knockout_ref.SHOOTOUT_TOL), or when its resampling target lies within inplay_ref.FLAG_REL W of
some C[s]."""
import numpy as np

import h2h_ref as H
import knockout_ref as K
import live_ref as LR
import season_ref as SR
import tournament_ref as TR

NO_PLAY = tuple(np.zeros(0, dtype=dt) for dt in (np.uint8, np.uint8, np.uint8, np.uint8, np.float64))


def oriented(inp, in_play):
    """The states in the home / away orientation: (home slot, away slot, on, home goals, away goals, swapped)."""
    p, q, gp, gq = (np.asarray(v, np.int64) for v in in_play[:4])
    hs, as_, on = TR.venue(p, q, inp["host"])
    swap = hs != p
    return hs, as_, on, np.where(swap, gq, gp), np.where(swap, gp, gq), swap


def log_rates(tables, inp, hs, as_, on):
    """(eh, ea) [S, L] of the matches hs v as_ (slots) in every draw: tournament_ref.rates before its exp."""
    ti = inp["team_idx"].astype(np.int64)
    h, a = ti[hs][None, :], ti[as_][None, :]
    s = np.arange(tables["attack"].shape[0])[:, None]
    eh = tables["attack"][s, h] - tables["defence"][s, a]
    ea = tables["attack"][s, a] - tables["defence"][s, h]
    eh = np.where(on[None, :], eh + (tables["home_attack"][s, h] - tables["away_defence"][s, a]), eh)
    ea = np.where(on[None, :], ea + (tables["away_attack"][s, a] - tables["home_defence"][s, h]), ea)
    cs = tables.get("confederation_strength")
    if cs is not None:
        conf = inp["conf"].astype(np.int64)
        dc = cs[s, conf[hs][None, :]] - cs[s, conf[as_][None, :]]
        eh, ea = eh + dc, ea - dc
    return eh, ea


def state_loglik(tables, inp, in_play):
    """l [S, L] as live_cup_loglik forms it: live_ref.state_loglik's terms on the tournament's log rates."""
    hs, as_, on, x, y, _ = oriented(inp, in_play)
    t = np.asarray(in_play[4], np.float64)
    EH, EA = log_rates(tables, inp, hs, as_, on)
    rho = tables["corr_coef"]
    S = rho.size
    out = np.zeros((S, hs.size))
    zero = np.zeros(S)
    for m in range(hs.size):
        eh, ea = EH[:, m], EA[:, m]
        lh, la = np.exp(eh), np.exp(ea)
        r = 1.0 - t[m]
        lhr, lar = lh * r, la * r
        u0, v0 = np.exp(-lhr), np.exp(-lar)
        c00, c01, c10, c11 = rho * -(lh * la), rho * lh, rho * la, rho * -1.0
        u1, v1 = u0 * lhr, v0 * lar
        hx0 = u0 if x[m] == 0 else zero
        hx1 = u1 if x[m] == 0 else (u0 if x[m] == 1 else zero)
        hy0 = v0 if y[m] == 0 else zero
        hy1 = v1 if y[m] == 0 else (v0 if y[m] == 1 else zero)
        Z = 1.0 + (((np.maximum(c00, -1.0) * (hx0 * hy0) + np.maximum(c01, -1.0) * (hx0 * hy1)) +
                    np.maximum(c10, -1.0) * (hx1 * hy0)) + np.maximum(c11, -1.0) * (hx1 * hy1))
        with np.errstate(all="ignore"):
            lt = np.log(t[m])
            pa = (float(x[m]) * (eh + lt) if x[m] > 0 else 0.0) - lh * t[m] - LR._LGF[x[m]]
            pb = (float(y[m]) * (ea + lt) if y[m] > 0 else 0.0) - la * t[m] - LR._LGF[y[m]]
        out[:, m] = (pa + pb) + np.log(Z)
    return out


def gathered(tables, s):
    """The tables with row j the draw of simulation j."""
    return {k: (None if v is None else v[s]) for k, v in tables.items()}


def first_round(gt, inp, key, in_play, flagged, head_to_head=False, pair_init=None):
    """The group stage on the gathered tables `gt`: knockout_ref.first_round's, with the matches in play after the
    ordinary fixtures and the bracket through inp["best_allocation"] when there is one.  Returns a dict: "bracket"
    [N, 2^R], "stage" [N, n] 0 / 1, "position" [N, n], "final_p" / "final_q" [N, L] (the final scores of the listed
    sides) and, under a table, "slot_counts" [groups, B]."""
    N, n = inp["num_simulations"], len(inp["team_idx"])
    nb = 1 << inp["rounds"]
    j = np.arange(N, dtype=np.int64)
    Lm = np.asarray(in_play[0]).size
    out = {"final_p": np.zeros((N, Lm), dtype=np.uint8), "final_q": np.zeros((N, Lm), dtype=np.uint8)}
    if inp["group"] is None:
        out.update(bracket=np.tile(inp["bracket"].astype(np.int64), (N, 1)), stage=np.ones((N, n), dtype=np.int64),
                   position=np.full((N, n), -1, dtype=np.int64))
        return out
    group = inp["group"].astype(np.int64)
    table = inp["table"]
    pts, gf, ga = (np.tile(table[:, c], (N, 1)) for c in range(3))
    init = np.zeros((n, n), dtype=np.int64) if pair_init is None else np.asarray(pair_init).astype(np.int64)
    pp, pg = np.tile(init >> 16, (N, 1, 1)), np.tile(init & 0xFFFF, (N, 1, 1))
    win, draw, loss = inp["points"]

    def book(rows, hs, as_, x, y):
        ph = np.where(x > y, win, np.where(x == y, draw, loss))
        pa = np.where(y > x, win, np.where(x == y, draw, loss))
        for acc, sl, v in ((pts, hs, ph), (pts, as_, pa), (gf, hs, x), (gf, as_, y), (ga, hs, y), (ga, as_, x)):
            np.add.at(acc, (rows, sl), v)
        np.add.at(pp, (rows, hs, as_), ph)
        np.add.at(pp, (rows, as_, hs), pa)
        np.add.at(pg, (rows, hs, as_), x)
        np.add.at(pg, (rows, as_, hs), y)

    fp, fq = inp["fix_p"].astype(np.int64), inp["fix_q"].astype(np.int64)
    F = fp.size
    if F:
        J2, F2 = np.meshgrid(j, np.arange(F), indexing="ij")
        rows, f = J2.ravel(), F2.ravel()
        hs, as_, on = TR.venue(fp[f], fq[f], inp["host"])
        x, y = K.play(gt, inp, key, rows, rows, hs, as_, on, f, 1.0, flagged)
        book(rows, hs, as_, x, y)
    if Lm:
        ohs, oas, oon, oa, ob, oswap = oriented(inp, in_play)
        t = np.asarray(in_play[4], np.float64)
        J2, M2 = np.meshgrid(j, np.arange(Lm), indexing="ij")
        rows, m = J2.ravel(), M2.ravel()
        hs, as_ = ohs[m], oas[m]
        ti = inp["team_idx"].astype(np.int64)
        ch = ca = None
        if inp["conf"] is not None:
            ch, ca = inp["conf"].astype(np.int64)[hs], inp["conf"].astype(np.int64)[as_]
        lh, la = TR.rates(gt, rows, ti[hs], ti[as_], oon[m], ch, ca)
        o0, o1 = SR.threefry_block(key, rows.astype(np.uint32), (F + m).astype(np.uint32))
        x, y, fl = LR.sample_conditional(lh, la, gt["corr_coef"][rows], oa[m], ob[m], 1.0 - t[m], SR.unit_open(o0),
                                         SR.unit_open(o1))
        np.logical_or.at(flagged, rows, fl)
        book(rows, hs, as_, x, y)
        out["final_p"] = np.where(oswap[m], y, x).reshape(N, Lm).astype(np.uint8)
        out["final_q"] = np.where(oswap[m], x, y).reshape(N, Lm).astype(np.uint8)
    r = H.words(key, N, n)
    better = H.overall_ahead(pts, gf, ga, r)
    if head_to_head:
        position = H.rank(pts, gf, ga, (pp << 16) | pg, r, group)
    else:
        position = (better & (group[:, None] == group[None, :])[None]).sum(axis=1)
    adv, bor = inp["advance"], inp["best_of_rest"]
    rest = position == adv
    rest_rank = (better & rest[:, :, None]).sum(axis=1)
    through = rest & (rest_rank < bor)
    slot = rest_rank
    alloc = inp.get("best_allocation")
    if alloc is not None:
        # the allocated fill, read from the mapping itself as allocation_ref.group_stage reads it
        names = list(inp["group_names"])
        slot = np.full((N, n), -1, dtype=np.int64)
        for sim in range(N):
            lanes = np.nonzero(through[sim])[0]
            order = alloc[tuple(names[g] for g in sorted(group[lanes]))]
            for tm in lanes:
                slot[sim, tm] = order.index(names[group[tm]])
        out["slot_counts"] = np.zeros((len(names), bor), dtype=np.int64)
        tj, tt = np.nonzero(through)
        np.add.at(out["slot_counts"], (group[tt], slot[tj, tt]), 1)
    code = np.where(position < adv, TR.MAX_GROUP * group[None, :] + position, np.where(through, 128 + slot, -1))
    code_pos = np.full(193, -1, dtype=np.int64)   # index 192: "no code"
    for b, c in enumerate(inp["bracket"].astype(np.int64)):
        hi, lo = c >> 8, c & 0xFF
        code_pos[128 + lo - 1 if hi == 0xFF else TR.MAX_GROUP * hi + lo - 1] = b
    bpos = code_pos[np.where(code >= 0, code, 192)]
    jj, ii = np.nonzero(bpos >= 0)
    br = np.full((N, nb), -1, dtype=np.int64)
    br[jj, bpos[jj, ii]] = ii
    assert (br >= 0).all()
    out.update(bracket=br, stage=(bpos >= 0).astype(np.int64), position=position)
    return out


def _redraw_rounds(gt, inp, key, br, stage, flagged):
    """tournament_ref.simulate_tournament's knockout rounds from the first round `br`; fills `stage`."""
    N, R = inp["num_simulations"], inp["rounds"]
    nb = 1 << R
    j = np.arange(N, dtype=np.int64)
    k0 = 0
    for rnd in range(R):
        M = nb >> (rnd + 1)
        p, q = br[:, 0::2], br[:, 1::2]
        win = p.copy()
        active = np.ones((N, M), dtype=bool)
        kk = k0 + np.arange(M)
        for t in range(TR.ATTEMPTS):
            jj, mm = np.nonzero(active)
            if jj.size == 0:
                break
            ctr = TR.KNOCKOUT_COUNTER | (kk[mm] << 5) | t
            hs, as_, x, y = TR._play(gt, inp, key, jj, jj, p[jj, mm], q[jj, mm], ctr, flagged)
            done = x != y
            win[jj[done], mm[done]] = np.where(x > y, hs, as_)[done]
            active[jj[done], mm[done]] = False
        stage[np.repeat(j, M).reshape(N, M), win] = rnd + 2
        br = win
        k0 += M


def simulate_tournament_live(tables, inp, key, in_play=None, reweight=True, log_weights_in=None, head_to_head=False,
                             pair_init=None):
    """The raw results of `simulate_tournament(..., in_play=..., log_weights=...)` for the checked inputs `inp`:
    simulate_tournament's ("stage_counts", "position_counts" with groups, "stage", "position", under the extra-time
    rule "decided" and "decided_counts", under a table "slot_counts"), plus "draw" [N], "in_play_home_goals" /
    "in_play_away_goals" [N, L] (listed order), "flagged" [N], "L", "L0" [S], "weights" (live_ref.weights' dict, or
    None without weights in force), "ess" and "log_evidence".  in_play: (slot p, slot q, goals of p, goals of q,
    elapsed) arrays [L] in the listed order, or None."""
    in_play = NO_PLAY if in_play is None else in_play
    N, n, R = inp["num_simulations"], len(inp["team_idx"]), inp["rounds"]
    S = tables["attack"].shape[0]
    Lm = np.asarray(in_play[0]).size
    j = np.arange(N, dtype=np.int64)
    flagged = np.zeros(N, dtype=bool)
    in_force = log_weights_in is not None or (reweight and Lm > 0)
    wt, L, L0 = None, np.zeros(S), np.zeros(S)
    if in_force:
        L, L0 = LR.log_weights(state_loglik(tables, inp, in_play), reweight, log_weights_in)
        wt = LR.weights(L, L0)
        s, flagged = LR.resample(wt["C"], N, key)
        flagged = flagged.copy()
    else:
        s = j % S
    gt = gathered(tables, s)
    g = first_round(gt, inp, key, in_play, flagged, head_to_head, pair_init)
    if inp["knockout_rule"] == "extra_time":
        def given(_tables, _inp, _key, fl, _h2h=False, _pair=None):
            return g["bracket"], g["stage"].copy(), g["position"]
        saved, K.first_round = K.first_round, given
        try:
            out = K.simulate_tournament(gt, inp, key, head_to_head, pair_init)
        finally:
            K.first_round = saved
        flagged = flagged | out["flagged"]
    else:
        stage = g["stage"].copy()
        _redraw_rounds(gt, inp, key, g["bracket"], stage, flagged)
        idx = np.broadcast_to(np.arange(n), (N, n))
        stage_counts = np.zeros((n, R + 2), dtype=np.int64)
        np.add.at(stage_counts, (idx, stage), 1)
        out = {"stage_counts": stage_counts, "stage": stage.astype(np.uint8), "position": g["position"]}
        if inp["group"] is not None:
            pc = np.zeros((n, TR.MAX_GROUP), dtype=np.int64)
            np.add.at(pc, (idx, g["position"]), 1)
            out["position_counts"] = pc
    if "slot_counts" in g:
        out["slot_counts"] = g["slot_counts"]
    out.update(flagged=flagged, draw=s.astype(np.int32), in_play_home_goals=g["final_p"], in_play_away_goals=g["final_q"],
               L=L, L0=L0, weights=wt, ess=float(S) if wt is None else float(wt["ess"]),
               log_evidence=(float("nan") if Lm else 0.0) if wt is None else float(wt["log_evidence"]))
    return out
