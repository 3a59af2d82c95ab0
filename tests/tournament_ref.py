"""numpy float64 restatement of `simulate_tournament` (bpl/neutral_dixon_coles.py,
csrc/dc_tournament.hip.h), operation for operation, for the tests: the venue-form rates, the group
matches, the group and best-of-rest ranking, the bracket and the knockout rounds with their redrawn
level attempts.  Scorelines come from season_ref's threefry blocks and exact sampler; a simulation is
flagged when any comparison of any of its walks (group matches and every knockout attempt) came
within season_ref.FLAG_TOL of its boundary, the only place where exp's last bit can change a draw."""
import numpy as np

import season_ref as SR

KNOCKOUT_COUNTER = 0x40000000
ATTEMPTS = 32
MAX_GROUP = 8


def venue(p, q, host):
    """(home slot, away slot, on) of matches between slots p and q (listed order): with exactly one
    host the host is at home (on = 1), else the listed order at a neutral venue (on = 0)."""
    hp, hq = host[p].astype(bool), host[q].astype(bool)
    swap = hq & ~hp
    return np.where(swap, q, p), np.where(swap, p, q), hp != hq


def rates(tables, s, h, a, on, ch=None, ca=None):
    """Home and away rates of draws s, model indices h / a (broadcast arrays): the venue-aware form."""
    att, dfn = tables["attack"], tables["defence"]
    eh = att[s, h] - dfn[s, a]
    ea = att[s, a] - dfn[s, h]
    eh = np.where(on, eh + (tables["home_attack"][s, h] - tables["away_defence"][s, a]), eh)
    ea = np.where(on, ea + (tables["away_attack"][s, a] - tables["home_defence"][s, h]), ea)
    cs = tables.get("confederation_strength")
    if cs is not None:
        dc = cs[s, ch] - cs[s, ca]
        eh = eh + dc
        ea = ea - dc
    return np.exp(eh), np.exp(ea)


def model_tables(m):
    """The posterior tables of a neutral-family model as `simulate_tournament` takes them."""
    out = {nm: np.asarray(getattr(m, nm), np.float64) for nm in
           ("attack", "defence", "home_attack", "away_attack", "home_defence", "away_defence", "corr_coef")}
    cs = getattr(m, "confederation_strength", None)
    out["confederation_strength"] = None if cs is None else np.asarray(cs, np.float64)
    return out


def _play(tables, inp, key, j, s, p, q, ctr, flagged):
    """Scorelines of matches (j, p, q) (1-d arrays) on block (j, ctr): (home slot, away slot, x, y)."""
    hs, as_, on = venue(p, q, inp["host"])
    ti = inp["team_idx"].astype(np.int64)
    conf = inp["conf"]
    ch = ca = None
    if conf is not None:
        ch, ca = conf.astype(np.int64)[hs], conf.astype(np.int64)[as_]
    lh, la = rates(tables, s, ti[hs], ti[as_], on, ch, ca)
    o0, o1 = SR.threefry_block(key, j.astype(np.uint32), np.asarray(ctr, dtype=np.int64).astype(np.uint32))
    x, y, fl = SR.sample_scorelines(lh, la, tables["corr_coef"][s], SR.unit_open(o0), SR.unit_open(o1))
    np.logical_or.at(flagged, j, fl)
    return hs, as_, x, y


def simulate_tournament(tables, inp, key):
    """The raw results of `simulate_tournament` for the checked inputs `inp` (the dict of
    NeutralDixonColesMatchPredictor._tournament_inputs): "stage_counts" [n, R + 2], "position_counts"
    [n, 8] (with groups), "stage" and "position" [N, n] (position -1 without groups), and "flagged" [N]."""
    N, n, R = inp["num_simulations"], len(inp["team_idx"]), inp["rounds"]
    nb = 1 << R
    S = tables["attack"].shape[0]
    j = np.arange(N, dtype=np.int64)
    s = j % S
    flagged = np.zeros(N, dtype=bool)
    stage = np.ones((N, n), dtype=np.int64)
    position = np.full((N, n), -1, dtype=np.int64)
    idx = np.arange(n)
    if inp["group"] is None:
        br = np.tile(inp["bracket"].astype(np.int64), (N, 1))
    else:
        group = inp["group"].astype(np.int64)
        table = inp["table"]
        pts = np.tile(table[:, 0], (N, 1))
        gf = np.tile(table[:, 1], (N, 1))
        ga = np.tile(table[:, 2], (N, 1))
        fp, fq = inp["fix_p"].astype(np.int64), inp["fix_q"].astype(np.int64)
        nf = fp.size
        if nf:
            J2, F2 = np.meshgrid(j, np.arange(nf), indexing="ij")
            hs, as_, x, y = _play(tables, inp, key, J2.ravel(), s[J2.ravel()], fp[F2.ravel()], fq[F2.ravel()],
                                  F2.ravel(), flagged)
            win, draw, loss = inp["points"]
            ph = np.where(x > y, win, np.where(x == y, draw, loss))
            pa = np.where(y > x, win, np.where(x == y, draw, loss))
            rows = J2.ravel()
            for acc, sl, v in ((pts, hs, ph), (pts, as_, pa), (gf, hs, x), (gf, as_, y), (ga, hs, y), (ga, as_, x)):
                np.add.at(acc, (rows, sl), v)
        gd = gf - ga
        r, _ = SR.threefry_block(key, j[:, None].astype(np.uint32),
                                 (SR.TIEBREAK_COUNTER | idx).astype(np.uint32)[None, :])
        r = r.astype(np.int64)
        # better[j, k, i]: slot k is ahead of slot i by the table keys
        P, G, F, RR = (v[:, :, None] for v in (pts, gd, gf, r))
        Pi, Gi, Fi, Ri = (v[:, None, :] for v in (pts, gd, gf, r))
        better = (P > Pi) | ((P == Pi) & ((G > Gi) | ((G == Gi) & ((F > Fi) | ((F == Fi) & (
            (RR > Ri) | ((RR == Ri) & (idx[:, None] < idx[None, :]))))))))
        same = group[:, None] == group[None, :]
        position = (better & same[None]).sum(axis=1)
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
        stage = (bpos >= 0).astype(np.int64)
        jj, ii = np.nonzero(bpos >= 0)
        br = np.full((N, nb), -1, dtype=np.int64)
        br[jj, bpos[jj, ii]] = ii
        assert (br >= 0).all()
    k0 = 0
    for rnd in range(R):
        M = nb >> (rnd + 1)
        p, q = br[:, 0::2], br[:, 1::2]
        win = p.copy()
        active = np.ones((N, M), dtype=bool)
        kk = k0 + np.arange(M)
        for t in range(ATTEMPTS):
            jj, mm = np.nonzero(active)
            if jj.size == 0:
                break
            ctr = KNOCKOUT_COUNTER | (kk[mm] << 5) | t
            hs, as_, x, y = _play(tables, inp, key, jj, s[jj], p[jj, mm], q[jj, mm], ctr, flagged)
            done = x != y
            win[jj[done], mm[done]] = np.where(x > y, hs, as_)[done]
            active[jj[done], mm[done]] = False
        rows = np.repeat(j, M).reshape(N, M)
        stage[rows, win] = rnd + 2
        br = win
        k0 += M
    stage_counts = np.zeros((n, R + 2), dtype=np.int64)
    np.add.at(stage_counts, (np.broadcast_to(idx, (N, n)), stage), 1)
    out = {"stage_counts": stage_counts, "stage": stage.astype(np.uint8), "position": position, "flagged": flagged}
    if inp["group"] is not None:
        pc = np.zeros((n, MAX_GROUP), dtype=np.int64)
        np.add.at(pc, (np.broadcast_to(idx, (N, n)), position), 1)
        out["position_counts"] = pc
    return out


# ---- tournament formats shared by the tests and tools/tournament_bench.py
def _letters(k):
    return [chr(ord("A") + i) for i in range(k)]


def group_format(teams, n_groups, size, best, seed=0, advance=2):
    """simulate_tournament kwargs: n_groups groups of `size` of `teams` (in order), the top `advance`
    (default two) and the `best` best of the rest qualify; the first knockout round in a seeded
    shuffled order."""
    names = _letters(n_groups)
    groups = {g: list(teams[i * size:(i + 1) * size]) for i, g in enumerate(names)}
    entries = [(g, p) for g in names for p in range(1, advance + 1)] + [("best", k) for k in range(1, best + 1)]
    order = np.random.RandomState(seed).permutation(len(entries))
    return {"groups": groups, "advance": advance, "best_of_rest": best, "knockout": [entries[i] for i in order]}


def world_cup_48(teams, seed=0):
    """48 teams: 12 groups of 4, top two + the 8 best thirds, a 32-team bracket."""
    return group_format(teams[:48], 12, 4, 8, seed)


def euro_24(teams, seed=0):
    """24 teams: 6 groups of 4, top two + the 4 best thirds, a 16-team bracket."""
    return group_format(teams[:24], 6, 4, 4, seed)


def knockout_64(teams):
    """A 64-team knockout only, in the given order."""
    return {"knockout": list(teams[:64])}
