"""numpy restatement of the group stage under a `best_allocation` (bpl/allocation.py, bpl/neutral_dixon_coles.py,
csrc/dc_tournament.hip.h), for the tests: the group matches, the group and best-of-rest ranking exactly as
knockout_ref.first_round has them -- through h2h_ref.words / overall_ahead / rank, knockout_ref.play and
tournament_ref.venue -- and then the ALLOCATED bracket fill: the groups of the qualifiers placed advance + 1 select a
row of the table, and the qualifier from group g goes to the bracket position of ("best", k) where g is the row's
element k - 1.  The table is read from inp["best_allocation"] (the mapping in bpl.allocation.check's form, keyed by
group names), row by row in plain Python -- not from the arrays the device reads.

`first_round` has knockout_ref.first_round's signature and returns, so pytest's monkeypatch of that name turns
knockout_ref.simulate_tournament, paths_ref, tournament_scenarios_ref and tournament_points_ref into allocation
restatements under knockout_rule="extra_time".  `simulate_redraw` is tournament_ref.simulate_tournament's knockout
loop on the same first round, for the redraw rule in either tie-break order."""
import numpy as np

import h2h_ref as H
import knockout_ref as K
import tournament_ref as TR


def group_stage(tables, inp, key, flagged, head_to_head=False, pair_init=None):
    """The group stage under inp["best_allocation"]: "bracket" [N, 2^R] slots, "stage" [N, n] 0 / 1, "position"
    [N, n], "through" bool [N, n] (a qualifier placed advance + 1), "rest_rank" [N, n] (its rank among the teams so
    placed), "slot" [N, n] (its 0-based allocation slot, -1 for every other team), "row" [N] (the index of the
    simulation's combination in the table's order) and "slot_counts" [groups, B]."""
    N, n = inp["num_simulations"], len(inp["team_idx"])
    nb = 1 << inp["rounds"]
    j = np.arange(N, dtype=np.int64)
    s = j % tables["attack"].shape[0]
    group = inp["group"].astype(np.int64)
    table = inp["table"]
    pts, gf, ga = (np.tile(table[:, c], (N, 1)) for c in range(3))
    init = np.zeros((n, n), dtype=np.int64) if pair_init is None else np.asarray(pair_init).astype(np.int64)
    pp, pg = np.tile(init >> 16, (N, 1, 1)), np.tile(init & 0xFFFF, (N, 1, 1))
    fp, fq = inp["fix_p"].astype(np.int64), inp["fix_q"].astype(np.int64)
    if fp.size:
        J2, F2 = np.meshgrid(j, np.arange(fp.size), indexing="ij")
        rows, f = J2.ravel(), F2.ravel()
        hs, as_, on = TR.venue(fp[f], fq[f], inp["host"])
        x, y = K.play(tables, inp, key, rows, s[rows], hs, as_, on, f, 1.0, flagged)
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
    through = rest & (rest_rank < bor)
    # ---- the allocated fill: the row of the qualifying groups, read from the mapping itself
    names = list(inp["group_names"])
    alloc = inp["best_allocation"]
    row_index = {k: i for i, k in enumerate(alloc)}
    slot = np.full((N, n), -1, dtype=np.int64)
    row = np.zeros(N, dtype=np.int64)
    for sim in range(N):
        lanes = np.nonzero(through[sim])[0]
        combo = tuple(names[g] for g in sorted(group[lanes]))
        assert len(combo) == bor and len(set(combo)) == bor
        order = alloc[combo]
        row[sim] = row_index[combo]
        for t in lanes:
            slot[sim, t] = order.index(names[group[t]])
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
    slot_counts = np.zeros((len(names), bor), dtype=np.int64)
    tj, tt = np.nonzero(through)
    np.add.at(slot_counts, (group[tt], slot[tj, tt]), 1)
    return {"bracket": br, "stage": (bpos >= 0).astype(np.int64), "position": position, "through": through,
            "rest_rank": rest_rank, "slot": slot, "row": row, "slot_counts": slot_counts}


def first_round(tables, inp, key, flagged, head_to_head=False, pair_init=None):
    """knockout_ref.first_round under inp["best_allocation"]: (bracket [N, 2^R] slots, stage [N, n] 0 / 1, position
    [N, n]).  Without a table (or without groups) it is knockout_ref.first_round itself."""
    if inp.get("best_allocation") is None:
        return _RANKED_FIRST_ROUND(tables, inp, key, flagged, head_to_head, pair_init)
    g = group_stage(tables, inp, key, flagged, head_to_head, pair_init)
    return g["bracket"], g["stage"], g["position"]


_RANKED_FIRST_ROUND = K.first_round   # (bound at import: a test may replace knockout_ref's name with `first_round`)


def simulate_redraw(tables, inp, key, head_to_head=False, pair_init=None):
    """The raw results of `simulate_tournament` under the redraw rule and inp["best_allocation"]: the knockout-round
    loop of tournament_ref.simulate_tournament on the allocated first round.  "stage_counts" [n, R + 2],
    "position_counts" [n, 8], "slot_counts" [groups, B], "stage" and "position" [N, n], "bracket" [N, 2^R], "row" [N]
    and "flagged" [N]."""
    N, n, R = inp["num_simulations"], len(inp["team_idx"]), inp["rounds"]
    nb = 1 << R
    j = np.arange(N, dtype=np.int64)
    s = j % tables["attack"].shape[0]
    flagged = np.zeros(N, dtype=bool)
    g = group_stage(tables, inp, key, flagged, head_to_head, pair_init)
    br, stage, position = g["bracket"], g["stage"].copy(), g["position"]
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
            hs, as_, x, y = TR._play(tables, inp, key, jj, s[jj], p[jj, mm], q[jj, mm], ctr, flagged)
            done = x != y
            win[jj[done], mm[done]] = np.where(x > y, hs, as_)[done]
            active[jj[done], mm[done]] = False
        stage[np.repeat(j, M).reshape(N, M), win] = rnd + 2
        br = win
        k0 += M
    idx = np.broadcast_to(np.arange(n), (N, n))
    stage_counts = np.zeros((n, R + 2), dtype=np.int64)
    np.add.at(stage_counts, (idx, stage), 1)
    pc = np.zeros((n, TR.MAX_GROUP), dtype=np.int64)
    np.add.at(pc, (idx, position), 1)
    return {"stage_counts": stage_counts, "position_counts": pc, "slot_counts": g["slot_counts"],
            "stage": stage.astype(np.uint8), "position": position, "bracket": g["bracket"], "row": g["row"],
            "flagged": flagged}
