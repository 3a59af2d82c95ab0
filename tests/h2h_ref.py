"""numpy restatement of the head-to-head tie-break (csrc/dc_h2h.hip.h, bpl/base.py `tiebreak="head_to_head"`)
for the tests: the ranking rule from (points, GF, GA, pair records, tie-break words), vectorised over the
simulations, the pair records of a set of scorelines, and the tournament with head-to-head groups, built on
tournament_ref's `_play` / `rates` / `venue` and season_ref's threefry blocks (neither is changed)."""
import numpy as np

import season_ref as SR
import tournament_ref as TR


def _ahead(keys, idx):
    """better[j, k, i]: slot k is ahead of slot i, lexicographically over `keys` ([N, n] each, descending),
    then slot ascending."""
    better = idx[:, None] < idx[None, :]
    better = np.broadcast_to(better, keys[0].shape[:1] + better.shape)
    for v in reversed(keys):
        K, Ki = v[:, :, None], v[:, None, :]
        better = (K > Ki) | ((K == Ki) & better)
    return better


def overall_ahead(pts, gf, ga, words):
    """better[j, k, i] under the overall order: points, GD, GF, word, slot."""
    pts, gf, ga, words = (np.asarray(v).astype(np.int64) for v in (pts, gf, ga, words))
    return _ahead([pts, gf - ga, gf, words], np.arange(pts.shape[1]))


def h2h_keys(pts, pair, group=None):
    """(head-to-head points, goal difference, goals) [N, n] of every slot against the slots level with it on
    points (of its group).  pair [N, n, n] or [n, n]: points << 16 | goals of row against column."""
    pts = np.asarray(pts).astype(np.int64)
    N, n = pts.shape
    pair = np.broadcast_to(np.asarray(pair).astype(np.int64), (N, n, n))
    pp, pg = pair >> 16, pair & 0xFFFF
    level = (pts[:, :, None] == pts[:, None, :]) & ~np.eye(n, dtype=bool)[None]
    if group is not None:
        group = np.asarray(group).astype(np.int64)
        level = level & (group[:, None] == group[None, :])[None]
    hp = (level * pp).sum(axis=2)
    hgf = (level * pg).sum(axis=2)
    hga = (level * pg.transpose(0, 2, 1)).sum(axis=2)
    return hp, hgf - hga, hgf


def rank(pts, gf, ga, pair, words, group=None):
    """position [N, n] of every slot (within its group) under the eight keys: points, head-to-head points,
    head-to-head GD, head-to-head goals, overall GD, overall GF, word (all descending), slot ascending."""
    pts, gf, ga, words = (np.asarray(v).astype(np.int64) for v in (pts, gf, ga, words))
    hp, hgd, hgf = h2h_keys(pts, pair, group)
    better = _ahead([pts, hp, hgd, hgf, gf - ga, gf, words], np.arange(pts.shape[1]))
    if group is not None:
        group = np.asarray(group).astype(np.int64)
        better = better & (group[:, None] == group[None, :])[None]
    return better.sum(axis=1)


def pair_from_scores(hs, as_, x, y, points, n, init=None):
    """[N, n, n] int64 pair records: `init` ([n, n] packed, or None) plus the matches hs v as_ ([F] slots) that
    ended x : y ([N, F])."""
    x, y = np.asarray(x).astype(np.int64), np.asarray(y).astype(np.int64)
    N, F = x.shape
    win, draw, loss = points
    init = np.zeros((n, n), dtype=np.int64) if init is None else np.asarray(init).astype(np.int64)
    pp = np.tile(init >> 16, (N, 1, 1))
    pg = np.tile(init & 0xFFFF, (N, 1, 1))
    if F:
        rows = np.broadcast_to(np.arange(N)[:, None], (N, F))
        H, A = np.broadcast_to(np.asarray(hs, np.int64), (N, F)), np.broadcast_to(np.asarray(as_, np.int64), (N, F))
        np.add.at(pp, (rows, H, A), np.where(x > y, win, np.where(x == y, draw, loss)))
        np.add.at(pp, (rows, A, H), np.where(y > x, win, np.where(x == y, draw, loss)))
        np.add.at(pg, (rows, H, A), x)
        np.add.at(pg, (rows, A, H), y)
    return (pp << 16) | pg


def words(key, N, n):
    """The tie-break words [N, n]: o0 of the threefry block (j, TIEBREAK_COUNTER | slot)."""
    r, _ = SR.threefry_block(key, np.arange(N, dtype=np.int64)[:, None].astype(np.uint32),
                             (SR.TIEBREAK_COUNTER | np.arange(n)).astype(np.uint32)[None, :])
    return r.astype(np.int64)


def season_positions(home_slot, away_slot, home_goals, away_goals, table, points, key, pair_init=None):
    """position [N, n] of a season whose remaining fixtures (slots) ended home_goals : away_goals [N, F], on top
    of `table` [n, 3] and `pair_init`; also returns the points [N, n]."""
    x, y = np.asarray(home_goals).astype(np.int64), np.asarray(away_goals).astype(np.int64)
    table = np.asarray(table).astype(np.int64)
    N, n = x.shape[0], table.shape[0]
    hs, as_ = np.asarray(home_slot, np.int64), np.asarray(away_slot, np.int64)
    win, draw, loss = points
    pts, gf, ga = (np.tile(table[:, c], (N, 1)) for c in range(3))
    if x.shape[1]:
        rows = np.broadcast_to(np.arange(N)[:, None], x.shape)
        H, A = np.broadcast_to(hs, x.shape), np.broadcast_to(as_, x.shape)
        ph = np.where(x > y, win, np.where(x == y, draw, loss))
        pa = np.where(y > x, win, np.where(x == y, draw, loss))
        for acc, sl, v in ((pts, H, ph), (pts, A, pa), (gf, H, x), (gf, A, y), (ga, H, y), (ga, A, x)):
            np.add.at(acc, (rows, sl), v)
    pair = pair_from_scores(hs, as_, x, y, points, n, pair_init)
    return rank(pts, gf, ga, pair, words(key, N, n)), pts


def simulate_tournament(tables, inp, key, pair_init=None):
    """tournament_ref.simulate_tournament with the groups ranked by the head-to-head order (the best of the rest
    keep the overall keys): the same dict, "flagged" included."""
    N, n, R = inp["num_simulations"], len(inp["team_idx"]), inp["rounds"]
    if inp["group"] is None:
        return TR.simulate_tournament(tables, inp, key)
    nb = 1 << R
    S = tables["attack"].shape[0]
    j = np.arange(N, dtype=np.int64)
    s = j % S
    flagged = np.zeros(N, dtype=bool)
    idx = np.arange(n)
    group = inp["group"].astype(np.int64)
    table = inp["table"]
    pts, gf, ga = (np.tile(table[:, c], (N, 1)) for c in range(3))
    init = np.zeros((n, n), dtype=np.int64) if pair_init is None else np.asarray(pair_init).astype(np.int64)
    pp, pg = np.tile(init >> 16, (N, 1, 1)), np.tile(init & 0xFFFF, (N, 1, 1))
    fp, fq = inp["fix_p"].astype(np.int64), inp["fix_q"].astype(np.int64)
    nf = fp.size
    if nf:
        J2, F2 = np.meshgrid(j, np.arange(nf), indexing="ij")
        hs, as_, x, y = TR._play(tables, inp, key, J2.ravel(), s[J2.ravel()], fp[F2.ravel()], fq[F2.ravel()],
                                 F2.ravel(), flagged)
        win, draw, loss = inp["points"]
        ph = np.where(x > y, win, np.where(x == y, draw, loss))
        pa = np.where(y > x, win, np.where(x == y, draw, loss))
        rows = J2.ravel()
        for acc, sl, v in ((pts, hs, ph), (pts, as_, pa), (gf, hs, x), (gf, as_, y), (ga, hs, y), (ga, as_, x)):
            np.add.at(acc, (rows, sl), v)
        np.add.at(pp, (rows, hs, as_), ph)
        np.add.at(pp, (rows, as_, hs), pa)
        np.add.at(pg, (rows, hs, as_), x)
        np.add.at(pg, (rows, as_, hs), y)
    r = words(key, N, n)
    position = rank(pts, gf, ga, (pp << 16) | pg, r, group)
    better = overall_ahead(pts, gf, ga, r)
    adv, bor = inp["advance"], inp["best_of_rest"]
    rest = position == adv
    rest_rank = (better & rest[:, :, None]).sum(axis=1)
    code = np.where(position < adv, TR.MAX_GROUP * group[None, :] + position,
                    np.where(rest & (rest_rank < bor), 128 + rest_rank, -1))
    code_pos = np.full(193, -1, dtype=np.int64)   # index 192: "no code"
    for b, c in enumerate(inp["bracket"].astype(np.int64)):
        hi, lo = c >> 8, c & 0xFF
        code_pos[128 + lo - 1 if hi == 0xFF else TR.MAX_GROUP * hi + lo - 1] = b
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
        win_ = p.copy()
        active = np.ones((N, M), dtype=bool)
        kk = k0 + np.arange(M)
        for t in range(TR.ATTEMPTS):
            jj, mm = np.nonzero(active)
            if jj.size == 0:
                break
            ctr = TR.KNOCKOUT_COUNTER | (kk[mm] << 5) | t
            hs, as_, x, y = TR._play(tables, inp, key, jj, s[jj], p[jj, mm], q[jj, mm], ctr, flagged)
            done = x != y
            win_[jj[done], mm[done]] = np.where(x > y, hs, as_)[done]
            active[jj[done], mm[done]] = False
        rows = np.repeat(j, M).reshape(N, M)
        stage[rows, win_] = rnd + 2
        br = win_
        k0 += M
    stage_counts = np.zeros((n, R + 2), dtype=np.int64)
    np.add.at(stage_counts, (np.broadcast_to(idx, (N, n)), stage), 1)
    pc = np.zeros((n, TR.MAX_GROUP), dtype=np.int64)
    np.add.at(pc, (np.broadcast_to(idx, (N, n)), position), 1)
    return {"stage_counts": stage_counts, "stage": stage.astype(np.uint8), "position": position, "flagged": flagged,
            "position_counts": pc}
