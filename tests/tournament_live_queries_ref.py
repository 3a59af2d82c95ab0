"""numpy restatement of `tournament_paths`, `tournament_scenarios` and `tournament_points` with group matches in
progress and weighted draws (bpl/neutral_dixon_coles.py, csrc/dc_tournament_live_queries.hip.h),
as per-simulation records, for the tests.  It is composed from the restatements already here, none of which is changed:
the tournament is played by tournament_live_ref (the weights, the resampled draws, the conditional final scores, the
ranking, the allocation fill and the knockout under either rule), and the records it does not return are formed here
on ITS draws, from the posterior tables gathered by simulation as it gathers them:
  margin, group_outcome   on the CONCATENATED list, the F fixtures still to kick off and then the L matches in play: the
                          ordinary fixtures played again from knockout_ref.play's blocks (the same operations, so the same
                          scorelines) and turned to the listed order as paths_ref does, the matches in play from the
                          final scores tournament_live_ref returns in the listed order;
  pair, winner            its first round walked round by round, as paths_ref walks knockout_ref's;
  points, goal_difference every match of the concatenated list booked on the current table, as tournament_points_ref
                          books the ordinary ones; rest_rank as there.
The integer tables are then the pure cross-tabulations of paths_ref, tournament_scenarios_ref and tournament_points_ref
on these records, with the fixture list of the inputs concatenated (`shown`)."""
import numpy as np

import h2h_ref as H
import knockout_ref as K
import tournament_live_ref as TLR
import tournament_ref as TR
import tournament_scenarios_ref as TS


def shown(inp, in_play):
    """The checked inputs with the group-fixture list concatenated: what the cross-tabulations index."""
    in_play = TLR.NO_PLAY if in_play is None else in_play
    return dict(inp, fix_p=np.concatenate([inp["fix_p"], np.asarray(in_play[0], np.uint8)]),
                fix_q=np.concatenate([inp["fix_q"], np.asarray(in_play[1], np.uint8)]))


def simulate(tables, inp, key, in_play=None, reweight=True, log_weights=None, head_to_head=False, pair_init=None):
    """The per-simulation records of the three live queries for the checked inputs `inp`: tournament_live_ref's
    results ("stage", "draw", "in_play_home_goals", "in_play_away_goals", "flagged", "ess", "log_evidence",
    "stage_counts", with groups "position_counts", under "extra_time" "decided" and "decided_counts") and "position"
    u8 [N, n] (with groups), "margin" int64 and "group_outcome" u8 [N, F + L], "pair" u8 [N, 2^R - 1, 2], "winner" u8
    [N, 2^R - 1], and with groups int64 [N, n] "points", "goal_difference" and "rest_rank" (-1: not placed
    advance + 1)."""
    in_play = TLR.NO_PLAY if in_play is None else in_play
    ref = TLR.simulate_tournament_live(tables, inp, key, in_play, reweight, log_weights, head_to_head, pair_init)
    N, n, R = inp["num_simulations"], len(inp["team_idx"]), inp["rounds"]
    nb = 1 << R
    j = np.arange(N, dtype=np.int64)
    gt = TLR.gathered(tables, ref["draw"].astype(np.int64))
    scratch = np.zeros(N, dtype=bool)   # (the same walks as tournament_live_ref's: its flags already cover them)
    g = TLR.first_round(gt, inp, key, in_play, scratch, head_to_head, pair_init)
    np.testing.assert_array_equal(g["final_p"], ref["in_play_home_goals"])
    out = {k: ref[k] for k in ("stage", "draw", "in_play_home_goals", "in_play_away_goals", "flagged", "ess",
                               "log_evidence", "stage_counts", "position_counts", "decided", "decided_counts",
                               "slot_counts") if k in ref}
    # the listed sides' goals over the concatenated list
    fp, fq = inp["fix_p"].astype(np.int64), inp["fix_q"].astype(np.int64)
    F = fp.size
    first, second = np.zeros((N, F), dtype=np.int64), np.zeros((N, F), dtype=np.int64)
    if F:
        J2, F2 = np.meshgrid(j, np.arange(F), indexing="ij")
        rows, f = J2.ravel(), F2.ravel()
        hs, as_, on = TR.venue(fp[f], fq[f], inp["host"])
        x, y = K.play(gt, inp, key, rows, rows, hs, as_, on, f, 1.0, scratch)
        first = np.where(hs == fp[f], x, y).reshape(N, F).astype(np.int64)
        second = np.where(hs == fp[f], y, x).reshape(N, F).astype(np.int64)
    first = np.concatenate([first, ref["in_play_home_goals"].astype(np.int64)], axis=1)
    second = np.concatenate([second, ref["in_play_away_goals"].astype(np.int64)], axis=1)
    margin = first - second
    out["margin"] = margin
    out["group_outcome"] = np.where(margin > 0, 0, np.where(margin == 0, 1, 2)).astype(np.uint8)
    # the knockout matches, from the first round and the final stages
    stage = ref["stage"].astype(np.int64)
    br = g["bracket"]
    pair = np.zeros((N, nb - 1, 2), dtype=np.uint8)
    winner = np.zeros((N, nb - 1), dtype=np.uint8)
    k0 = 0
    for rnd in range(R):
        M = nb >> (rnd + 1)
        p, q = br[:, 0::2], br[:, 1::2]
        p_on = np.take_along_axis(stage, p, axis=1) >= rnd + 2
        q_on = np.take_along_axis(stage, q, axis=1) >= rnd + 2
        assert (p_on ^ q_on).all()
        win = np.where(p_on, p, q)
        pair[:, k0:k0 + M, 0], pair[:, k0:k0 + M, 1], winner[:, k0:k0 + M] = p, q, win
        br = win
        k0 += M
    out.update(pair=pair, winner=winner)
    if inp["group"] is None:
        return out
    position = g["position"].astype(np.int64)
    np.testing.assert_array_equal(position, ref["position"])
    # the final group tables: every match of the concatenated list booked for its listed sides
    sp = np.concatenate([fp, np.asarray(in_play[0], np.int64)])
    sq = np.concatenate([fq, np.asarray(in_play[1], np.int64)])
    table = np.asarray(inp["table"]).astype(np.int64)
    pts, gf, ga = (np.tile(table[:, c], (N, 1)) for c in range(3))
    win_, draw_, loss_ = inp["points"]
    rows = np.broadcast_to(j[:, None], first.shape)
    P1 = np.where(margin > 0, win_, np.where(margin == 0, draw_, loss_))
    P2 = np.where(margin < 0, win_, np.where(margin == 0, draw_, loss_))
    a, b = np.broadcast_to(sp, first.shape), np.broadcast_to(sq, first.shape)
    for acc, sl, v in ((pts, a, P1), (pts, b, P2), (gf, a, first), (gf, b, second), (ga, a, second), (ga, b, first)):
        np.add.at(acc, (rows, sl), v)
    better = H.overall_ahead(pts, gf, ga, H.words(key, N, n))
    rest = position == inp["advance"]
    out.update(position=position.astype(np.uint8), points=pts, goal_difference=gf - ga,
               rest_rank=np.where(rest, (better & rest[:, :, None]).sum(axis=1), -1))
    return out


def scenario(margin, keys, caps):
    """uint32 [N]: the row-major index of c - clip(margin, -c, c) over the key columns of `margin` [N, F + L]."""
    caps = np.asarray(caps, dtype=np.int64)
    stride, _ = TS.strides(caps)
    m = np.asarray(margin)[:, np.asarray(keys, dtype=np.int64)].astype(np.int64)
    cls = caps[None, :] - np.clip(m, -caps[None, :], caps[None, :])
    return (cls * stride[None, :]).sum(axis=1).astype(np.uint32)


def target_set(stage, position, rounds):
    """uint8 [N, n]: bit k <= R: stage >= k + 1; bit R + 1: first in its group."""
    stage = np.asarray(stage).astype(np.int64)
    return (((1 << stage) - 1) | ((np.asarray(position).astype(np.int64) == 0).astype(np.int64) << (rounds + 1))).astype(np.uint8)


def points_records(rec):
    """The records tournament_points_ref.counts reads, int64."""
    return {k: np.asarray(rec[k]).astype(np.int64) for k in ("points", "goal_difference", "position", "rest_rank", "stage")}
