"""numpy restatement of `tournament_paths` (bpl/neutral_dixon_coles.py, csrc/dc_paths.hip.h) for the tests: the
tournament is played by the existing restatements -- tournament_ref (redraw, overall order), h2h_ref (redraw,
head-to-head order) and knockout_ref (extra time, either order) -- and the per-simulation records they do not return
are formed here from what they do:
  group_outcome  the group fixtures played again from knockout_ref.play's blocks (the same operations, so the same
                 scorelines) and read in the LISTED order of the fixture;
  pair, winner   knockout_ref.first_round's bracket walked round by round: of the two slots of a match the one whose
                 final stage is at least r + 2 went through (exactly one is).
`counts` is the pure cross-tabulation of such records -- the device's own or the restatement's -- into the integer
tables of the result."""
import numpy as np

import h2h_ref as H
import knockout_ref as K
import tournament_ref as TR


def simulate(tables, inp, key, head_to_head=False, pair_init=None):
    """The per-simulation records of `tournament_paths` for the checked inputs `inp` (the dict of _tournament_inputs):
    "stage" u8 [N, n], "position" u8 [N, n] (with groups), "group_outcome" u8 [N, nf], "pair" u8 [N, 2^R - 1, 2],
    "winner" u8 [N, 2^R - 1], under "extra_time" "decided" u8 [N, 2^R - 1], and "flagged" [N], the restatement's own
    vector."""
    N, n, R = inp["num_simulations"], len(inp["team_idx"]), inp["rounds"]
    nb = 1 << R
    if inp["knockout_rule"] == "extra_time":
        ref = K.simulate_tournament(tables, inp, key, head_to_head=head_to_head, pair_init=pair_init)
    elif head_to_head:
        ref = H.simulate_tournament(tables, inp, key, pair_init=pair_init)
    else:
        ref = TR.simulate_tournament(tables, inp, key)
    stage = ref["stage"].astype(np.int64)
    scratch = np.zeros(N, dtype=bool)   # (the same walks as the restatement's: its flags already cover them)
    br, _, position = K.first_round(tables, inp, key, scratch, head_to_head, pair_init)
    if inp["group"] is not None:
        np.testing.assert_array_equal(position, ref["position"])
    j = np.arange(N, dtype=np.int64)
    s = j % tables["attack"].shape[0]
    fp, fq = inp["fix_p"].astype(np.int64), inp["fix_q"].astype(np.int64)
    outcome = np.zeros((N, fp.size), dtype=np.uint8)
    if fp.size:
        J2, F2 = np.meshgrid(j, np.arange(fp.size), indexing="ij")
        rows, f = J2.ravel(), F2.ravel()
        hs, as_, on = TR.venue(fp[f], fq[f], inp["host"])
        x, y = K.play(tables, inp, key, rows, s[rows], hs, as_, on, f, 1.0, scratch)
        first, second = np.where(hs == fp[f], x, y), np.where(hs == fp[f], y, x)
        outcome = np.where(first > second, 0, np.where(first == second, 1, 2)).reshape(N, fp.size).astype(np.uint8)
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
    out = {"stage": ref["stage"], "group_outcome": outcome, "pair": pair, "winner": winner, "flagged": ref["flagged"]}
    if inp["group"] is not None:
        out["position"] = position.astype(np.uint8)
    if "decided" in ref:
        out["decided"] = ref["decided"]
    return out


def counts(records, inp):
    """The integer tables of `tournament_paths` from per-simulation records: "stage_count" [n, R + 2], "advance_count"
    and "meet_count" [R, n, n], with groups "position_stage_count" [n, P, R + 2], with group fixtures "outcome_count"
    [nf, 3], "target_count" [n, R + 1] and "joint_count" [nf, 3, n, R + 1]."""
    stage = np.asarray(records["stage"]).astype(np.int64)
    N, n = stage.shape
    R = inp["rounds"]
    nb = 1 << R
    idx = np.broadcast_to(np.arange(n), (N, n))
    stage_count = np.zeros((n, R + 2), dtype=np.int64)
    np.add.at(stage_count, (idx, stage), 1)
    pair, winner = np.asarray(records["pair"]).astype(np.int64), np.asarray(records["winner"]).astype(np.int64)
    advance = np.zeros((R, n, n), dtype=np.int64)
    k0 = 0
    for r in range(R):
        M = nb >> (r + 1)
        p, q, w = pair[:, k0:k0 + M, 0], pair[:, k0:k0 + M, 1], winner[:, k0:k0 + M]
        assert ((w == p) | (w == q)).all()
        np.add.at(advance[r], (w.ravel(), np.where(w == p, q, p).ravel()), 1)
        k0 += M
    out = {"stage_count": stage_count, "advance_count": advance, "meet_count": advance + advance.transpose(0, 2, 1)}
    if inp["group"] is not None:
        ps = np.zeros((n, inp["group_size"], R + 2), dtype=np.int64)
        np.add.at(ps, (idx, np.asarray(records["position"]).astype(np.int64), stage), 1)
        out["position_stage_count"] = ps
    nf = len(inp["fix_p"])
    if nf:
        o = np.asarray(records["group_outcome"]).astype(np.int64)
        reach = stage[:, :, None] >= np.arange(1, R + 2)[None, None, :]                 # [N, n, K]
        onehot = (o[:, :, None] == np.arange(3)[None, None, :]).astype(np.int64)         # [N, nf, 3]
        out["outcome_count"] = onehot.sum(axis=0)
        out["target_count"] = reach.sum(axis=0)
        # (a float64 product of 0 / 1 matrices: exact, the sums are far below 2^53)
        joint = onehot.reshape(N, nf * 3).astype(np.float64).T @ reach.reshape(N, n * (R + 1)).astype(np.float64)
        out["joint_count"] = joint.astype(np.int64).reshape(nf, 3, n, R + 1)
    return out
