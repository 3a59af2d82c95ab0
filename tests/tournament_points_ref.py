"""numpy restatement of `tournament_points` (bpl/neutral_dixon_coles.py, csrc/dc_group_points.hip.h) for the tests:
the tournament is played by tests/paths_ref.py (which plays it through tournament_ref, h2h_ref and knockout_ref), and
the per-simulation records it does not return are formed here:
  points, goal_difference  the group fixtures played again from knockout_ref.play's blocks (the same operations, so the
                           same scorelines) and booked on top of the current table;
  rest_rank                h2h_ref.overall_ahead over the slots placed advance + 1 (the best of the rest keep the
                           overall keys in both tie-break modes), -1 for every other slot.
`counts` is the pure cross-tabulation of such records into the integer tables of the result; `records_from_paths` forms
the records `tournament_paths(return_records=True)` can give (everything but the goal difference and the rest ranks)."""
import numpy as np

import h2h_ref as H
import knockout_ref as K
import paths_ref as P
import tournament_ref as TR


def group_tables(tables, inp, key):
    """(points, goals for, goals against) int64 [N, n] each: the current table plus every simulated group fixture."""
    N = inp["num_simulations"]
    j = np.arange(N, dtype=np.int64)
    s = j % tables["attack"].shape[0]
    table = np.asarray(inp["table"]).astype(np.int64)
    pts, gf, ga = (np.tile(table[:, c], (N, 1)) for c in range(3))
    fp, fq = inp["fix_p"].astype(np.int64), inp["fix_q"].astype(np.int64)
    if fp.size:
        J2, F2 = np.meshgrid(j, np.arange(fp.size), indexing="ij")
        rows, f = J2.ravel(), F2.ravel()
        hs, as_, on = TR.venue(fp[f], fq[f], inp["host"])
        scratch = np.zeros(N, dtype=bool)   # (the same walks as paths_ref.simulate's: its flags already cover them)
        x, y = K.play(tables, inp, key, rows, s[rows], hs, as_, on, f, 1.0, scratch)
        win, draw, loss = inp["points"]
        ph = np.where(x > y, win, np.where(x == y, draw, loss))
        pa = np.where(y > x, win, np.where(x == y, draw, loss))
        for acc, sl, v in ((pts, hs, ph), (pts, as_, pa), (gf, hs, x), (gf, as_, y), (ga, hs, y), (ga, as_, x)):
            np.add.at(acc, (rows, sl), v)
    return pts, gf, ga


def simulate(tables, inp, key, head_to_head=False, pair_init=None):
    """The per-simulation records of `tournament_points` for the checked inputs `inp` (the dict of _tournament_inputs,
    with groups): int64 [N, n] "points", "goal_difference", "position", "rest_rank" (-1: not placed advance + 1) and
    "stage"; under "extra_time" "decided"; and "flagged" [N], the restatement's own vector."""
    rec = P.simulate(tables, inp, key, head_to_head=head_to_head, pair_init=pair_init)
    N, n = inp["num_simulations"], len(inp["team_idx"])
    pts, gf, ga = group_tables(tables, inp, key)
    position = rec["position"].astype(np.int64)
    better = H.overall_ahead(pts, gf, ga, H.words(key, N, n))
    rest = position == inp["advance"]
    rest_rank = np.where(rest, (better & rest[:, :, None]).sum(axis=1), -1)
    out = {"points": pts, "goal_difference": gf - ga, "position": position, "rest_rank": rest_rank,
           "stage": rec["stage"].astype(np.int64), "flagged": rec["flagged"]}
    if "decided" in rec:
        out["decided"] = rec["decided"]
    return out


def records_from_paths(res, inp):
    """The records a `tournament_paths(return_records=True)` result holds: "points" from its group outcomes (listed
    order) on top of the current table, "position" and "stage"."""
    o = np.asarray(res["group_outcome"]).astype(np.int64)
    fx = np.asarray(res["fixtures"]).astype(np.int64)
    N, n = o.shape[0], len(inp["team_idx"])
    win, draw, loss = inp["points"]
    first = np.array([win, draw, loss], dtype=np.int64)[o]
    second = np.array([loss, draw, win], dtype=np.int64)[o]
    pts = np.tile(np.asarray(inp["table"]).astype(np.int64)[:, 0], (N, 1))
    rows = np.broadcast_to(np.arange(N)[:, None], o.shape)
    np.add.at(pts, (rows, np.broadcast_to(fx[:, 0], o.shape)), first)
    np.add.at(pts, (rows, np.broadcast_to(fx[:, 1], o.shape)), second)
    return {"points": pts, "position": np.asarray(res["position"]).astype(np.int64),
            "stage": np.asarray(res["stage"]).astype(np.int64)}


def counts(rec, inp, points_min, n_bins, gd_cap=None):
    """The integer tables of `tournament_points` from per-simulation records, int64: "team_points_count" [n, P],
    "team_target_count" [n, P, K], "team_place_count" [n, P, Z], "place_points_count" [Gn, Z, P], "place_gap_count"
    [Gn, Z - 1, P]; and, with `gd_cap` and a best of the rest, "rest_count" and "rest_through_count" [P, D] and
    "rest_rank_count" [B, P, D]."""
    pts, pos, stage = rec["points"], rec["position"], rec["stage"]
    N, n = pts.shape
    Rr, Z, Pn = inp["rounds"], inp["group_size"], int(n_bins)
    Kt = Rr + 2
    group = inp["group"].astype(np.int64)
    Gn = len(inp["group_names"])
    v = pts - int(points_min)
    assert (v >= 0).all() and (v < Pn).all() and (pos >= 0).all() and (pos < Z).all()
    slot = np.broadcast_to(np.arange(n), (N, n))
    inside = np.concatenate([stage[:, :, None] >= np.arange(1, Rr + 2)[None, None, :], (pos == 0)[:, :, None]], axis=2)
    out = {"team_points_count": np.zeros((n, Pn), dtype=np.int64), "team_target_count": np.zeros((n, Pn, Kt), dtype=np.int64),
           "team_place_count": np.zeros((n, Pn, Z), dtype=np.int64), "place_points_count": np.zeros((Gn, Z, Pn), dtype=np.int64),
           "place_gap_count": np.zeros((Gn, Z - 1, Pn), dtype=np.int64)}
    np.add.at(out["team_points_count"], (slot, v), 1)
    for k in range(Kt):
        np.add.at(out["team_target_count"][:, :, k], (slot, v), inside[:, :, k].astype(np.int64))
    np.add.at(out["team_place_count"], (slot, v, pos), 1)
    np.add.at(out["place_points_count"], (np.broadcast_to(group, (N, n)), pos, v), 1)
    # the points by (group, place), -1 where the group lacks the place
    by_place = np.full((N, Gn, Z), -1, dtype=np.int64)
    by_place[np.broadcast_to(np.arange(N)[:, None], (N, n)), np.broadcast_to(group, (N, n)), pos] = v
    for g in range(Gn):
        for z in range(Z - 1):
            if (by_place[:, g, z + 1] >= 0).all():
                gap = by_place[:, g, z] - by_place[:, g, z + 1]
                assert (gap >= 0).all()
                out["place_gap_count"][g, z] = np.bincount(gap, minlength=Pn)
    best = inp["best_of_rest"]
    if gd_cap is not None and best > 0:
        c = int(gd_cap)
        D = 2 * c + 1
        d = np.clip(rec["goal_difference"], -c, c) + c
        rank = rec["rest_rank"]
        B = int((np.bincount(group, minlength=Gn) > inp["advance"]).sum())
        on = rank >= 0
        assert (on.sum(axis=1) == B).all() and (rank < B).all()
        out["rest_count"] = np.zeros((Pn, D), dtype=np.int64)
        out["rest_through_count"] = np.zeros((Pn, D), dtype=np.int64)
        out["rest_rank_count"] = np.zeros((B, Pn, D), dtype=np.int64)
        np.add.at(out["rest_count"], (v[on], d[on]), 1)
        through = on & (rank < best)
        np.add.at(out["rest_through_count"], (v[through], d[through]), 1)
        np.add.at(out["rest_rank_count"], (rank[on], v[on], d[on]), 1)
    return out
