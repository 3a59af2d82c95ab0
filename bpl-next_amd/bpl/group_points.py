"""How many group points it takes in a tournament (no reference counterpart): the floats and the reading helpers of
`tournament_points` (bpl/neutral_dixon_coles.py), the tournament counterpart of `points_needed`.

The device (csrc/dc_group_points.hip.h) returns integer tables over `simulate_tournament`'s simulations.  With n slots,
P points bins, K = R + 2 targets, Gn groups of at most Z teams, B groups with a place advance + 1 and D = 2 gd_cap + 1
goal-difference bins: `team_points_count` [n, P], `team_target_count` [n, P, K], `team_place_count` [n, P, Z],
`place_points_count` [Gn, Z, P], `place_gap_count` [Gn, Z - 1, P] and, with a best of the rest, `rest_count` and
`rest_through_count` [P, D] and `rest_rank_count` [B, P, D].  Everything else is formed here, one float64 operation per
cell on integer sums, by the formulas of `bpl.base.points_from_counts` (definition: DESIGN.md section 37).

The helpers below are pure host functions on a result dict."""

from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

from bpl.base import _first_bin, check_levels, points_from_counts
from bpl.paths import _ratio, _slot

GD_CAP_MAX = 8   # include/bplhip.h BPLHIP_GROUP_POINTS_MAX_GD_CAP
MAX_BINS = 256   # include/bplhip.h BPLHIP_GROUP_POINTS_MAX_BINS


def check_gd_cap(gd_cap) -> int:
    """tournament_points' `gd_cap`: a non-bool integer in 0..8."""
    if isinstance(gd_cap, (bool, np.bool_)) or not isinstance(gd_cap, (int, np.integer)) or not 0 <= gd_cap <= GD_CAP_MAX:
        raise ValueError(f"gd_cap must be an integer in [0, {GD_CAP_MAX}], not {gd_cap!r}")
    return int(gd_cap)


# pylint: disable=too-many-arguments,too-many-locals
def from_counts(team_points_count, team_target_count, team_place_count, place_points_count, place_gap_count,
                points_min: int, n_sims: int, levels, rest_count=None, rest_through_count=None, rest_rank_count=None,
                best_of_rest: int = 0) -> Dict[str, np.ndarray]:
    """tournament_points' tables and floats from the device's integer tables and `levels` [L] (`check_levels`).  The
    team tables go through `points_from_counts` unchanged, the (group, place) rows standing for its positions and the
    (group, gap) rows for its gaps; a place that never occurred (a place the group lacks) has mean NaN and quantile
    -1.  The rest tables are taken when `best_of_rest` > 0."""
    levels = check_levels(levels)
    tz = np.asarray(team_place_count).astype(np.int64)
    pp = np.asarray(place_points_count).astype(np.int64)
    gap = np.asarray(place_gap_count).astype(np.int64)
    groups, size, bins = pp.shape
    base = points_from_counts(team_points_count, team_target_count, pp.reshape(groups * size, bins),
                              gap.reshape(groups * (size - 1), bins), points_min, n_sims, levels)
    tp, points = base["team_points_count"], base["points"]
    rounds = base["team_target_count"].shape[2] - 2
    missing = pp.sum(axis=2) == 0                                                       # [Gn, Z]
    out = {k: base[k] for k in ("points", "levels", "team_points_count", "team_points_proba", "team_target_count",
                                "target_count", "target_proba", "proba_given_points", "se_given_points",
                                "proba_given_at_least", "points_needed")}
    out.update({
        "round_proba": base["target_count"][:, :rounds + 1] / n_sims,
        "team_place_count": tz, "group_position_proba": tz.sum(axis=1) / n_sims,
        "place_given_points": _ratio(tz, tp[:, :, None]),
        "place_points_count": pp,
        "place_points_mean": np.where(missing, np.nan, base["position_points_mean"].reshape(groups, size)),
        "place_points_quantile": np.where(missing[None], -1, base["position_points_quantile"].reshape(-1, groups, size)),
        "place_gap_count": gap, "level_proba": base["level_proba"].reshape(groups, size - 1),
    })
    if best_of_rest > 0:
        rc = np.asarray(rest_count).astype(np.int64)
        rt = np.asarray(rest_through_count).astype(np.int64)
        rr = np.asarray(rest_rank_count).astype(np.int64)
        cap = (rc.shape[1] - 1) // 2
        # "at least p": the integer reverse cumulative sums over the bins, pooled over the goal difference
        had = rc.sum(axis=1)[::-1].cumsum()[::-1]
        through = rt.sum(axis=1)[::-1].cumsum()[::-1]
        at_least = _ratio(through, had)
        with np.errstate(invalid="ignore"):
            reached = at_least[None, :] >= levels[:, None]                              # [L, P] (NaN compares False)
        cut = rr[best_of_rest - 1]
        out.update({
            "goal_difference": np.arange(-cap, cap + 1, dtype=np.int64),
            "rest_count": rc, "rest_through_count": rt, "rest_rank_count": rr,
            "rest_proba": _ratio(rt, rc), "rest_proba_given_at_least": at_least,
            "rest_points_needed": _first_bin(reached, points),
            "cut_points_proba": cut.sum(axis=1) / n_sims, "cut_proba": cut / n_sims,
        })
    return out


def cut_line(result) -> Optional[Tuple[int, int, float]]:
    """(points, goal difference, probability) of the most likely last qualifier among the best of the rest (the first
    such cell in points, then goal-difference order on a tie); the goal difference is the clipped one, an end bin
    reading "that or beyond".  None without a best of the rest."""
    if "cut_proba" not in result:
        return None
    proba = np.asarray(result["cut_proba"])
    p, d = np.unravel_index(int(proba.argmax()), proba.shape)
    return int(result["points"][p]), int(result["goal_difference"][d]), float(proba[p, d])


def format_table(result, team) -> str:
    """A plain-text summary for one team: per points total it ended the groups on, P(points), P(each target | those
    points), P(each target | at least those points); then the points its targets need at each level, and with a best
    of the rest the cut line."""
    t = _slot(result, team)
    targets = [str(k) for k in result["targets"]]
    lines = [f"{result['teams'][t]}", "  points  P(points)  " + "  ".join(f"{k:>12}" for k in targets)]
    for b, p in enumerate(result["points"]):
        if result["team_points_count"][t, b] > 0:
            lines.append(f"  {int(p):>6}  {result['team_points_proba'][t, b]:9.1%}  "
                         + "  ".join(f"{v:12.1%}" for v in result["proba_given_points"][t, b]))
    lines.append("  points needed (at least)  " + "  ".join(f"{lv:>6.0%}" for lv in result["levels"]))
    for k, name in enumerate(targets):
        lines.append(f"  {name:<24}  " + "  ".join(f"{v:>6.0f}" for v in result["points_needed"][t, k]))
    cut = cut_line(result)
    if cut is not None:
        lines.append(f"  most likely last qualifier of the rest: {cut[0]} points, goal difference {cut[1]:+d} ({cut[2]:.1%})")
    return "\n".join(lines)
