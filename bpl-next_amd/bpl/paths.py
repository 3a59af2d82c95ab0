"""Who meets whom in a tournament (no reference counterpart): the floats and the reading helpers of
`tournament_paths` (bpl/neutral_dixon_coles.py).

The device (csrc/dc_paths.hip.h) returns integer tables over `simulate_tournament`'s simulations: `stage_count`
[n, R + 2] (each slot's furthest stage), `advance_count` [R, n, n] (t went through against u in knockout round r),
with groups `position_stage_count` [n, P, R + 2] (group position x furthest stage), and for the group fixtures
`match_leverage`'s three tables.  Everything else is formed here, one float64 operation per cell on integer sums
(definition: DESIGN.md section 35).  R knockout rounds give K = R + 1 targets, named `round_0` .. `round_{R-1}`
("plays knockout round r") and `winner`.

The helpers below are pure host functions on a result dict."""

from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np


def target_names(rounds: int) -> np.ndarray:
    """The K = R + 1 targets of a tournament with R knockout rounds."""
    return np.array([f"round_{r}" for r in range(rounds)] + ["winner"])


def _ratio(num, den) -> np.ndarray:
    """num / den in float64, NaN where den is 0."""
    num, den = np.broadcast_arrays(np.asarray(num, dtype=np.int64), np.asarray(den, dtype=np.int64))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / den, np.nan)


def from_counts(stage_count, advance_count, n_sims: int, position_stage_count=None) -> Dict[str, np.ndarray]:
    """tournament_paths' knockout and group-place tables and floats from the device's integer tables: "stage_count",
    "advance_count", "meet_count" = advance + its transpose, "meet_proba" = meet / n_sims, "opponent_proba" = meet /
    (the simulations in which t plays round r; NaN where there are none), "advance_given_meet" = advance / meet (NaN
    where the two never met); with `position_stage_count` [n, P, R + 2] also that table and
    "round_proba_given_position" [n, P, R + 1] (NaN where the position never occurred)."""
    stage = np.asarray(stage_count).astype(np.int64)
    adv = np.asarray(advance_count).astype(np.int64)
    rounds = adv.shape[0]
    meet = adv + adv.transpose(0, 2, 1)
    reached = np.cumsum(stage[:, ::-1], axis=1)[:, ::-1]   # [n, R + 2]: stage >= k
    plays = reached[:, 1:rounds + 1].T                      # [R, n]: t plays knockout round r
    out = {"stage_count": stage, "advance_count": adv, "meet_count": meet, "meet_proba": meet / n_sims,
           "opponent_proba": _ratio(meet, plays[:, :, None]), "advance_given_meet": _ratio(adv, meet)}
    if position_stage_count is not None:
        ps = np.asarray(position_stage_count).astype(np.int64)
        tail = np.cumsum(ps[:, :, ::-1], axis=2)[:, :, ::-1]   # [n, P, R + 2]: position p and stage >= k
        out["position_stage_count"] = ps
        out["round_proba_given_position"] = _ratio(tail[:, :, 1:], tail[:, :, :1])
    return out


def _slot(result, team) -> int:
    teams = [str(t) for t in result["teams"]]
    if not isinstance(team, (str, np.str_)) or str(team) not in teams:
        raise ValueError(f"{team!r} does not play in the tournament")
    return teams.index(str(team))


def opponents(result, team, top: int = 3) -> List[List[Tuple[str, float]]]:
    """Per knockout round, the `top` most likely opponents of `team` as (name, P(that opponent | the team plays the
    round)), most likely first (ties in slot order); a round the team never plays has an empty list."""
    if isinstance(top, (bool, np.bool_)) or not isinstance(top, (int, np.integer)) or top < 1:
        raise ValueError("top must be a positive integer")
    t = _slot(result, team)
    out = []
    for r in range(result["meet_count"].shape[0]):
        count, proba = result["meet_count"][r, t], result["opponent_proba"][r, t]
        order = [u for u in np.argsort(-count, kind="stable") if count[u] > 0][:top]
        out.append([(str(result["teams"][u]), float(proba[u])) for u in order])
    return out


def most_likely_final(result) -> Optional[Tuple[str, str, float]]:
    """(team, team, probability) of the most likely pairing of the last knockout round."""
    final = np.triu(result["meet_count"][-1])
    if not final.any():
        return None
    t, u = np.unravel_index(int(final.argmax()), final.shape)
    return str(result["teams"][t]), str(result["teams"][u]), float(result["meet_proba"][-1, t, u])


def format_table(result, team, top: int = 3) -> str:
    """A plain-text summary for one team: per knockout round P(plays it), the most likely opponents with
    P(opponent | plays) and P(goes through | meets); with groups, what each group place is worth, P(reaches each
    round | place)."""
    t = _slot(result, team)
    targets = [str(k) for k in result["targets"]]
    lines = [f"{result['teams'][t]}"]
    best = opponents(result, team, top)
    for r, rivals in enumerate(best):
        lines.append(f"  {targets[r]:<8} plays {result['round_proba'][t, r]:6.1%}")
        for name, p in rivals:
            u = _slot(result, name)
            lines.append(f"      v {name:<12} {p:6.1%}   goes through {result['advance_given_meet'][r, t, u]:6.1%}")
    lines.append(f"  {targets[-1]:<8}       {result['round_proba'][t, -1]:6.1%}")
    if "round_proba_given_position" in result:
        lines.append("  group place  P(place)  " + "  ".join(f"{k:>8}" for k in targets))
        given = result["round_proba_given_position"][t]
        for p in range(given.shape[0]):
            share = result["group_position_proba"][t, p]
            if share > 0:
                lines.append(f"  {p + 1:>11}  {share:8.1%}  " + "  ".join(f"{v:8.1%}" for v in given[p]))
    return "\n".join(lines)
