"""The joint result of a few chosen fixtures against finishing targets (no reference counterpart): "we stay up if
we win, or if we draw and they lose by two".

`match_scenarios` (bpl/base.py) names 1..8 key fixtures of the fixture list.  Key fixture q with margin cap c_q has
C_q = 2 c_q + 1 classes: class j holds the simulations whose clipped margin clip(home goals - away goals, -c_q, c_q)
equals c_q - j, so class 0 reads "home by c_q or more", class 2 c_q "away by c_q or more", and with c_q = 1 the
classes are `match_leverage`'s outcomes 0 home win, 1 draw, 2 away win.  A scenario is one class per key fixture; its
index is row-major in the order given, m = sum_q class_q prod_{r > q} C_r, so every array with a leading M reshapes
to (*shape, ...).  The device (csrc/dc_scenario.hip.h) returns two integer tables over `simulate_season`'s
simulations, `scenario_count` [M] and `joint_count` [M, n, K]; everything else is formed here, one float64 operation
per cell on integer sums (definition: DESIGN.md section 34).

The tournament form, `tournament_scenarios` (bpl/neutral_dixon_coles.py, csrc/dc_tscen.hip.h), keys on positions in
the GROUP-fixture list of `simulate_tournament` and counts over its simulations.  Its classes take the margin in the
LISTED orientation, first-listed goals minus second-listed goals, also when a host listed second plays at home, so
"home" and "away" of such a result read "first-listed" and "second-listed"; its targets are "round_0" ..
"round_{R-1}", "winner" and "group_winner".  The result carries the same keys and the same two integer tables, and
every helper below takes it unchanged (definition: DESIGN.md section 36).

The helpers below are pure host functions on a result dict: they re-sum the integer tables and form the floats
again, so a marginal or coarsened result is exactly what the narrower call returns under the same `random_state`."""

from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

from bpl._ffi import SCENARIO_MAX_CAP, SCENARIO_MAX_CELLS, SCENARIO_MAX_KEYS


def _whole(v) -> bool:
    return (isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)))


def check_keys(fixtures, margin_cap, n_fixtures: int) -> Tuple[np.ndarray, np.ndarray]:
    """match_scenarios' `fixtures` and `margin_cap` on a list of n_fixtures: (positions int64 [k], caps int64 [k]).
    ValueError unless the positions are 1..SCENARIO_MAX_KEYS distinct integers in 0..n_fixtures - 1 (no bools, no
    floats), the cap is an integer in 1..SCENARIO_MAX_CAP or one such per key fixture, and the scenarios number at
    most SCENARIO_MAX_CELLS."""
    try:
        keys = list(fixtures)
    except TypeError:
        raise ValueError("fixtures must be a sequence of positions in the fixture list") from None
    if not 1 <= len(keys) <= SCENARIO_MAX_KEYS:
        raise ValueError(f"match_scenarios takes 1..{SCENARIO_MAX_KEYS} key fixtures, not {len(keys)}")
    for f in keys:
        if not _whole(f) or not 0 <= f < n_fixtures:
            raise ValueError(f"a key fixture must be an integer in 0..{n_fixtures - 1}, not {f!r}")
    if len(set(int(f) for f in keys)) != len(keys):
        raise ValueError("the key fixtures must be distinct")
    if _whole(margin_cap):
        caps = [margin_cap] * len(keys)
    else:
        try:
            caps = list(margin_cap)
        except TypeError:
            raise ValueError(f"margin_cap must be an integer in 1..{SCENARIO_MAX_CAP}, or one per key fixture") from None
        if len(caps) != len(keys):
            raise ValueError(f"margin_cap has {len(caps)} entries for {len(keys)} key fixtures")
    for c in caps:
        if not _whole(c) or not 1 <= c <= SCENARIO_MAX_CAP:
            raise ValueError(f"a margin cap must be an integer in 1..{SCENARIO_MAX_CAP}, not {c!r}")
    cells = 1
    for c in caps:
        cells *= 2 * int(c) + 1
    if cells > SCENARIO_MAX_CELLS:
        raise ValueError(f"{cells} scenarios; at most {SCENARIO_MAX_CELLS}")
    return np.array([int(f) for f in keys], dtype=np.int64), np.array([int(c) for c in caps], dtype=np.int64)


def scenario_shape(caps) -> Tuple[int, ...]:
    """The class counts (C_q) of the key fixtures."""
    return tuple(2 * int(c) + 1 for c in caps)


def scenario_margins(caps) -> np.ndarray:
    """int64 [M, k]: the clipped margin of every key fixture in scenario m (+-c reads "by c or more")."""
    shape = scenario_shape(caps)
    classes = np.indices(shape, dtype=np.int64).reshape(len(shape), -1).T
    return np.asarray(caps, dtype=np.int64)[None, :] - classes


def scenario_from_counts(scenario_count, joint_count, n_sims: int) -> Dict[str, np.ndarray]:
    """match_scenarios' derived arrays from its two integer tables ([M], [M, n, K])."""
    sc = np.asarray(scenario_count).astype(np.int64)
    jc = np.asarray(joint_count).astype(np.int64)
    target_count = jc.sum(axis=0)
    target_proba = target_count / n_sims
    scenario_proba = sc / n_sims
    of = sc[:, None, None]
    seen = of > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        conditional = np.where(seen, jc / of, np.nan)
        se = np.sqrt(conditional * (1.0 - conditional) / of)
    settled = np.where(seen & (jc == of), 1, np.where(seen & (jc == 0), -1, 0)).astype(np.int8)
    moved = np.where(seen, np.abs(conditional - target_proba[None]), 0.0)
    # (a running sum in scenario order, whatever the shape: a scenario that never occurred adds 0.0)
    leverage = np.cumsum(scenario_proba[:, None, None] * moved, axis=0)[-1]
    return {
        "scenario_count": sc, "scenario_proba": scenario_proba,
        "target_count": target_count, "target_proba": target_proba,
        "joint_count": jc, "conditional_proba": conditional, "conditional_se": se,
        "settled": settled, "leverage": leverage,
    }


def _rebuild(result, order, caps, scenario_count, joint_count) -> Dict[str, np.ndarray]:
    """A result for the key fixtures `order` (positions in result's key list) with `caps`, from re-summed tables."""
    order = [int(q) for q in order]
    caps = np.asarray(caps, dtype=np.int64)
    out = {"teams": result["teams"], "targets": result["targets"],
           "fixtures": np.asarray(result["fixtures"])[order], "home": np.asarray(result["home"])[order],
           "away": np.asarray(result["away"])[order], "margin_cap": caps, "shape": scenario_shape(caps),
           "margins": scenario_margins(caps)}
    n_sims = int(np.asarray(result["scenario_count"]).sum())
    out.update(scenario_from_counts(scenario_count.reshape(-1), joint_count.reshape((-1,) + joint_count.shape[-2:]),
                                    n_sims))
    return out


def _tables(result):
    shape = tuple(int(c) for c in result["shape"])
    sc = np.asarray(result["scenario_count"]).astype(np.int64).reshape(shape)
    jc = np.asarray(result["joint_count"]).astype(np.int64)
    return shape, sc, jc.reshape(shape + jc.shape[1:])


def marginal(result, keep) -> Dict[str, np.ndarray]:
    """The result for some of the key fixtures: `keep` lists positions in the result's key list (0 = the first key
    fixture), distinct and at least one; the count tables are summed over the others and the kept ones come in the
    order of `keep`.  Under one `random_state` this equals the call that names only those key fixtures."""
    shape, sc, jc = _tables(result)
    k = len(shape)
    keep = list(keep)
    if not keep or any(not _whole(q) or not 0 <= q < k for q in keep) or len(set(int(q) for q in keep)) != len(keep):
        raise ValueError(f"keep must list distinct positions in 0..{k - 1} of the key fixtures, at least one")
    keep = [int(q) for q in keep]
    drop = tuple(q for q in range(k) if q not in keep)
    left = [q for q in range(k) if q in keep]            # the axes that remain, in their old order
    turn = [left.index(q) for q in keep]
    sc = sc.sum(axis=drop).transpose(turn)
    jc = jc.sum(axis=drop).transpose(turn + [len(keep), len(keep) + 1])
    return _rebuild(result, keep, np.asarray(result["margin_cap"])[keep], np.ascontiguousarray(sc),
                    np.ascontiguousarray(jc))


def coarsen(result, margin_cap) -> Dict[str, np.ndarray]:
    """The result with smaller margin caps: `margin_cap` is one integer, or one per key fixture, each in 1..the
    fixture's present cap; the margin classes beyond a new cap are merged into its outer classes by summing.  Under
    one `random_state` this equals the call made with the smaller caps."""
    shape, sc, jc = _tables(result)
    old = [int(c) for c in result["margin_cap"]]
    try:
        new = [margin_cap] * len(old) if _whole(margin_cap) else list(margin_cap)
    except TypeError:
        new = []
    if len(new) != len(old) or any(not _whole(c) or not 1 <= c <= o for c, o in zip(new, old)):
        raise ValueError("margin_cap must be an integer, or one per key fixture, each in 1..the fixture's present cap")
    new = [int(c) for c in new]
    for q, (o, c) in enumerate(zip(old, new)):
        to = c - np.clip(o - np.arange(2 * o + 1), -c, c)      # old class -> new class
        merged = []
        for table in (sc, jc):
            table = np.moveaxis(table, q, 0)
            acc = np.zeros((2 * c + 1,) + table.shape[1:], dtype=np.int64)
            np.add.at(acc, to, table)
            merged.append(np.moveaxis(acc, 0, q))
        sc, jc = merged
    return _rebuild(result, range(len(old)), new, np.ascontiguousarray(sc), np.ascontiguousarray(jc))


def _row(result, key, value, what) -> int:
    names = [str(v) for v in result[key]]
    if _whole(value):
        if not 0 <= value < len(names):
            raise ValueError(f"{what} {value} outside 0..{len(names) - 1}")
        return int(value)
    if str(value) not in names:
        raise ValueError(f"unknown {what} {value!r}")
    return names.index(str(value))


def requirements(result, team, target, level: float = 1.0, min_count: int = 1) -> np.ndarray:
    """What it takes: the rows of `margins` (int64 [R, k], in scenario order) of the scenarios seen at least
    `min_count` >= 1 times whose conditional probability that `team` finishes inside `target` reaches `level`
    (0 < level <= 1).  `team` and `target` are names, or rows of "teams" / "targets".  At level 1.0 these are the
    scenarios with settled = +1: about the simulated seasons, not a mathematical guarantee."""
    t, k = _row(result, "teams", team, "team"), _row(result, "targets", target, "target")
    if not _whole(min_count) or min_count < 1:
        raise ValueError("min_count must be an integer >= 1")
    if not 0.0 < float(level) <= 1.0:
        raise ValueError("level must be in (0, 1]")
    sc = np.asarray(result["scenario_count"])
    often = sc >= min_count
    reach = np.zeros(sc.shape, dtype=bool)
    reach[often] = np.asarray(result["conditional_proba"])[often, t, k] >= float(level)
    return np.asarray(result["margins"])[reach]


def _margin_text(margin: int, cap: int) -> str:
    if margin == 0:
        return "draw"
    side, by = ("home", margin) if margin > 0 else ("away", -margin)
    return f"{side} by {by}{'+' if by == cap else ''}"


def format_table(result, team, target) -> str:
    """A readable table of the scenarios that occurred, most frequent first: the key fixtures' results, how often the
    scenario came up and how often `team` then finished inside `target`."""
    t, k = _row(result, "teams", team, "team"), _row(result, "targets", target, "target")
    caps = [int(c) for c in result["margin_cap"]]
    heads = [f"{h} v {a}" for h, a in zip(result["home"], result["away"])]
    sc, jc = np.asarray(result["scenario_count"]), np.asarray(result["joint_count"])[:, t, k]
    order = [m for m in np.argsort(-sc, kind="stable") if sc[m] > 0]
    rows = [heads + ["P(scenario)", "count", f"P({result['targets'][k]} | scenario)", "settled"]]
    for m in order:
        cells = [_margin_text(int(v), c) for v, c in zip(result["margins"][m], caps)]
        mark = {1: "yes", -1: "no", 0: ""}[int(result["settled"][m, t, k])]
        rows.append(cells + [f"{result['scenario_proba'][m]:.4f}", str(int(sc[m])), f"{int(jc[m]) / int(sc[m]):.4f}", mark])
    widths = [max(len(r[i]) for r in rows) for i in range(len(rows[0]))]
    lines = [f"{result['teams'][t]}: {result['targets'][k]} {result['target_proba'][t, k]:.4f} overall, "
             f"{len(order)} of {sc.size} scenarios occurred"]
    lines += ["  ".join(c.ljust(w) for c, w in zip(r, widths)).rstrip() for r in rows]
    return "\n".join(lines)
