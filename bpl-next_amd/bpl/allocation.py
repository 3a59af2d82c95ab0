"""Best-of-rest allocation tables for the tournament simulators (no reference counterpart): which bracket position a
qualifier placed advance + 1 takes, by WHICH groups those qualifiers come from -- the Euros since 2016 (4 of 6 thirds,
15 combinations), the World Cup from 2026 (8 of 12 thirds, 495 combinations) -- instead of by its rank among them.

A table is a mapping {groups: groups in slot order}: a key is the B = best_of_rest groups whose team placed
advance + 1 qualified, a tuple or frozenset of group names in any order; its value lists the same B groups so that
element k - 1 is the group whose team takes the bracket position of the knockout entry ("best", k).  It has one row
for every combination of B of the groups that have a place advance + 1.  `simulate_tournament`, `tournament_paths`,
`tournament_scenarios` and `tournament_points` (bpl/neutral_dixon_coles.py) take it as `best_allocation`, checked by
`check`; the device reads it as the two arrays of `device_tables` (include/bplhip.h,
bplhip_tournament_set_allocation).

No organiser's table is shipped.  `from_constraints` builds a complete table from the rule behind one ("slot k may
not take the third of these groups"), but an organiser's published table may pick a different valid matching for a
combination: pass the published table for the official bracket.

Pure host functions, numpy only."""

from __future__ import annotations

from collections.abc import Mapping
from itertools import combinations
from math import comb
from typing import Dict, Sequence, Tuple

import numpy as np

MAX_ROWS = 12870   # include/bplhip.h BPLHIP_TOURNAMENT_MAX_ALLOCATION_ROWS: C(16, 8), what a u16 row index holds


def _eligible(groups, advance) -> Tuple[list, list]:
    """(all group names in order, those with a place advance + 1).  `groups` is simulate_tournament's {name: [teams]},
    or a plain sequence of names, every one of which then counts as large enough."""
    names = list(groups)
    if isinstance(groups, Mapping):
        return names, [g for g in names if len(groups[g]) > advance]
    return names, names


def _rows(n_eligible: int, best: int) -> int:
    """C(n_eligible, best), refused before anything is enumerated when the device arrays cannot hold it."""
    rows = comb(n_eligible, best)
    if rows > MAX_ROWS:
        raise ValueError(f"best_allocation: {best} of {n_eligible} groups are {rows} combinations; at most {MAX_ROWS}")
    return rows


def check(table, groups, best_of_rest: int, advance: int = 2) -> Dict[tuple, tuple]:
    """The validator behind `best_allocation`: `table` against `groups` (simulate_tournament's {name: [teams]}, or a
    sequence of names), B = `best_of_rest` and `advance`.  Returns the table in one form -- {key: value}, the key a
    tuple of group names in the order of `groups`, the value the tuple of the same names in slot order, the rows in
    the order of itertools.combinations -- or raises ValueError: not a mapping; an unknown group; a group without a
    place advance + 1; a key that is not B distinct groups; a value that is not a permutation of its key; a
    combination that is missing or given twice."""
    if not isinstance(table, Mapping):
        raise ValueError("best_allocation must be a mapping {groups: the same groups in slot order}, not "
                         f"{type(table).__name__}")
    names, eligible = _eligible(groups, advance)
    best = int(best_of_rest)
    if not 1 <= best <= len(eligible):
        raise ValueError(f"best_allocation needs best_of_rest in [1, {len(eligible)}] (groups with a place "
                         f"{advance + 1}), not {best_of_rest!r}")
    rows = _rows(len(eligible), best)
    order = {g: i for i, g in enumerate(names)}
    found = {}
    for key, value in table.items():
        try:
            members = list(key) if isinstance(key, (tuple, frozenset, set, list)) else None
            slots = list(value) if not isinstance(value, (str, bytes)) else None
        except TypeError:
            members = slots = None
        if members is None or slots is None:
            raise ValueError(f"best_allocation: the row {key!r}: {value!r} must map a tuple or frozenset of groups to a "
                             "sequence of groups")
        for g in members + slots:
            try:
                known = g in order
            except TypeError:
                known = False
            if not known:
                raise ValueError(f"best_allocation: unknown group {g!r}")
            if g not in eligible:
                raise ValueError(f"best_allocation: group {g!r} has no place {advance + 1}")
        if len(members) != best or len(set(members)) != best:
            raise ValueError(f"best_allocation: the key {tuple(members)!r} must name {best} distinct groups")
        canon = tuple(sorted(members, key=order.get))
        if len(slots) != best or set(slots) != set(members):
            raise ValueError(f"best_allocation[{canon!r}]: {tuple(slots)!r} is not a permutation of its key")
        if canon in found:
            raise ValueError(f"best_allocation: the combination {canon!r} appears twice")
        found[canon] = tuple(slots)
    out = {}
    for combo in combinations(eligible, best):
        if combo not in found:
            raise ValueError(f"best_allocation: the combination {combo!r} is missing ({len(found)} of {rows} rows)")
        out[combo] = found[combo]
    return out


def _matchable(slots, groups, allowed) -> bool:
    """Whether the slots (indices into `allowed`) can each take a different one of `groups`: augmenting paths."""
    taken = {}

    def place(k, seen):
        for g in groups:
            if g in allowed[k] and g not in seen:
                seen.add(g)
                if g not in taken or place(taken[g], seen):
                    taken[g] = k
                    return True
        return False

    return all(place(k, set()) for k in slots)


def from_constraints(groups, allowed: Sequence, advance: int = 2) -> Dict[tuple, tuple]:
    """A complete allocation table from the rule behind one.  `groups` is simulate_tournament's {name: [teams]} or a
    sequence of group names; `allowed[k - 1]` is the collection of groups whose team placed advance + 1 may take
    slot k (the bracket position of ("best", k)), so B = len(allowed) -- "never the slot that meets your own group's
    winner" is the usual rule.  For every combination of B groups with a place advance + 1 the row is the
    lexicographically first perfect matching: slot 1 takes the earliest group (in the order of `groups`) that leaves
    the other slots a matching, then slot 2, and so on.  ValueError naming the first combination (in the order of
    itertools.combinations) that has no perfect matching.  Deterministic; `check` accepts its result.

    An organiser's published table may pick a DIFFERENT valid matching for a combination: this function knows the
    rule, not the table.  For the official bracket pass the official table."""
    names, eligible = _eligible(groups, advance)
    allowed = [frozenset(a) for a in allowed]
    best = len(allowed)
    if not 1 <= best <= len(eligible):
        raise ValueError(f"allowed must list 1..{len(eligible)} slots (groups with a place {advance + 1}), not {best}")
    for k, a in enumerate(allowed):
        for g in a:
            if g not in names:
                raise ValueError(f"allowed[{k}]: unknown group {g!r}")
    _rows(len(eligible), best)
    out = {}
    for combo in combinations(eligible, best):
        if not _matchable(range(best), combo, allowed):
            raise ValueError(f"the combination {combo!r} has no perfect matching under `allowed`")
        left, row = list(combo), []
        for k in range(best):
            for g in left:
                rest = [h for h in left if h != g]
                if g in allowed[k] and _matchable(range(k + 1, best), rest, allowed):
                    row.append(g)
                    left = rest
                    break
        out[combo] = tuple(row)
    return out


def device_tables(table: Dict[tuple, tuple], group_names) -> Dict[str, np.ndarray]:
    """A checked table (`check`'s result) as the device reads it, with G = len(group_names): "row_of_mask" uint16
    [1 << G], the row of the set of groups with bits m (bit g = group g of `group_names`; 0 for a mask that is no
    row's), and "slots" uint8 [rows, G], in row r the 0-based slot of group g's team, 0xFF for a group outside the
    row; "best" is B."""
    order = {g: i for i, g in enumerate(group_names)}
    row_of_mask = np.zeros(1 << len(order), dtype=np.uint16)
    slots = np.full((len(table), len(order)), 0xFF, dtype=np.uint8)
    best = 0
    for r, (key, value) in enumerate(table.items()):
        row_of_mask[sum(1 << order[g] for g in key)] = r
        for k, g in enumerate(value):
            slots[r, order[g]] = k
        best = len(value)
    return {"row_of_mask": row_of_mask, "slots": slots, "best": best}


def format_table(table) -> str:
    """A table as text, one row per combination: the qualifying groups, then the group of every slot."""
    rows = list(table.items())
    if not rows:
        return "(empty allocation table)"
    best = len(rows[0][1])
    head = "groups".ljust(max(6, max(len(" ".join(map(str, k))) for k, _ in rows)))
    lines = [head + "  " + "  ".join(f"best {k + 1}" for k in range(best))]
    for key, value in rows:
        lines.append(" ".join(map(str, key)).ljust(len(head)) + "  " +
                     "  ".join(str(g).ljust(len(f"best {k + 1}")) for k, g in enumerate(value)))
    return "\n".join(lines)
