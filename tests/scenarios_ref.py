"""match_scenarios restated in numpy (csrc/dc_scenario.hip.h, bpl/scenarios.py): the cross-tabulation of
per-simulation finishing positions and scorelines -- what simulate_season(return_tables=True, return_scores=True)
gives -- into the two integer count tables, the derived arrays written out cell by cell from their definitions, and
plain-loop versions of `marginal` and `coarsen`."""
import itertools

import numpy as np


def shape_of(key_cap):
    return tuple(2 * int(c) + 1 for c in key_cap)


def margins(key_cap):
    """[M, k]: the clipped margin of every key fixture in scenario m, scenarios in row-major order."""
    rows = [[int(c) - j for c, j in zip(key_cap, classes)]
            for classes in itertools.product(*[range(C) for C in shape_of(key_cap)])]
    return np.array(rows, dtype=np.int64).reshape(len(rows), len(key_cap))


def index(home_goals, away_goals, key_fixture, key_cap):
    """home_goals / away_goals [N, F] -> the scenario index [N] of every simulation."""
    x, y = np.asarray(home_goals).astype(np.int64), np.asarray(away_goals).astype(np.int64)
    m = np.zeros(x.shape[0], dtype=np.int64)
    for f, c in zip(key_fixture, key_cap):           # row-major: the last key fixture runs fastest
        m = m * (2 * int(c) + 1) + (int(c) - np.clip(x[:, int(f)] - y[:, int(f)], -int(c), int(c)))
    return m


def counts(position, home_goals, away_goals, inside, key_fixture, key_cap):
    """position [N, n] (slot -> finishing position), home_goals / away_goals [N, F], inside [K, n] (target, position)
    -> scenario_count int64 [M], joint_count int64 [M, n, K]."""
    position = np.asarray(position).astype(np.int64)
    N, n = position.shape
    M = int(np.prod(shape_of(key_cap)))
    m = index(home_goals, away_goals, key_fixture, key_cap)
    scenario = np.zeros(M, dtype=np.int64)
    np.add.at(scenario, m, 1)
    B = np.asarray(inside).T[position].astype(np.int64)                      # [N, n, K]: slot's position in k
    joint = np.zeros((M,) + B.shape[1:], dtype=np.int64)
    np.add.at(joint, m, B)
    return scenario, joint


def derived(scenario_count, joint_count, n_sims):
    """The host-side arrays from the integer tables, one cell at a time."""
    M, n, K = joint_count.shape
    out = {
        "scenario_proba": np.empty(M), "target_count": np.zeros((n, K), dtype=np.int64),
        "target_proba": np.empty((n, K)),
        "conditional_proba": np.full((M, n, K), np.nan), "conditional_se": np.full((M, n, K), np.nan),
        "settled": np.zeros((M, n, K), dtype=np.int8), "leverage": np.zeros((n, K)),
    }
    for t in range(n):
        for k in range(K):
            total = sum(int(v) for v in joint_count[:, t, k])
            out["target_count"][t, k] = total
            out["target_proba"][t, k] = total / n_sims
    for m in range(M):
        of = int(scenario_count[m])
        out["scenario_proba"][m] = of / n_sims
        if of == 0:
            continue
        for t in range(n):
            for k in range(K):
                j = int(joint_count[m, t, k])
                p = j / of
                out["conditional_proba"][m, t, k] = p
                out["conditional_se"][m, t, k] = np.sqrt(p * (1 - p) / of)
                out["settled"][m, t, k] = 1 if j == of else (-1 if j == 0 else 0)
                out["leverage"][t, k] += (of / n_sims) * abs(p - out["target_proba"][t, k])
    return out


def marginal(scenario_count, joint_count, key_cap, keep):
    """The tables of the key fixtures `keep` (positions in the key list, in that order), by plain loops."""
    shape = shape_of(key_cap)
    kept = tuple(shape[q] for q in keep)
    sc = np.zeros(kept, dtype=np.int64)
    jc = np.zeros(kept + joint_count.shape[1:], dtype=np.int64)
    for m, classes in enumerate(itertools.product(*[range(C) for C in shape])):
        at = tuple(classes[q] for q in keep)
        sc[at] += int(scenario_count[m])
        jc[at] += joint_count[m]
    return sc.reshape(-1), jc.reshape((-1,) + joint_count.shape[1:])


def coarsen(scenario_count, joint_count, key_cap, new_cap):
    """The tables under the smaller caps `new_cap` (one per key fixture), by plain loops."""
    shape = shape_of(key_cap)
    small = shape_of(new_cap)
    sc = np.zeros(small, dtype=np.int64)
    jc = np.zeros(small + joint_count.shape[1:], dtype=np.int64)
    for m, classes in enumerate(itertools.product(*[range(C) for C in shape])):
        at = []
        for j, c, c2 in zip(classes, key_cap, new_cap):
            margin = int(c) - j
            at.append(int(c2) - max(-int(c2), min(int(c2), margin)))
        sc[tuple(at)] += int(scenario_count[m])
        jc[tuple(at)] += joint_count[m]
    return sc.reshape(-1), jc.reshape((-1,) + joint_count.shape[1:])
