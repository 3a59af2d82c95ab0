"""match_leverage restated in numpy (csrc/dc_leverage.hip.h, bpl/base.py): the cross-tabulation of
per-simulation finishing positions and scorelines -- what simulate_season(return_tables=True,
return_scores=True) gives -- into the three integer count tables, and the derived floats written out
cell by cell from their definitions."""
import numpy as np


def target_masks(targets, n):
    """name -> positions (0 = top, negative from the bottom) as [K, n] booleans; positions outside the
    table are dropped."""
    inside = np.zeros((len(targets), n), dtype=bool)
    for k, positions in enumerate(targets.values()):
        for p in positions:
            p = p + n if p < 0 else p
            if 0 <= p < n:
                inside[k, p] = True
    return inside


def counts(position, home_goals, away_goals, inside):
    """position [N, n] (slot -> finishing position), home_goals / away_goals [N, F], inside [K, n]
    (target, position) -> outcome_count int64 [F, 3], target_count [n, K], joint_count [F, 3, n, K];
    o = 0 home win, 1 draw, 2 away win."""
    position = np.asarray(position).astype(np.int64)
    x, y = np.asarray(home_goals).astype(np.int64), np.asarray(away_goals).astype(np.int64)
    N, n = position.shape
    outcome = np.where(x > y, 0, np.where(x == y, 1, 2))                     # [N, F]
    # one-hot in float64: its matrix product goes through BLAS, and counts below 2^53 are exact in it
    A = (outcome[:, :, None] == np.arange(3)).astype(np.float64)             # [N, F, 3]
    B = np.asarray(inside).T[position].astype(np.float64)                    # [N, n, K]: slot's position in k
    F, K = x.shape[1], B.shape[2]
    joint = (A.reshape(N, F * 3).T @ B.reshape(N, n * K)).reshape(F, 3, n, K)
    return A.sum(axis=0).astype(np.int64), B.sum(axis=0).astype(np.int64), joint.astype(np.int64)


def derived(outcome_count, target_count, joint_count, n_sims):
    """The host-side floats from the integer tables, one cell at a time."""
    F, _, n, K = joint_count.shape
    out = {
        "outcome_proba": outcome_count / n_sims,
        "target_proba": target_count / n_sims,
        "conditional_proba": np.full((F, 3, n, K), np.nan),
        "conditional_se": np.full((F, 3, n, K), np.nan),
        "leverage": np.zeros((F, n, K)),
    }
    for f in range(F):
        for o in range(3):
            m = int(outcome_count[f, o])
            if m == 0:
                continue
            for t in range(n):
                for k in range(K):
                    p = int(joint_count[f, o, t, k]) / m
                    out["conditional_proba"][f, o, t, k] = p
                    out["conditional_se"][f, o, t, k] = np.sqrt(p * (1 - p) / m)
                    out["leverage"][f, t, k] += (m / n_sims) * abs(p - int(target_count[t, k]) / n_sims)
    return out
