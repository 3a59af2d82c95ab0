"""numpy restatement of `tournament_scenarios` (bpl/neutral_dixon_coles.py, csrc/dc_tscen.hip.h) for the tests: the
tournament is played by tests/paths_ref.py (which plays it through tournament_ref, h2h_ref and knockout_ref), and the
two per-simulation records are formed here from what it returns:
  scenario    the key fixtures played again from knockout_ref.play's blocks (the same operations, so the same
              scorelines), the margin turned to the LISTED orientation as paths_ref does for group_outcome, the classes
              c - clip(margin, -c, c) combined row-major in the order of the keys;
  target_set  bit k <= R: stage >= k + 1; bit R + 1: position 0 of its group.
`counts` is the pure cross-tabulation of such records -- the device's own or the restatement's -- into the two integer
tables of the result."""
import numpy as np

import knockout_ref as K
import paths_ref as P
import tournament_ref as TR


def strides(caps):
    """Row-major strides of the classes (2 c + 1 per key) and their product M."""
    shape = [2 * int(c) + 1 for c in caps]
    out = [int(np.prod(shape[q + 1:], dtype=np.int64)) for q in range(len(shape))]
    return np.array(out, dtype=np.int64), int(np.prod(shape, dtype=np.int64))


def key_margins(tables, inp, key, keys):
    """int64 [N, k]: first-listed goals minus second-listed goals of the key fixtures in every simulation."""
    N = inp["num_simulations"]
    keys = np.asarray(keys, dtype=np.int64)
    j = np.arange(N, dtype=np.int64)
    s = j % tables["attack"].shape[0]
    fp, fq = inp["fix_p"].astype(np.int64), inp["fix_q"].astype(np.int64)
    J2, F2 = np.meshgrid(j, keys, indexing="ij")
    rows, f = J2.ravel(), F2.ravel()
    hs, as_, on = TR.venue(fp[f], fq[f], inp["host"])
    scratch = np.zeros(N, dtype=bool)   # (the same walks as paths_ref.simulate's: its flags already cover them)
    x, y = K.play(tables, inp, key, rows, s[rows], hs, as_, on, f, 1.0, scratch)
    listed = hs == fp[f]
    return np.where(listed, x - y, y - x).astype(np.int64).reshape(N, keys.size)


def simulate(tables, inp, key, keys, caps, head_to_head=False, pair_init=None):
    """The per-simulation records of `tournament_scenarios` for the checked inputs `inp` (the dict of
    _tournament_inputs, with groups and group fixtures): "scenario" u32 [N], "target_set" u8 [N, n], "stage" and
    "position" (paths_ref's), under "extra_time" "decided", and "flagged" [N], the restatement's own vector."""
    rec = P.simulate(tables, inp, key, head_to_head=head_to_head, pair_init=pair_init)
    R = inp["rounds"]
    caps = np.asarray(caps, dtype=np.int64)
    margin = key_margins(tables, inp, key, keys)
    stride, _ = strides(caps)
    cls = caps[None, :] - np.clip(margin, -caps[None, :], caps[None, :])
    stage = rec["stage"].astype(np.int64)
    tset = ((1 << stage) - 1) | ((rec["position"].astype(np.int64) == 0).astype(np.int64) << (R + 1))
    out = {"scenario": (cls * stride[None, :]).sum(axis=1).astype(np.uint32), "target_set": tset.astype(np.uint8),
           "stage": rec["stage"], "position": rec["position"], "flagged": rec["flagged"]}
    if "decided" in rec:
        out["decided"] = rec["decided"]
    return out


def counts(records, inp, keys, caps):
    """The integer tables of `tournament_scenarios` from per-simulation records: "scenario_count" int64 [M] and
    "joint_count" int64 [M, n, R + 2].  `keys` only fixes how many there are: the records carry the index."""
    assert len(keys) == len(caps)
    _, M = strides(caps)
    scen = np.asarray(records["scenario"]).astype(np.int64)
    tset = np.asarray(records["target_set"]).astype(np.int64)
    N, n = tset.shape
    Kt = inp["rounds"] + 2
    assert scen.shape == (N,) and (scen >= 0).all() and (scen < M).all() and (tset >> Kt == 0).all()
    row = (scen[:, None] * n + np.arange(n)[None, :]).ravel()                            # [N n]: cell (m, slot)
    joint = np.zeros((M, n, Kt), dtype=np.int64)
    for k in range(Kt):
        # (float64 sums of 0 / 1 weights: exact, the counts are far below 2^53)
        joint[:, :, k] = np.bincount(row, weights=((tset >> k) & 1).ravel(), minlength=M * n).reshape(M, n)
    return {"scenario_count": np.bincount(scen, minlength=M).astype(np.int64), "joint_count": joint}
