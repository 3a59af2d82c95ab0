"""The tournament shapes of the `best_allocation` tests (tests/test_allocation_host.py on the CPU,
tests/test_gpu_allocation.py on the device), their tables and their restatements, each computed once and shared.

The posteriors are hand-built with near-equal teams (test_tournament_host.hand_posterior at a fifth of its spread), so
that the thirds of every group qualify often and every combination of a small table occurs.  The seeds were run
through the restatement on the CPU: it flags no simulation of any case (a flag marks a comparison within 1e-12 of its
boundary), and tests/test_allocation_host.py asserts that, and the two conditions of the smallest shape, without a
GPU."""
import functools

import numpy as np

import allocation_ref as A
import knockout_ref as K
import tournament_ref as R
from bpl import allocation
from bpl.base import _prng_key
from test_tournament_host import hand_posterior

SEED, DRAWS = 9753, 7
MODE_IDS = ["overall-redraw", "h2h-redraw", "overall-extra_time", "h2h-extra_time"]
# the third-placed team that may meet the winner of group A, B, C, D in a 24-team European Championship (UEFA's
# published rule for 2016 onwards): slot k meets the k-th of those winners
EURO_ALLOWED = [("C", "D", "E"), ("A", "C", "D"), ("A", "B", "F"), ("B", "E", "F")]


def near_equal(T, seed):
    m = hand_posterior(T=T, S=DRAWS, seed=seed)
    for nm in ("attack", "defence", "home_attack", "away_attack", "home_defence", "away_defence"):
        setattr(m, nm, 0.2 * getattr(m, nm))
    return m


def cyclic_allowed(names, best, skip):
    """Slot k may take every group but names[k] and names[k + skip] (where there is one): "not the groups whose
    qualifiers slot k could meet first"."""
    return [[g for i, g in enumerate(names) if i not in (k, k + skip)] for k in range(best)]


@functools.lru_cache(maxsize=None)
def shape(name):
    """(model, simulate_tournament's format keywords with "best_allocation", hosts, N) of a case."""
    if name == "3x3":
        # the smallest discriminating shape: 3 groups of 3, two of the three thirds, 3 rows that are not all one
        # permutation ((A, C) is turned round), an 8-entry bracket
        m = near_equal(9, 61)
        t = list(m.teams)
        kw = {"groups": {"A": t[0:3], "B": t[3:6], "C": t[6:9]}, "advance": 2, "best_of_rest": 2,
              "knockout": [("A", 1), ("best", 1), ("B", 1), ("C", 2), ("C", 1), ("best", 2), ("A", 2), ("B", 2)],
              "best_allocation": {("A", "B"): ("A", "B"), ("A", "C"): ("C", "A"), ("B", "C"): ("B", "C")}}
        return m, kw, None, 512
    if name == "one_row":
        # 4 groups of 4, the winners and ALL four seconds as "the best of the rest": one row
        m = near_equal(16, 62)
        t = list(m.teams)
        names = ["A", "B", "C", "D"]
        kw = {"groups": {g: t[4 * i:4 * i + 4] for i, g in enumerate(names)}, "advance": 1, "best_of_rest": 4,
              "knockout": [("A", 1), ("best", 2), ("C", 1), ("best", 4), ("B", 1), ("best", 1), ("D", 1), ("best", 3)],
              "best_allocation": {tuple(names): tuple(names)}}
        return m, kw, None, 700
    if name == "euro24":
        m = near_equal(24, 63)
        kw = R.euro_24(list(m.teams), seed=3)
        kw["best_allocation"] = allocation.from_constraints(kw["groups"], EURO_ALLOWED)
        return m, kw, None, 4096
    if name == "wc48":
        m = near_equal(48, 64)
        kw = R.world_cup_48(list(m.teams), seed=4)
        kw["best_allocation"] = allocation.from_constraints(kw["groups"], cyclic_allowed(list(kw["groups"]), 8, 12))
        return m, kw, ["t05", "t30"], 2000
    if name == "14x3":
        # 14 groups of 3 and the 4 best thirds: 1001 rows, mask bits up to 13
        m = near_equal(42, 65)
        kw = R.group_format(list(m.teams), 14, 3, 4, seed=5)
        kw["best_allocation"] = allocation.from_constraints(kw["groups"], cyclic_allowed(list(kw["groups"]), 4, 4))
        return m, kw, ["t02", "t40"], 2000
    raise KeyError(name)


def mode(mode_id, rounds):
    """(tiebreak, the knockout rule's keywords) of a mode for a bracket of `rounds` rounds."""
    tiebreak = "head_to_head" if mode_id.startswith("h2h") else "overall"
    if mode_id.endswith("redraw"):
        return tiebreak, {}
    if tiebreak == "overall":
        return tiebreak, dict(knockout_rule="extra_time", legs=tuple(2 - r % 2 for r in range(rounds)), away_goals=True,
                              shootout={"t01": 0.8, "t04": -0.4})
    return tiebreak, dict(knockout_rule="extra_time", legs=tuple(1 + r % 2 for r in range(rounds)), shootout={"t03": 1.5})


def call(name, mode_id, allocated=True, n_sims=None, seed=SEED):
    """(the public call's keywords, the checked inputs, the device call) of a case in a mode, the last two as the
    public call itself forms them; allocated=False: the same call without its table."""
    m, kw, hosts, N = shape(name)
    kw = dict(kw)
    table = kw.pop("best_allocation")
    rounds = len(kw["knockout"]).bit_length() - 1
    tiebreak, rule = mode(mode_id, rounds)
    n_sims = N if n_sims is None else n_sims
    extra = {"best_allocation": table} if allocated else {}
    common = dict(num_simulations=n_sims, random_state=seed, hosts=hosts, tiebreak=tiebreak, **kw, **rule, **extra)
    inp, dev = m._tournament_call(kw["knockout"], kw["groups"], kw["advance"], kw["best_of_rest"], None, None, hosts,
                                  (3, 1, 0), n_sims, seed, None, tiebreak, None, rule.get("knockout_rule", "redraw"),
                                  rule.get("legs"), rule.get("extra_time_scale", 1 / 3), rule.get("shootout"),
                                  rule.get("away_goals", False), table if allocated else None)
    return m, common, inp, dev


class allocated_first_round:
    """knockout_ref.first_round replaced by allocation_ref.first_round inside the block (what pytest's monkeypatch
    does for a test, for the cached references here)."""

    def __enter__(self):
        self.saved, K.first_round = K.first_round, A.first_round

    def __exit__(self, *exc):
        K.first_round = self.saved


@functools.lru_cache(maxsize=None)
def reference(name, mode_id):
    """simulate_tournament's raw results by the restatement under the case's table, with "slot_counts", "row" [N]
    and "bracket" [N, 2^R] (the allocated first round)."""
    m, common, inp, dev = call(name, mode_id)
    if name == "3x3":
        # the smallest shape's restatement reads the hand-written mapping itself, not what bpl.allocation.check made
        # of it: nothing of the code under test stands between the table and the reference
        inp = dict(inp, best_allocation=dict(shape(name)[1]["best_allocation"]))
    tables, key = R.model_tables(m), _prng_key(SEED)
    h2h, pair = common["tiebreak"] == "head_to_head", dev["kwargs"].get("pair_init")
    if inp["knockout_rule"] == "redraw":
        return A.simulate_redraw(tables, inp, key, head_to_head=h2h, pair_init=pair)
    with allocated_first_round():
        ref = K.simulate_tournament(tables, inp, key, head_to_head=h2h, pair_init=pair)
    g = A.group_stage(tables, inp, key, np.zeros(inp["num_simulations"], dtype=bool), h2h, pair)
    ref.update(slot_counts=g["slot_counts"], row=g["row"], bracket=g["bracket"])
    return ref


@functools.lru_cache(maxsize=None)
def ranked_first_round(name, mode_id):
    """The rank-seeded first round [N, 2^R] of the same simulations (knockout_ref.first_round without the table)."""
    m, common, inp, dev = call(name, mode_id, allocated=False)
    return K.first_round(R.model_tables(m), inp, _prng_key(SEED), np.zeros(inp["num_simulations"], dtype=bool),
                         common["tiebreak"] == "head_to_head", dev["kwargs"].get("pair_init"))[0]
