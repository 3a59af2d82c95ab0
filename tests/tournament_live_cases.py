"""The shapes of the live-tournament tests (tests/test_tournament_live_host.py on the CPU,
tests/test_gpu_tournament_live.py on the device) and their restatements, each computed once and shared.  The shapes
are the smallest at which the kernels can still go wrong, N = 2000 simulations each:

  A   eight teams in two groups of four, the top two through, a bracket of four.  F = 66 ordinary fixtures (the two
      round robins five and a half times over: more than 64, the lane-stride loop of the group stage wraps) and L = 3
      in play: one at 0-0 with elapsed 0 (the kick-off law), one with the HOST listed second (the sides and the two
      goal counts swap), one at 2-1 (no tau cell remains).  S = 300 draws: no multiple of the scan's 256 segments.
  B   nine teams in three groups of three, the winners and the best second through, with and without a 3-row
      allocation table.  F = 0 and L = 2; S = 40 draws, fewer than the 64 lanes of the search; the WC class with
      confederations and a host.
  C   a knockout-only bracket of eight with `log_weights` alone, S = 40.

The seeds were run through the restatement on the CPU; tests/test_tournament_live_host.py asserts without a GPU that
it flags at most 1 % of the simulations of every case below."""
import functools

import numpy as np

import allocation_cases as AC
import tournament_live_ref as TLR
import tournament_ref as TR
from bpl import NeutralDixonColesMatchPredictor, NeutralDixonColesMatchPredictorWC
from bpl.base import _prng_key
from test_tournament_host import conf_of, hand_posterior

N, SEED = 2000, 4242
MODE_IDS = AC.MODE_IDS   # {overall, h2h} x {redraw, extra_time}
KEYS = ("home_team", "away_team", "home_goals", "away_goals", "elapsed")


def _round_robin(members):
    return [(p, q) for i, p in enumerate(members) for q in members[i + 1:]]


@functools.lru_cache(maxsize=None)
def shape(name):
    """(model, the format keywords with group_fixtures, hosts, team_conf, in_play, the allocation table or None)."""
    if name == "A":
        m = hand_posterior(NeutralDixonColesMatchPredictor, T=8, S=300, seed=71)
        t = list(m.teams)
        groups = {"A": t[0:4], "B": t[4:8]}
        rr = _round_robin(groups["A"]) + _round_robin(groups["B"])
        fixtures = (rr * 6)[:66]
        kw = {"groups": groups, "advance": 2, "best_of_rest": 0, "group_fixtures": fixtures,
              "knockout": [("A", 1), ("B", 2), ("B", 1), ("A", 2)]}
        ip = {"home_team": ["t02", "t00", "t05"], "away_team": ["t03", "t01", "t06"], "home_goals": [0, 1, 2],
              "away_goals": [0, 0, 1], "elapsed": [0.0, 0.55, 0.7]}
        return m, kw, ["t01"], None, ip, None
    if name == "B":
        m = hand_posterior(NeutralDixonColesMatchPredictorWC, T=9, S=40, seed=72)
        t = list(m.teams)
        groups = {"A": t[0:3], "B": t[3:6], "C": t[6:9]}
        kw = {"groups": groups, "advance": 1, "best_of_rest": 1, "group_fixtures": [],
              "knockout": [("A", 1), ("best", 1), ("B", 1), ("C", 1)]}
        ip = {"home_team": ["t00", "t07"], "away_team": ["t01", "t06"], "home_goals": [1, 0], "away_goals": [1, 3],
              "elapsed": [0.4, 0.85]}
        table = {("A",): ("A",), ("B",): ("B",), ("C",): ("C",)}
        return m, kw, ["t06"], conf_of(m), ip, table
    if name == "C":
        m = hand_posterior(NeutralDixonColesMatchPredictor, T=8, S=40, seed=73)
        return m, {"knockout": list(m.teams)}, ["t03"], None, None, None
    raise KeyError(name)


def current_table(name):
    """A table to start from: the matches already played are not restated, only their totals matter."""
    m = shape(name)[0]
    return {t: (i % 4, 1 + i % 3, i % 2) for i, t in enumerate(m.teams)}


def log_weights(name):
    S = np.asarray(shape(name)[0].corr_coef).size
    return np.random.RandomState(5).normal(0.0, 1.0, S)


def call(name, mode_id, table=False, with_lw=False, in_play="shape", reweight=True, n_sims=N, seed=SEED):
    """(model, the public call's keywords, the checked inputs, the device call) of a shape in a mode; `table`: under
    the shape's allocation table; in_play: "shape" (the shape's states) or a dict or None."""
    m, kw, hosts, conf, ip, alloc = shape(name)
    ip = ip if isinstance(in_play, str) else in_play
    rounds = len(kw["knockout"]).bit_length() - 1
    tiebreak, rule = AC.mode(mode_id, rounds)
    grouped = "groups" in kw
    common = dict(num_simulations=n_sims, random_state=seed, hosts=hosts, tiebreak=tiebreak, **kw, **rule)
    if grouped:
        common["current_table"] = current_table(name)
    if conf is not None:
        common["team_conf"] = conf
    if table:
        common["best_allocation"] = alloc
    lw = log_weights(name) if with_lw else None
    live = dict(in_play=ip, reweight=reweight, log_weights=lw)
    inp, dev = m._tournament_call(
        kw["knockout"], kw.get("groups"), kw.get("advance", 2), kw.get("best_of_rest", 0), kw.get("group_fixtures"),
        common.get("current_table"), hosts, (3, 1, 0), n_sims, seed, conf, tiebreak, None,
        rule.get("knockout_rule", "redraw"), rule.get("legs"), rule.get("extra_time_scale", 1 / 3), rule.get("shootout"),
        rule.get("away_goals", False), alloc if table else None, ip, lw, True)
    return m, dict(common, **live), inp, dev


# every restatement the GPU test compares against: (shape, mode, table, with log_weights)
GPU_CASES = ([("A", mode_id, False, lw) for mode_id in MODE_IDS for lw in (False, True)]
             + [("B", mode_id, table, lw) for mode_id in MODE_IDS for table in (False, True) for lw in (False, True)]
             + [("C", mode_id, False, True) for mode_id in ("overall-redraw", "overall-extra_time")])


@functools.lru_cache(maxsize=None)
def restatement(name, mode_id, table, with_lw):
    m, common, inp, dev = call(name, mode_id, table, with_lw)
    return TLR.simulate_tournament_live(
        TR.model_tables(m), inp, _prng_key(SEED), inp["in_play"], True, common["log_weights"],
        head_to_head=common["tiebreak"] == "head_to_head", pair_init=dev["kwargs"].get("pair_init"))


def kick_off(name):
    """The shape's matches in play as kick-off states, and the same matches as (home, away) pairs."""
    ip = shape(name)[4]
    k = len(ip["home_team"])
    states = dict(ip, home_goals=[0] * k, away_goals=[0] * k, elapsed=[0.0] * k)
    return states, list(zip(ip["home_team"], ip["away_team"]))
