"""The shapes of the live tournament-query tests (tests/test_tournament_live_queries_host.py on the CPU,
tests/test_gpu_tournament_live_queries.py on the device) and their restatements, each computed once and shared.  They
are tests/tournament_live_cases.py's shapes with its seeds, N = 2000 simulations each, plus one of their own:

  A    two groups of four, F = 66 > 64 ordinary fixtures and L = 3 in play (0-0 at 0, a host listed second, 2-1),
       S = 300.  Scenario keys: fixture 65, an ordinary fixture in the second block of 64, then F + 1 (the swapped
       one) and F + 2, with caps (1, 2, 3).
  A2   shape A with `group_fixtures` cut to F = 62 and a fourth state, L = 4: the matches in play are fixtures 62..65
       of the concatenated list and straddle the 64-fixture block boundary, so the first two share a ballot block with
       the last ordinary fixtures.  Keys 63 and 64, one on each side of the boundary, caps (2, 1).
  B    the WC class, three groups of three, F = 0 and L = 2, S = 40 < 64 lanes, confederations and a host, with and
       without its 3-row allocation table: every fixture of the axis is in play.  Keys 0 and 1, caps (1, 3): at 0-3
       after 85 % the second key has classes the score has ruled out.
  C    a knockout-only bracket of eight with `log_weights` alone: `tournament_paths` only.

The seeds were run through the restatement on the CPU; tests/test_tournament_live_queries_host.py asserts without a GPU
that it flags at most 1 % of the simulations of every case the device's tables are compared against."""
import functools

import numpy as np

import allocation_cases as AC
import tournament_live_cases as C
import tournament_live_queries_ref as QR
import tournament_ref as TR
from bpl.base import _prng_key

N, SEED = C.N, C.SEED
MODE_IDS = C.MODE_IDS
LIVE_KEYS = ("in_play", "reweight", "log_weights")
# the scenario keys (positions in the concatenated list) and their caps
KEYS = {"A": ((65, 67, 68), (1, 2, 3)), "A2": ((63, 64), (2, 1)), "B": ((0, 1), (1, 3))}


@functools.lru_cache(maxsize=None)
def shape(name):
    """tournament_live_cases.shape, and A2 derived from its A."""
    if name != "A2":
        return C.shape(name)
    m, kw, hosts, conf, ip, alloc = C.shape("A")
    kw = dict(kw, group_fixtures=list(kw["group_fixtures"])[:62])
    more = {"home_team": "t04", "away_team": "t07", "home_goals": 0, "away_goals": 2, "elapsed": 0.3}
    return m, kw, hosts, conf, {k: list(v) + [more[k]] for k, v in ip.items()}, alloc


def _base(name):
    return "A" if name == "A2" else name


def call(name, mode_id, table=False, with_lw=False, in_play="shape", reweight=True, n_sims=N, seed=SEED):
    """tournament_live_cases.call on this file's shapes: (model, the public keywords shared by the three queries and
    simulate_tournament, the checked inputs, the device call)."""
    m, kw, hosts, conf, ip, alloc = shape(name)
    ip = ip if isinstance(in_play, str) else in_play
    rounds = len(kw["knockout"]).bit_length() - 1
    tiebreak, rule = AC.mode(mode_id, rounds)
    common = dict(num_simulations=n_sims, random_state=seed, hosts=hosts, tiebreak=tiebreak, **kw, **rule)
    if "groups" in kw:
        common["current_table"] = C.current_table(_base(name))
    if conf is not None:
        common["team_conf"] = conf
    if table:
        common["best_allocation"] = alloc
    lw = C.log_weights(_base(name)) if with_lw else None
    inp, dev = m._tournament_call(
        kw["knockout"], kw.get("groups"), kw.get("advance", 2), kw.get("best_of_rest", 0), kw.get("group_fixtures"),
        common.get("current_table"), hosts, (3, 1, 0), n_sims, seed, conf, tiebreak, None,
        rule.get("knockout_rule", "redraw"), rule.get("legs"), rule.get("extra_time_scale", 1 / 3), rule.get("shootout"),
        rule.get("away_goals", False), alloc if table else None, ip, lw, True)
    return m, dict(common, in_play=ip, reweight=reweight, log_weights=lw), inp, dev


def kick_off(name):
    """The shape's matches in play as kick-off states, and the same matches as (home, away) pairs."""
    ip = shape(name)[4]
    k = len(ip["home_team"])
    return dict(ip, home_goals=[0] * k, away_goals=[0] * k, elapsed=[0.0] * k), list(zip(ip["home_team"], ip["away_team"]))


def plain(common, pairs=()):
    """The public keywords without the live ones, `pairs` appended to the group fixtures."""
    kw = {k: v for k, v in common.items() if k not in LIVE_KEYS}
    if pairs:
        kw["group_fixtures"] = list(kw["group_fixtures"]) + list(pairs)
    return kw


# simulation j is simulation j: tournament_live_cases.GPU_CASES' pattern, and A2 in every mode
GPU_CASES = C.GPU_CASES + [("A2", mode_id, False, lw) for mode_id in MODE_IDS for lw in (False, True)]
# the cases whose tables are compared against the restatement
REF_CASES = ([("A", mode_id, False, True) for mode_id in MODE_IDS]
             + [("A2", mode_id, False, False) for mode_id in MODE_IDS] + [("A2", "overall-redraw", False, True)]
             + [("B", mode_id, table, True) for mode_id in MODE_IDS for table in (False, True)]
             + [("C", mode_id, False, True) for mode_id in ("overall-redraw", "overall-extra_time")])
KICK_OFF = ([(name, mode_id, False) for name in ("A", "A2") for mode_id in MODE_IDS]
            + [("B", mode_id, table) for mode_id in MODE_IDS for table in (False, True)])


@functools.lru_cache(maxsize=None)
def restatement(name, mode_id, table, with_lw):
    m, common, inp, dev = call(name, mode_id, table, with_lw)
    return QR.simulate(TR.model_tables(m), inp, _prng_key(SEED), inp["in_play"], True, common["log_weights"],
                       head_to_head=common["tiebreak"] == "head_to_head", pair_init=dev["kwargs"].get("pair_init"))


def listed_margin(res):
    """int64 [N, L]: the final margins of the matches in play in the listed order, from a result's records."""
    return res["in_play_home_goals"].astype(np.int64) - res["in_play_away_goals"].astype(np.int64)
