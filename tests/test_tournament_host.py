"""simulate_tournament without a GPU: every argument check (all made on the host before the device
is touched), the default round robin, the bracket resolution, the host venue swap, the restatement's
invariants and its knockout rule against the posterior draws' scoreline grids."""
import numpy as np
import pytest
from scipy.stats import poisson

import tournament_ref as R
from bpl import NeutralDixonColesMatchPredictor, NeutralDixonColesMatchPredictorWC
from bpl.base import _prng_key

CONFS = np.array(["AFC", "CAF", "UEFA"])


def hand_posterior(cls=NeutralDixonColesMatchPredictor, T=64, S=8, seed=1):
    rs = np.random.RandomState(seed)
    m = cls()
    m.teams = np.array([f"t{i:02d}" for i in range(T)])
    m._teams_dict = {t: i for i, t in enumerate(m.teams)}
    m.attack, m.defence = rs.normal(0, 0.3, (S, T)), rs.normal(0, 0.3, (S, T))
    for nm in ("home_attack", "away_attack", "home_defence", "away_defence"):
        setattr(m, nm, rs.normal(0, 0.1, (S, T)))
    m.corr_coef = rs.uniform(-0.05, 0.05, S)
    if cls is NeutralDixonColesMatchPredictorWC:
        m.conferences = CONFS
        m._conferences_dict = {c: i for i, c in enumerate(CONFS)}
        m.confederation_strength = rs.normal(0, 0.2, (S, len(CONFS)))
    return m


def conf_of(m):
    return {t: CONFS[i % len(CONFS)] for i, t in enumerate(m.teams)}


def _raises(m, *args, **kwargs):
    with pytest.raises(ValueError):
        m.simulate_tournament(*args, **kwargs)
    assert m._predict_ctx is None   # no device context was ever made


def test_argument_checks_run_on_the_host():
    m = hand_posterior()
    t = list(m.teams)
    euro = R.euro_24(t)
    groups, ko = euro["groups"], euro["knockout"]
    kw = dict(advance=2, best_of_rest=4, num_simulations=10)
    # unknown teams, anywhere
    _raises(m, ["t00", "nope"])
    _raises(m, ko, {**groups, "A": ["t00", "nope", "t02", "t03"]}, **kw)
    _raises(m, ko, groups, hosts=["nope"], **kw)
    _raises(m, ko, groups, hosts=["t60"], **kw)                     # known, but not playing
    _raises(m, ko, groups, current_table={"nope": (1, 1, 1)}, **kw)
    _raises(m, ko, groups, current_table={"t60": (1, 1, 1)}, **kw)
    _raises(m, ko, groups, group_fixtures=[("t00", "nope")], **kw)
    # a team in two groups, or twice in one
    _raises(m, ko, {**groups, "B": ["t00", "t05", "t06", "t07"]}, **kw)
    _raises(m, ko, {**groups, "A": ["t00", "t00", "t02", "t03"]}, **kw)
    # group bounds
    _raises(m, ko, {**groups, "A": ["t00"]}, **kw)
    _raises(m, ["t00", "t01"], {f"G{i}": [t[2 * i], t[2 * i + 1]] for i in range(17)}, advance=1)
    _raises(m, ko, {"A": t[:9]}, **kw)
    _raises(m, ko, {"best": t[:4]}, **kw)
    _raises(m, ["t00"] * 8, {**{f"G{i}": t[8 * i:8 * i + 8] for i in range(8)}, "X": ["t62", "t63"]}, advance=1)
    # knockout-only bounds: power of two, 2..64 entries, distinct teams
    _raises(m, t[:3])
    _raises(m, t[:1])
    _raises(m, [])
    _raises(m, ["t00", "t00"])
    m2 = hand_posterior(T=130)
    _raises(m2, list(m2.teams[:128]))
    # unresolvable or repeated bracket references, qualifier count != 2^R
    bad = list(ko)
    bad[0] = ("Z", 1)
    _raises(m, bad, groups, **kw)
    bad[0] = ("A", 3)
    _raises(m, bad, groups, **kw)
    bad[0] = ("best", 5)
    _raises(m, bad, groups, **kw)
    bad[0] = ko[1]
    _raises(m, bad, groups, **kw)
    bad[0] = ("A", 1.0)
    _raises(m, bad, groups, **kw)
    bad[0] = "A1"
    _raises(m, bad, groups, **kw)
    _raises(m, ko, groups, advance=2, best_of_rest=2, num_simulations=10)       # 14 qualifiers for 16
    _raises(m, ko + ko, groups, **kw)                                          # 16 qualifiers for 32
    _raises(m, ko[:12], groups, **kw)                                          # not a power of two
    _raises(m, ko, groups, advance=2, best_of_rest=7, num_simulations=10)      # only 6 thirds
    _raises(m, ko, groups, advance=0, best_of_rest=4, num_simulations=10)
    _raises(m, ko, groups, advance=9, best_of_rest=4, num_simulations=10)
    # fixtures: same group, two different teams, pairs
    _raises(m, ko, groups, group_fixtures=[("t00", "t04")], **kw)
    _raises(m, ko, groups, group_fixtures=[("t00", "t00")], **kw)
    _raises(m, ko, groups, group_fixtures=[("t00", "t01", "t02")], **kw)
    # group-only arguments without groups
    _raises(m, t[:4], group_fixtures=[("t00", "t01")])
    _raises(m, t[:4], current_table={"t00": (1, 1, 1)})
    # table, points, simulation bounds
    for table in ({"t00": (-1, 0, 0)}, {"t00": (0, 1 << 25, 0)}, {"t00": (1, 2)}, {"t00": (1.5, 0, 0)}):
        _raises(m, ko, groups, current_table=table, **kw)
    for points in ((3, -1, 0), (3, 1), (1001, 1, 0), (3.5, 1, 0)):
        _raises(m, ko, groups, points=points, **kw)
    for n in (0, 2 ** 31, 1.5, True):
        _raises(m, t[:4], num_simulations=n)
    # team_conf: given to the wrong class, missing or incomplete for the World-Cup class
    _raises(m, t[:4], team_conf=conf_of(m))
    w = hand_posterior(NeutralDixonColesMatchPredictorWC)
    _raises(w, t[:4])
    _raises(w, t[:4], team_conf={"t00": "AFC", "t01": "AFC", "t02": "AFC"})
    _raises(w, t[:4], team_conf={**conf_of(w), "t03": "CONMEBOL"})


def test_default_round_robin_and_its_order():
    m = hand_posterior()
    groups = {"X": ["t05", "t01", "t09"], "Y": ["t02", "t03", "t04", "t07"]}
    inp = m._tournament_inputs([("X", 1), ("Y", 1), ("X", 2), ("Y", 2)], groups, 2, 0, None, None, None, (3, 1, 0),
                               10, None)
    assert list(inp["teams"]) == ["t05", "t01", "t09", "t02", "t03", "t04", "t07"]
    pairs = [(inp["teams"][p], inp["teams"][q]) for p, q in zip(inp["fix_p"], inp["fix_q"])]
    assert pairs == [("t05", "t01"), ("t05", "t09"), ("t01", "t09"),
                     ("t02", "t03"), ("t02", "t04"), ("t02", "t07"), ("t03", "t04"), ("t03", "t07"), ("t04", "t07")]
    np.testing.assert_array_equal(inp["group"], [0, 0, 0, 1, 1, 1, 1])
    assert inp["rounds"] == 2 and inp["group_size"] == 4
    # given fixtures keep their order and orientation
    inp = m._tournament_inputs([("X", 1), ("Y", 1), ("X", 2), ("Y", 2)], groups, 2, 0, [("t09", "t05"), ("t07", "t02")],
                               {"t05": (3, 2, 1)}, None, (3, 1, 0), 10, None)
    np.testing.assert_array_equal(inp["fix_p"], [2, 6])
    np.testing.assert_array_equal(inp["fix_q"], [0, 3])
    np.testing.assert_array_equal(inp["table"][0], [3, 2, 1])
    assert not inp["table"][1:].any()


def test_bracket_codes():
    m = hand_posterior()
    wc = R.world_cup_48(list(m.teams))
    inp = m._tournament_inputs(wc["knockout"], wc["groups"], 2, 8, None, None, None, (3, 1, 0), 10, None)
    names = list(wc["groups"])
    for b, (ref, place) in enumerate(wc["knockout"]):
        code = int(inp["bracket"][b])
        if ref == "best":
            assert code == 0xFF00 | place
        else:
            assert code == names.index(ref) << 8 | place
    assert inp["rounds"] == 5 and len(set(inp["bracket"].tolist())) == 32
    # without groups the bracket is the slot order, the teams are in bracket order
    ko = ["t10", "t03", "t07", "t01"]
    inp = m._tournament_inputs(ko, None, 2, 0, None, None, ["t07"], (3, 1, 0), 10, None)
    assert list(inp["teams"]) == ko
    np.testing.assert_array_equal(inp["bracket"], np.arange(4))
    np.testing.assert_array_equal(inp["host"], [0, 0, 1, 0])
    np.testing.assert_array_equal(inp["team_idx"], [10, 3, 7, 1])


def test_bracket_resolution_with_best_of_rest():
    # no matches left: the table decides; 3 groups of 3, top one and the best 1 of the seconds
    m = hand_posterior()
    groups = {"A": ["t00", "t01", "t02"], "B": ["t03", "t04", "t05"], "C": ["t06", "t07", "t08"]}
    table = {"t00": (9, 5, 0), "t01": (6, 4, 2), "t02": (0, 0, 9),
             "t03": (1, 1, 1), "t04": (7, 3, 3), "t05": (7, 5, 5),      # t05 ahead of t04 on goals for
             "t06": (4, 2, 2), "t07": (4, 2, 3), "t08": (2, 1, 1)}
    ko = [("A", 1), ("best", 1), ("B", 1), ("C", 1)]
    inp = m._tournament_inputs(ko, groups, 1, 1, [], table, None, (3, 1, 0), 200, None)
    out = R.simulate_tournament(R.model_tables(m), inp, _prng_key(3))
    pos = out["position"]
    assert (pos == [0, 1, 2, 2, 1, 0, 0, 1, 2]).all()
    # qualifiers: the winners t00, t05, t06 and the best second, t04 (7 points against 6 and 4)
    stage = out["stage"]
    assert (stage[:, [0, 4, 5, 6]] >= 1).all() and (stage[:, [1, 2, 3, 7, 8]] == 0).all()
    # round 0: A1 meets the best second t04, B1 meets C1
    champions = stage.argmax(axis=1)
    assert set(np.unique(champions)) <= {0, 4, 5, 6}
    assert ((stage[:, 0] >= 2) ^ (stage[:, 4] >= 2)).all() and ((stage[:, 5] >= 2) ^ (stage[:, 6] >= 2)).all()


def test_tie_break_word_orders_level_teams():
    m = hand_posterior()
    groups = {"A": ["t00", "t01"], "B": ["t02", "t03"]}
    table = {t: (3, 2, 2) for t in ("t00", "t01", "t02", "t03")}
    inp = m._tournament_inputs([("A", 1), ("B", 1)], groups, 1, 0, [], table, None, (3, 1, 0), 4000, None)
    out = R.simulate_tournament(R.model_tables(m), inp, _prng_key(5))
    first = (out["position"][:, 0] == 0).mean()
    assert abs(first - 0.5) < 5 * np.sqrt(0.25 / 4000)


def test_host_venue_swap():
    host = np.array([0, 1, 0, 1], dtype=np.uint8)
    p = np.array([0, 1, 0, 1, 2])
    q = np.array([1, 0, 2, 3, 0])
    hs, as_, on = R.venue(p, q, host)
    np.testing.assert_array_equal(hs, [1, 1, 0, 1, 2])      # the host moves into the home role
    np.testing.assert_array_equal(as_, [0, 0, 2, 3, 0])
    np.testing.assert_array_equal(on, [True, True, False, False, False])   # two hosts or none: neutral
    # and the rates: only an on-venue match carries the home / away offsets
    m = hand_posterior(S=3)
    tabs = R.model_tables(m)
    s = np.arange(3)
    lh0, la0 = R.rates(tabs, s, 4, 9, False)
    lh1, la1 = R.rates(tabs, s, 4, 9, True)
    np.testing.assert_allclose(np.log(lh0), m.attack[:, 4] - m.defence[:, 9], rtol=1e-12)
    np.testing.assert_allclose(np.log(lh1), m.attack[:, 4] - m.defence[:, 9] + m.home_attack[:, 4] - m.away_defence[:, 9],
                               rtol=1e-12)
    np.testing.assert_allclose(np.log(la1), m.attack[:, 9] - m.defence[:, 4] + m.away_attack[:, 9] - m.home_defence[:, 4],
                               rtol=1e-12)
    # hosts in the tournament: the host slot is the home side of its knockout ties
    inp = m._tournament_inputs(["t01", "t02"], None, 2, 0, None, None, ["t02"], (3, 1, 0), 10, None)
    np.testing.assert_array_equal(inp["host"], [0, 1])


@pytest.mark.parametrize("fmt", ["world_cup_48", "euro_24", "knockout_64"])
def test_restatement_invariants(fmt):
    m = hand_posterior(S=16)
    kw = getattr(R, fmt)(list(m.teams))
    N = 300
    inp = m._tournament_inputs(kw["knockout"], kw.get("groups"), kw.get("advance", 2), kw.get("best_of_rest", 0), None,
                               None, None, (3, 1, 0), N, None)
    out = R.simulate_tournament(R.model_tables(m), inp, _prng_key(11))
    Rr = inp["rounds"]
    stage = out["stage"].astype(np.int64)
    for r in range(Rr + 1):
        np.testing.assert_array_equal((stage >= r + 1).sum(axis=1), 2 ** (Rr - r))
    assert out["stage_counts"].sum() == N * len(inp["teams"])
    if inp["group"] is not None:
        pc = out["position_counts"]
        for g in range(len(inp["group_names"])):
            rows = pc[inp["group"] == g]
            np.testing.assert_array_equal(rows[:, :rows.shape[0]].sum(axis=0), N)
            assert not rows[:, rows.shape[0]:].any()
    assert out["flagged"].mean() < 0.01


def test_knockout_rule_is_the_conditioned_scoreline_distribution():
    # a 2-team bracket: the winner frequency is the mean over draws of hw_s / (hw_s + aw_s)
    m = hand_posterior(S=5, seed=4)
    m.corr_coef = np.array([-0.1, 0.0, 0.08, 0.05, -0.02])
    N = 200_000
    inp = m._tournament_inputs(["t03", "t08"], None, 2, 0, None, None, ["t08"], (3, 1, 0), N, None)
    out = R.simulate_tournament(R.model_tables(m), inp, _prng_key(17))
    wins = int((out["stage"][:, 0] == 2).sum())
    G = 40
    x, y = np.meshgrid(np.arange(G + 1), np.arange(G + 1), indexing="ij")
    # t08 hosts: it is the home side at its venue
    h, a = 8, 3
    p = []
    for s in range(5):
        lh = np.exp(m.attack[s, h] - m.defence[s, a] + (m.home_attack[s, h] - m.away_defence[s, a]))
        la = np.exp(m.attack[s, a] - m.defence[s, h] + (m.away_attack[s, a] - m.home_defence[s, h]))
        rho = m.corr_coef[s]
        tau = np.ones_like(x, dtype=float)
        tau[0, 0], tau[0, 1], tau[1, 0], tau[1, 1] = 1 - lh * la * rho, 1 + lh * rho, 1 + la * rho, 1 - rho
        grid = np.maximum(tau, 0.0) * poisson.pmf(x, lh) * poisson.pmf(y, la)
        hw, aw = np.tril(grid, -1).sum(), np.triu(grid, 1).sum()
        p.append(aw / (hw + aw))      # t03 (slot 0) is the away side
    p = float(np.mean(p))
    assert abs(wins - N * p) < 5 * np.sqrt(N * p * (1 - p)), (wins / N, p)
