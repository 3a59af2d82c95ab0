"""simulate_season(..., playoffs=...) without a GPU: every argument check (all made on the host before the device
is touched), the resolution of positions, guests and byes, the invariants of the numpy restatement
(tests/playoff_ref.py), and the restatement's rule against the ladder's probability from the posterior draws'
scoreline grids -- with a home advantage large enough that the wrong orientation would be caught."""
import numpy as np
import pytest

import playoff_ref as PR
from bpl import DixonColesMatchPredictor, ExtendedDixonColesMatchPredictor
from bpl.base import PLAYOFF_BYE, PLAYOFF_GUEST, _prng_key, playoff_inputs, playoff_result
from test_knockout_host import _difference, _grid


def hand_posterior(cls=DixonColesMatchPredictor, T=10, S=8, seed=1, home=0.2):
    rs = np.random.RandomState(seed)
    m = cls()
    m.teams = np.array([f"t{i:02d}" for i in range(T)])
    m._teams_dict = {t: i for i, t in enumerate(m.teams)}
    m.attack = rs.normal(0, 0.2, (S, T))
    m.defence = rs.normal(0, 0.2, (S, T))
    m.home_advantage = rs.normal(home, 0.05, S if cls is DixonColesMatchPredictor else (S, T))
    m.corr_coef = rs.uniform(-0.05, 0.05, S)
    return m


def _fixtures(teams):
    """One round robin among `teams` (names)."""
    return ([h for h in teams for a in teams if h != a], [a for h in teams for a in teams if h != a])


def _raises(m, playoffs, teams=None):
    teams = list(m.teams[:6]) if teams is None else teams
    home, away = _fixtures(teams)
    with pytest.raises(ValueError):
        m.simulate_season(home, away, num_simulations=10, random_state=1, playoffs=playoffs)
    assert m._predict_ctx is None   # no device context was ever made


def test_argument_checks_run_on_the_host():
    m = hand_posterior()
    ok = [3, 0, 2, 1]                                     # two rounds on a table of six
    for bad in ("bracket", [3, 0], ("bracket", ok), 7, True):
        _raises(m, bad)
    _raises(m, {})                                        # "bracket" is required
    _raises(m, {"legs": 2})
    _raises(m, {"bracket": ok, "leg": 2})                 # unknown keys
    _raises(m, {"bracket": ok, "knockout_rule": "redraw"})
    # the bracket: 2**R entries, 1 <= R <= 6
    for br in ([], [0], [0, 1, 2], list(range(6)), 5, None, "0123", {0: 1}):
        _raises(m, {"bracket": br})
    big = hand_posterior(T=64)
    _raises(big, {"bracket": list(range(64)) + [None] * 64}, teams=list(big.teams))
    # entries: positions inside the table, once each
    for br in ([0, 6], [0, -7], [0, 0], [2, -4], [0, 1.0], [0, True], [0, (1,)], [0, 1, 2, 2], [0.0, 1]):
        _raises(m, {"bracket": br})
    # guests: known to the model, not a row of the table, once each
    for br in ([0, "nope"], [0, "t03"], ["t08", "t08"], [0, 1, "t08", "t08"], [0, b"t08"]):
        _raises(m, {"bracket": br})
    # byes: never two in a pair
    for br in ([None, None], [0, 1, None, None], [None, None, 0, 1]):
        _raises(m, {"bracket": br})
    # table rows plus guests number at most 64
    full = hand_posterior(T=66)
    _raises(full, {"bracket": [0, "t64", 1, "t65"]}, teams=list(full.teams[:63]))
    # legs
    for legs in (0, 3, True, 1.0, "2", [1], [1, 2, 1], [1, 3], [1, 2.0], [True, 1], "12", {1: 2}, [[1], [2]]):
        _raises(m, {"bracket": ok, "legs": legs})
    # venue
    for venue in ("home", None, 1, ["seed"], ["seed", "neutral", "seed"], ["seed", "away"], ["seed", 1], {"seed": 1},
                  "sn", [["seed"], ["seed"]]):
        _raises(m, {"bracket": ok, "venue": venue})
    # extra_time_scale in (0, 1]
    for c in (0, 0.0, -0.1, 1.0000001, 2, np.nan, np.inf, "0.3", None, True, [0.3]):
        _raises(m, {"bracket": ok, "extra_time_scale": c})
    # shootout: a dict of table rows or guests to finite strengths of at most 20
    for so in ([("t00", 1.0)], "t00", {"nope": 1.0}, {"t08": 1.0}, {"t00": np.nan}, {"t00": np.inf}, {"t00": 20.5},
               {"t00": -21}, {"t00": "1"}, {"t00": None}, {"t00": True}, {0: 1.0}):
        _raises(m, {"bracket": ok, "shootout": so})
    for ag in (1, 0, "yes", None):
        _raises(m, {"bracket": ok, "away_goals": ag})
    # the per-team home-advantage class passes them on to the same checks
    e = hand_posterior(ExtendedDixonColesMatchPredictor)
    _raises(e, {"bracket": ok, "legs": [2, 2, 1]})
    _raises(e, {"bracket": [0, "t01"]})
    # and the other arguments keep their checks with play-offs given
    with pytest.raises(ValueError):
        m.simulate_season(["t00"], ["t00"], playoffs={"bracket": [0, 1]})
    with pytest.raises(ValueError):
        m.simulate_season(["t00"], ["t01"], tiebreak="alphabet", playoffs={"bracket": [0, 1]})
    with pytest.raises(TypeError):
        m.match_leverage(["t00"], ["t01"], playoffs={"bracket": [0, 1]})   # out of scope
    assert m._predict_ctx is None


def test_codes_are_resolved():
    m = hand_posterior()
    table_idx = np.array([0, 2, 3, 5, 6, 7])
    po = playoff_inputs({"bracket": [3, 0, "t08", -1, None, 1, "t01", None]}, table_idx, m._teams_dict)
    G, B = PLAYOFF_GUEST, PLAYOFF_BYE
    np.testing.assert_array_equal(po["bracket"], [3, 0, G | 0, 5, B, 1, G | 1, B])
    assert po["bracket"].dtype == np.uint16 and po["rounds"] == 3
    np.testing.assert_array_equal(po["guests"], [8, 1])     # bracket order, not team order
    assert po["guest_names"] == ["t08", "t01"]
    np.testing.assert_array_equal(po["legs"], [1, 1, 1])
    assert po["legs_mask"] == 0 and po["neutral_mask"] == 0 and po["venue"] == ["seed"] * 3
    assert po["extra_time_scale"] == 1 / 3 and po["away_goals"] is False
    np.testing.assert_array_equal(po["strength"], np.zeros(8))
    po = playoff_inputs({"bracket": [3, 0, "t08", -1, None, 1, "t01", None], "legs": (2, 1, 2),
                         "venue": ("neutral", "neutral", "seed"), "extra_time_scale": 1, "away_goals": True,
                         "shootout": {"t08": -20, "t05": 0.25, "t01": 3}}, table_idx, m._teams_dict)
    assert po["legs_mask"] == 0b101 and po["neutral_mask"] == 0b011 and po["extra_time_scale"] == 1.0
    assert po["away_goals"] is True
    np.testing.assert_array_equal(po["strength"], [0, 0, 0, 0.25, 0, 0, -20, 3])   # slots: table rows, then guests
    assert playoff_inputs({"bracket": [0, 1], "legs": 2, "venue": "neutral"}, table_idx, m._teams_dict)["legs_mask"] == 1
    # positions -> slots in the restatement: the slot AT a position, guests at n + i, byes nowhere
    position = np.array([[2, 0, 5, 1, 4, 3], [0, 1, 2, 3, 4, 5]])
    br = PR.resolve(po["bracket"], position, 6)
    np.testing.assert_array_equal(br, [[5, 1, 6, 2, -1, 3, 7, -1], [3, 0, 6, 5, -1, 1, 7, -1]])
    # playoff_result: shares of the matches played; a round with nothing but byes gives zeros, not NaN
    raw = {"stage_counts": np.array([[0, 4, 6], [0, 6, 4], [10, 0, 0]], dtype=np.uint64),
           "decided_counts": np.array([[5, 0, 3, 2]], dtype=np.uint64)}
    res = playoff_result({"rounds": 1}, raw, 10)
    np.testing.assert_array_equal(res["playoff_round_proba"], [[1.0, 0.6], [1.0, 0.4], [0.0, 0.0]])
    np.testing.assert_array_equal(res["playoff_decided_proba"], [[0.5, 0, 0.3, 0.2]])
    raw["decided_counts"][:] = 0
    np.testing.assert_array_equal(playoff_result({"rounds": 1}, raw, 10)["playoff_decided_proba"], np.zeros((1, 4)))


FORMATS = {
    "championship": (10, {"bracket": [5, 2, 4, 3], "legs": (2, 1), "venue": ("seed", "neutral")}),
    "relegation": (8, {"bracket": [-3, "t09"], "legs": 2, "away_goals": True}),
    "byes": (10, {"bracket": [0, None, 4, 5, 1, None, 3, 6], "legs": (2, 2, 1), "away_goals": True,
                  "shootout": {"t02": 1.0, "t07": -1.0}}),
    "guests": (6, {"bracket": [None, "t07", 0, "t06", "t09", 1, 2, "t08"], "venue": "neutral"}),
}


@pytest.mark.parametrize("cls", [DixonColesMatchPredictor, ExtendedDixonColesMatchPredictor])
@pytest.mark.parametrize("tiebreak", ["overall", "head_to_head"])
@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_restatement_invariants(fmt, tiebreak, cls):
    n, playoffs = FORMATS[fmt]
    m = hand_posterior(cls)
    teams = list(m.teams[:n])
    home, away = _fixtures(teams[:5])                        # the others keep their zero rows: ties on points
    N = 300
    inputs = m._season_inputs(home, away, N, None, teams, (3, 1, 0))
    po = playoff_inputs(playoffs, inputs[2], m._teams_dict)
    out = PR.simulate_season(m, inputs, po, _prng_key(11), head_to_head=tiebreak == "head_to_head")
    R, nb = po["rounds"], len(po["bracket"])
    nt = n + len(po["guests"])
    stage, decided = out["playoff_stage"].astype(np.int64), out["playoff_decided"]
    assert stage.shape == (N, nt) and decided.shape == (N, nb - 1)
    entries = int((po["bracket"] != PLAYOFF_BYE).sum())
    # each round's entrants are the previous round's winners, one per match (a bye's team is its match's winner)
    np.testing.assert_array_equal((stage >= 1).sum(axis=1), entries)
    for r in range(R):
        np.testing.assert_array_equal((stage >= r + 2).sum(axis=1), nb >> (r + 1))
    # a table row is in the bracket exactly when its position is listed; a listed guest always
    listed = sorted(int(c) for c in po["bracket"] if c < PLAYOFF_GUEST)
    np.testing.assert_array_equal(stage[:, :n] >= 1, np.isin(out["position"], listed))
    assert (stage[:, n:] >= 1).all()
    res = playoff_result(po, out, N)
    assert res["playoff_round_proba"].shape == (nt, R + 1) and res["playoff_decided_proba"].shape == (R, 4)
    assert abs(res["playoff_round_proba"][:, 0].sum() - entries) < 1e-9
    assert abs(res["playoff_round_proba"][:, R].sum() - 1.0) < 1e-9
    # the counts are the records' bincount; byes are 255 and only where the bracket has them
    np.testing.assert_array_equal(out["stage_counts"], np.stack([np.bincount(stage[:, i], minlength=R + 2) for i in range(nt)]))
    k0 = 0
    for r in range(R):
        M = nb >> (r + 1)
        cols = decided[:, k0:k0 + M]
        np.testing.assert_array_equal(out["decided_counts"][r], np.bincount(cols.ravel(), minlength=256)[:4])
        if r == 0:
            bye = (po["bracket"].reshape(-1, 2) == PLAYOFF_BYE).any(axis=1)
            np.testing.assert_array_equal(cols == PR.DECIDED_BYE, np.broadcast_to(bye, (N, M)))
        else:
            assert not (cols == PR.DECIDED_BYE).any()
        if not (po["legs"][r] == 2 and po["away_goals"]):
            assert not (cols == PR.AWAY_GOALS).any()
        k0 += M
    assert out["flagged"].mean() < 0.01


def _ladder_probability(m, p, q, mode, wrong=False):
    """P(the worse seed p goes through against the better seed q), the mean over the draws of the ladder's
    probability from 41 x 41 grids.  mode: "seed", "neutral" or "two".  wrong: the mistaken orientation -- the
    worse seed at home ("seed": p hosts; "two": leg 2 and extra time at p's ground), or the home advantage
    applied under "neutral"."""
    shoot = 1.0 / (1.0 + np.exp(-0.4))                       # strength 0.4 for p, 0 for q
    out = []
    for s in range(m.attack.shape[0]):
        rho, ha = m.corr_coef[s], m.home_advantage[s]

        def rates(h, a, on):
            return (np.exp(m.attack[s, h] - m.defence[s, a] + (ha if on else 0.0)), np.exp(m.attack[s, a] - m.defence[s, h]))

        def diff(h, a, on, scale=1.0):
            """p's goals minus q's over one leg with h at home"""
            lh, la = rates(h, a, on)
            return _difference(_grid(lh * scale, la * scale, rho), +1 if h == p else -1)

        if mode == "neutral":
            D, E = diff(p, q, wrong), diff(p, q, wrong, 1 / 3)
        elif mode == "seed":
            host, guest = (p, q) if wrong else (q, p)
            D, E = diff(host, guest, True), diff(host, guest, True, 1 / 3)
        else:
            first, second = (q, p) if wrong else (p, q)
            D = np.convolve(diff(first, second, True), diff(second, first, True))
            E = diff(second, first, True, 1 / 3)
        c, e = D.size // 2, E.size // 2
        out.append(D[c + 1:].sum() + D[c] * (E[e + 1:].sum() + E[e] * shoot))
    return float(np.mean(out))


@pytest.mark.parametrize("mode", ["seed", "neutral", "two"])
def test_rule_is_the_stated_distribution(mode):
    # no fixtures left and distinct points: 1st and 4th are known.  Bracket [3, 0]: t02 (4th, p) against t04 (1st, q).
    # Home advantage 0.6: hosting is worth far more than the 5 sigma of 2e5 simulations, in every mode (printed)
    m = hand_posterior(T=6, S=5, seed=4, home=0.6)
    m.corr_coef = np.array([-0.1, 0.0, 0.08, 0.05, -0.02])
    table = {"t04": (30, 0, 0), "t00": (28, 0, 0), "t05": (25, 0, 0), "t02": (21, 0, 0), "t01": (20, 0, 0),
             "t03": (9, 0, 0)}
    N = 200_000
    playoffs = {"bracket": [3, 0], "shootout": {"t02": 0.4}, "legs": 2 if mode == "two" else 1,
                "venue": "neutral" if mode == "neutral" else "seed"}
    inputs = m._season_inputs([], [], N, table, None, (3, 1, 0))
    po = playoff_inputs(playoffs, inputs[2], m._teams_dict)
    out = PR.simulate_season(m, inputs, po, _prng_key(17))
    assert not out["flagged"].any(), out["flagged"].sum()
    np.testing.assert_array_equal(out["position"][0], [1, 4, 3, 5, 0, 2])
    stage = out["playoff_stage"]
    assert (stage[:, [0, 1, 3, 5]] == 0).all() and (stage[:, [2, 4]] >= 1).all()
    wins = int((stage[:, 2] == 2).sum())
    assert wins + int((stage[:, 4] == 2).sum()) == N
    p = _ladder_probability(m, 2, 4, mode)
    p_wrong = _ladder_probability(m, 2, 4, mode, wrong=True)
    sigma = (wins - N * p) / np.sqrt(N * p * (1 - p))
    sigma_wrong = (wins - N * p_wrong) / np.sqrt(N * p_wrong * (1 - p_wrong))
    print(f"{mode}: {wins / N:.5f} against {p:.5f}, {sigma:+.2f} sigma; the wrong orientation {p_wrong:.5f}, "
          f"{sigma_wrong:+.2f} sigma")
    assert abs(sigma) < 5, (wins / N, p)
    assert abs(sigma_wrong) > 5, (wins / N, p_wrong)
    res = playoff_result(po, out, N)
    np.testing.assert_array_equal(res["playoff_round_proba"][:, 0], [0, 0, 1, 0, 1, 0])
    assert res["playoff_round_proba"][2, 1] == wins / N
    np.testing.assert_array_equal(out["decided_counts"][0], np.bincount(out["playoff_decided"][:, 0], minlength=4))
    assert out["decided_counts"][0, PR.AWAY_GOALS] == 0 and (out["decided_counts"][0, [0, 2, 3]] > 0).all()
