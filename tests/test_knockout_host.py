"""simulate_tournament(knockout_rule="extra_time") without a GPU: the new argument checks (all made on the host
before the device is touched), the restatement's rule (tests/knockout_ref.py) against the posterior draws'
scoreline grids, and the restatement's invariants."""
import numpy as np
import pytest
from scipy.stats import poisson

import knockout_ref as K
import tournament_ref as R
from bpl import NeutralDixonColesMatchPredictorWC
from bpl.base import _prng_key
from bpl.neutral_dixon_coles import tournament_result
from test_tournament_host import conf_of, hand_posterior

ET = dict(knockout_rule="extra_time")


def _raises(m, *args, **kwargs):
    with pytest.raises(ValueError):
        m.simulate_tournament(*args, **kwargs)
    assert m._predict_ctx is None   # no device context was ever made


def test_rule_argument_checks_run_on_the_host():
    m = hand_posterior()
    t = list(m.teams)
    ko = t[:4]                                                         # two rounds
    _raises(m, ko, knockout_rule="golden_goal")
    _raises(m, ko, knockout_rule=None)
    _raises(m, ko, knockout_rule=1)
    # non-default values need the rule, given explicitly or not
    for kw in (dict(legs=1), dict(legs=2), dict(legs=[1, 1]), dict(extra_time_scale=0.5), dict(shootout={}),
               dict(shootout={"t00": 1.0}), dict(away_goals=True)):
        _raises(m, ko, **kw)
        _raises(m, ko, knockout_rule="redraw", **kw)
    # legs
    for legs in (0, 3, True, 1.0, "2", [1], [1, 2, 1], [1, 3], [1, 2.0], [True, 1], "12", {1: 2}, [[1], [2]]):
        _raises(m, ko, legs=legs, **ET)
    # extra_time_scale in (0, 1]
    for c in (0, 0.0, -0.1, 1.0000001, 2, np.nan, np.inf, "0.3", None, True, [0.3]):
        _raises(m, ko, extra_time_scale=c, **ET)
    # shootout: a dict of playing teams to finite strengths of at most 20
    for so in ([("t00", 1.0)], "t00", {"nope": 1.0}, {"t60": 1.0}, {"t00": np.nan}, {"t00": np.inf}, {"t00": 20.5},
               {"t00": -21}, {"t00": "1"}, {"t00": None}, {"t00": True}, {0: 1.0}):
        _raises(m, ko, shootout=so, **ET)
    for ag in (1, 0, "yes", None):
        _raises(m, ko, away_goals=ag, **ET)
    # the World-Cup class passes them on to the same checks
    w = hand_posterior(NeutralDixonColesMatchPredictorWC)
    _raises(w, ko, team_conf=conf_of(w), legs=2)
    _raises(w, ko, team_conf=conf_of(w), legs=[2, 2, 1], **ET)
    _raises(w, ko, team_conf=conf_of(w), shootout={"t00": 99.0}, **ET)


def test_rule_inputs_are_resolved():
    m = hand_posterior()
    ko = ["t10", "t03", "t07", "t01", "t20", "t21", "t22", "t23"]
    args = (ko, None, 2, 0, None, None, ["t07"], (3, 1, 0), 10, None)
    inp = m._tournament_inputs(*args)
    assert inp["knockout_rule"] == "redraw" and "legs" not in inp and "strength" not in inp
    inp = m._tournament_inputs(*args, **ET)
    np.testing.assert_array_equal(inp["legs"], [1, 1, 1])
    assert inp["legs_mask"] == 0 and inp["extra_time_scale"] == 1 / 3 and inp["away_goals"] is False
    np.testing.assert_array_equal(inp["strength"], np.zeros(8))
    inp = m._tournament_inputs(*args, knockout_rule="extra_time", legs=(2, 1, 2), extra_time_scale=1,
                               shootout={"t07": -20, "t23": 0.25}, away_goals=True)
    np.testing.assert_array_equal(inp["legs"], [2, 1, 2])
    assert inp["legs_mask"] == 0b101 and inp["extra_time_scale"] == 1.0 and inp["away_goals"] is True
    np.testing.assert_array_equal(inp["strength"], [0, 0, -20, 0, 0, 0, 0, 0.25])
    assert m._tournament_inputs(*args, knockout_rule="extra_time", legs=2)["legs_mask"] == 0b111
    # tournament_result: round r has 2^(R - 1 - r) matches per simulation
    raw = {"stage_counts": np.zeros((8, 5), dtype=np.uint64),
           "decided_counts": np.array([[20, 0, 12, 8], [10, 2, 4, 4], [10, 0, 0, 0]], dtype=np.uint64)}
    np.testing.assert_array_equal(tournament_result(inp, raw)["decided_proba"],
                                  [[0.5, 0, 0.3, 0.2], [0.5, 0.1, 0.2, 0.2], [1, 0, 0, 0]])


def _grid(lh, la, rho, G=40):
    """The normalised max(tau, 0) Pois Pois grid [G + 1, G + 1] (home goals, away goals)."""
    x, y = np.meshgrid(np.arange(G + 1), np.arange(G + 1), indexing="ij")
    tau = np.ones_like(x, dtype=float)
    tau[0, 0], tau[0, 1], tau[1, 0], tau[1, 1] = 1 - lh * la * rho, 1 + lh * rho, 1 + la * rho, 1 - rho
    g = np.maximum(tau, 0.0) * poisson.pmf(x, lh) * poisson.pmf(y, la)
    return g / g.sum()


def _difference(grid, sign):
    """The distribution of sign * (home goals - away goals) over -G..G, as an array [2G + 1] (index G = level)."""
    G = grid.shape[0] - 1
    d = np.array([np.trace(grid, offset=-k) for k in range(-G, G + 1)])   # home - away = k
    return d if sign > 0 else d[::-1]


@pytest.mark.parametrize("legs", [1, 2])
def test_rule_is_the_stated_distribution(legs):
    # a 2-team bracket: P(t03 through) = mean over draws of P(D > 0) + P(D = 0) (P(E > 0) + P(E = 0) logistic(0.4))
    m = hand_posterior(S=5, seed=4)
    m.corr_coef = np.array([-0.1, 0.0, 0.08, 0.05, -0.02])
    N = 200_000
    inp = m._tournament_inputs(["t03", "t08"], None, 2, 0, None, None, ["t08"], (3, 1, 0), N, None,
                               knockout_rule="extra_time", legs=legs, shootout={"t03": 0.4})
    out = K.simulate_tournament(R.model_tables(m), inp, _prng_key(17))
    assert not out["flagged"].any(), out["flagged"].sum()
    wins = int((out["stage"][:, 0] == 2).sum())

    def on_venue(s, h, a):
        return (np.exp(m.attack[s, h] - m.defence[s, a] + (m.home_attack[s, h] - m.away_defence[s, a])),
                np.exp(m.attack[s, a] - m.defence[s, h] + (m.away_attack[s, a] - m.home_defence[s, h])))

    shoot = 1.0 / (1.0 + np.exp(-0.4))
    p = []
    for s in range(5):
        rho = m.corr_coef[s]
        lh, la = on_venue(s, 8, 3)                      # t08 at home: the host, or leg 2
        D = _difference(_grid(lh, la, rho), -1)         # t03 is the away side
        if legs == 2:
            D = np.convolve(_difference(_grid(*on_venue(s, 3, 8), rho), +1), D)   # leg 1: t03 at home
        E = _difference(_grid(lh / 3, la / 3, rho), -1)
        c, e = D.size // 2, E.size // 2
        p.append(D[c + 1:].sum() + D[c] * (E[e + 1:].sum() + E[e] * shoot))
    p = float(np.mean(p))
    sigma = (wins - N * p) / np.sqrt(N * p * (1 - p))
    print(f"legs={legs}: {wins / N:.5f} against {p:.5f}, {sigma:+.2f} sigma")
    assert abs(sigma) < 5, (wins / N, p)
    # the counts are those of the per-match record
    np.testing.assert_array_equal(out["decided_counts"][0], np.bincount(out["decided"][:, 0], minlength=4))
    assert out["decided_counts"][0, K.AWAY_GOALS] == 0 and (out["decided_counts"][0, [0, 2, 3]] > 0).all()


FORMATS = [("world_cup_48", None), ("euro_24", (1, 2, 2, 1)), ("knockout_64", (2, 2, 2, 2, 2, 1))]


@pytest.mark.parametrize("away_goals", [False, True])
@pytest.mark.parametrize("fmt,legs", FORMATS)
def test_restatement_invariants(fmt, legs, away_goals):
    m = hand_posterior(S=16)
    kw = getattr(R, fmt)(list(m.teams))
    N = 300
    inp = m._tournament_inputs(kw["knockout"], kw.get("groups"), kw.get("advance", 2), kw.get("best_of_rest", 0), None,
                               None, None, (3, 1, 0), N, None, knockout_rule="extra_time", legs=legs,
                               away_goals=away_goals)
    out = K.simulate_tournament(R.model_tables(m), inp, _prng_key(11))
    Rr = inp["rounds"]
    stage = out["stage"].astype(np.int64)
    for r in range(Rr + 1):
        np.testing.assert_array_equal((stage >= r + 1).sum(axis=1), 2 ** (Rr - r))
    assert out["stage_counts"].sum() == N * len(inp["teams"])
    k0 = 0
    for r in range(Rr):
        M = (1 << Rr) >> (r + 1)
        cols = slice(k0, k0 + M)
        dec = out["decided"][:, cols]
        assert out["decided_counts"][r].sum() == N * M
        if inp["legs"][r] == 2 and away_goals:
            # no tie with a level aggregate and different away goals reaches extra time
            split = out["level"][:, cols] & (out["away"][:, cols, 0] != out["away"][:, cols, 1])
            np.testing.assert_array_equal(dec == K.AWAY_GOALS, split)
        else:
            assert not (dec == K.AWAY_GOALS).any()
        np.testing.assert_array_equal(dec == K.NORMAL, ~out["level"][:, cols])
        k0 += M
    want = tournament_result(inp, out)
    np.testing.assert_allclose(want["decided_proba"].sum(axis=1), 1.0, atol=1e-12)
    assert out["flagged"].mean() < 0.01
