"""posterior_predictive_check without a GPU: every argument check runs on the host before any device call,
the statistics and p-values from stubbed per-replication tallies, the summing of per-gameweek device calls,
and the observed statistics of a small data set counted by hand."""
import math

import numpy as np
import pytest

import loglik_ref as LR
import ppc_ref as PR
from bpl.ppc import PPC_MAX_REPLICATIONS, PPC_MAX_SCORE_CELLS, PPC_MAX_TEAMS


class FailCtx:
    """A device context that must never be touched."""

    def __getattr__(self, name):
        raise AssertionError(f"device call {name} before the host checks finished")


class StubCtx:
    """A device context whose `ppc` returns the tallies of fixed replications X, Y [R, n] (columns picked by
    fixture id), counted by tests/ppc_ref.py; records every call."""

    def __init__(self, X, Y):
        self.X, self.Y, self.calls = np.asarray(X), np.asarray(Y), []

    def predict_set_posterior(self, *args, **kwargs):
        pass

    def predict_set_posterior_venue(self, *args, **kwargs):
        pass

    def ppc(self, home_idx, away_idx, home_slot, away_slot, n_slots, max_goals, n_reps, key, fixture_id=None,
            neutral=None, conf=None, return_scores=False):
        f = np.arange(len(home_idx)) if fixture_id is None else np.asarray(fixture_id)
        self.calls.append(f)
        x, y = self.X[:n_reps, f], self.Y[:n_reps, f]
        raw = PR.raw_tallies(x, y, np.asarray(home_slot, np.int64), np.asarray(away_slot, np.int64), n_slots,
                             max_goals)
        out = {k: v.astype(np.int64 if k == "sums" else np.uint32) for k, v in raw.items()}
        if return_scores:
            out["home_goals"], out["away_goals"] = x.astype(np.uint8), y.astype(np.uint8)
        return out


def _raises(m, data, **kwargs):
    m._predict_ctx = FailCtx()
    with pytest.raises(ValueError):
        m.posterior_predictive_check(data, **kwargs)


@pytest.mark.parametrize("kind", LR.KINDS)
def test_argument_checks_run_on_the_host(kind):
    m = LR.hand_model(kind, S=16)
    good = LR.hand_data(m, n=6)
    _raises(m, {k: [] for k in good})
    for r in (0, -1, 2.5, True, np.bool_(True), "10", PPC_MAX_REPLICATIONS + 1):
        _raises(m, good, num_replications=r)
    for g in (0, 16, -3, True, 2.0, None):
        _raises(m, good, max_goals=g)
    for p in ((3, 1), (3, 1, True), (3, 1, -1), (1001, 0, 0), (3.5, 1, 0), "abc", None):
        _raises(m, good, points=p)
    _raises(m, dict(good, home_team=["nope"] + list(good["home_team"][1:])))
    _raises(m, dict(good, away_goals=[256] + list(good["away_goals"][1:])))
    d = dict(good)
    d.pop("away_goals")
    _raises(m, d)
    if kind != "basic" and kind != "extended":
        _raises(m, dict(good, neutral_venue=[2] + list(good["neutral_venue"][1:])))


def test_team_and_size_limits_run_on_the_host():
    m = LR.hand_model("neutral", S=4, T=PPC_MAX_TEAMS + 40)
    _raises(m, LR.hand_data(m, n=3000, seed=2))          # > 1024 teams appear in data
    m = LR.hand_model("basic", S=4, T=2)
    d = LR.hand_data(m, n=1100)
    assert PPC_MAX_REPLICATIONS * 1100 > PPC_MAX_SCORE_CELLS
    _raises(m, d, num_replications=PPC_MAX_REPLICATIONS, return_replications=True)
    m = LR.hand_model("basic", S=4, T=80)
    _raises(m, LR.hand_data(m, n=400), num_replications=PPC_MAX_REPLICATIONS)   # R x k over 2^26


def test_observed_statistics_by_hand():
    m = LR.hand_model("basic", S=4, T=5)
    # teams t00, t01, t03 appear (k = 3); t02 and t04 do not
    d = {"home_team": ["t00", "t01", "t03", "t00", "t03"], "away_team": ["t01", "t03", "t00", "t03", "t01"],
         "home_goals": [2, 0, 1, 9, 0], "away_goals": [1, 0, 1, 0, 3]}
    X = np.tile(np.asarray(d["home_goals"]), (4, 1))
    Y = np.tile(np.asarray(d["away_goals"]), (4, 1))
    m._predict_ctx = StubCtx(X, Y)
    res = m.posterior_predictive_check(d, max_goals=3, points=(3, 1, 0))
    assert list(res["teams"]) == ["t00", "t01", "t03"] and res["n"] == 5 and res["num_replications"] == 4
    sc = np.zeros((4, 4), dtype=np.int64)
    sc[2, 1] = sc[0, 0] = sc[1, 1] = sc[3, 0] = sc[0, 3] = 1    # 9-0 lands in row 3 ("3 or more")
    np.testing.assert_array_equal(res["scoreline"]["observed"], sc)
    np.testing.assert_array_equal(res["outcome"]["observed"], [2, 2, 1])
    assert res["home_goals"]["observed"] == 12 and res["away_goals"]["observed"] == 5
    # x = 2 0 1 9 0: mean 2.4, E x^2 = 86 / 5; y = 1 0 1 0 3: mean 1, E y^2 = 11 / 5; E xy = 3 / 5
    assert abs(res["home_goals_var"]["observed"] - (86 / 5 - 2.4 ** 2)) < 1e-12
    assert abs(res["away_goals_var"]["observed"] - (11 / 5 - 1.0)) < 1e-12
    cov = 3 / 5 - 2.4 * 1.0
    want = cov / math.sqrt((86 / 5 - 2.4 ** 2) * (11 / 5 - 1.0))
    assert abs(res["goals_corr"]["observed"] - want) < 1e-12
    # t00: 2-1 W, 1-1 D (away), 9-0 W -> GF 12, GA 2, 7 pts; t01: 1-2 L, 0-0 D, 3-0 W (away) -> GF 4, GA 2, 4 pts
    # t03: 0-0 D, 1-1 D, 0-9 L (away), 0-3 L -> GF 1, GA 13, 2 pts
    np.testing.assert_array_equal(res["team_goals_for"]["observed"], [12, 4, 1])
    np.testing.assert_array_equal(res["team_goals_against"]["observed"], [2, 2, 13])
    np.testing.assert_array_equal(res["team_points"]["observed"], [7, 4, 2])
    # every replication equals the data: both p-values are 1
    for nm in ("scoreline", "goals_corr", "team_points"):
        assert np.all(res[nm]["p_upper"] == 1.0) and np.all(res[nm]["p_lower"] == 1.0)


@pytest.mark.parametrize("kind", ["basic", "wc"])
def test_statistics_and_p_values_from_stubbed_tallies(kind):
    m = LR.hand_model(kind, S=8, T=6)
    d = LR.hand_data(m, n=30, seed=3)
    rs = np.random.RandomState(5)
    R = 40
    X, Y = rs.poisson(1.4, (R, 30)), rs.poisson(1.1, (R, 30))
    X[3] = 2                      # a replication with zero home variance: corr 0
    Y[7, :5] = 200                # large goals
    m._predict_ctx = stub = StubCtx(X, Y)
    pts = (2, 1, 0)
    res = m.posterior_predictive_check(d, num_replications=R, max_goals=5, points=pts, return_replications=True)
    assert len(stub.calls) == 1
    idx, hs, as_ = PR.slots(m, d)
    want = PR.stats(X, Y, hs, as_, idx.size, 5, pts)
    obs = PR.stats(d["home_goals"], d["away_goals"], hs, as_, idx.size, 5, pts)
    for nm, w in want.items():
        got = res[nm]["replicated"]
        assert got.shape == w.shape, nm
        if nm in ("home_goals_var", "away_goals_var", "goals_corr"):
            np.testing.assert_allclose(got, w, rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(res[nm]["observed"], obs[nm][0], rtol=1e-12, atol=1e-12)
        else:
            np.testing.assert_array_equal(got, w)
            np.testing.assert_array_equal(res[nm]["observed"], obs[nm][0])
        o = res[nm]["observed"]
        np.testing.assert_array_equal(res[nm]["p_upper"], np.mean(got >= o, axis=0))
        np.testing.assert_array_equal(res[nm]["p_lower"], np.mean(got <= o, axis=0))
        assert np.all(res[nm]["p_upper"] + res[nm]["p_lower"] >= 1.0)
    assert res["goals_corr"]["replicated"][3] == 0.0
    np.testing.assert_array_equal(res["replications"]["home_goals"], X)
    np.testing.assert_array_equal(res["replications"]["away_goals"], Y)
    assert res["replications"]["home_goals"].dtype == np.uint8


def test_dynamic_groups_are_summed():
    m = LR.hand_model("dynamic", S=8, T=6, G=4)
    d = LR.hand_data(m, n=50, seed=6)
    assert len(np.unique(d["gameweek"])) == 4
    rs = np.random.RandomState(7)
    X, Y = rs.poisson(1.3, (16, 50)), rs.poisson(1.0, (16, 50))
    m._predict_ctx = stub = StubCtx(X, Y)
    res = m.posterior_predictive_check(d, num_replications=16, max_goals=4, return_replications=True)
    assert len(stub.calls) == 4
    ids = np.sort(np.concatenate(stub.calls))
    np.testing.assert_array_equal(ids, np.arange(50))            # disjoint fixture ids covering the data
    idx, hs, as_ = PR.slots(m, d)
    want = PR.stats(X, Y, hs, as_, idx.size, 4)
    for nm in ("scoreline", "outcome", "home_goals", "team_goals_for", "team_goals_against", "team_points"):
        np.testing.assert_array_equal(res[nm]["replicated"], want[nm])
    np.testing.assert_allclose(res["goals_corr"]["replicated"], want["goals_corr"], rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(res["replications"]["home_goals"], X)
    np.testing.assert_array_equal(res["replications"]["away_goals"], Y)
