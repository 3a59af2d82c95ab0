"""simulate_season on the device (csrc/dc_season.hip.h) against the numpy restatement
(tests/season_ref.py), against the separately tested grid kernel, and on the property that per-fixture
sampling cannot give: one posterior draw per simulated season."""
import numpy as np
import pytest

import season_ref as R
from bpl import DixonColesMatchPredictor, ExtendedDixonColesMatchPredictor
from bpl._ffi import BPLHIP_EINVAL, BPLHIP_ESTATE, BplHipError, HipContext
from bpl.base import _prng_key

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _model(cls, attack, defence, home_advantage, corr_coef):
    m = cls()
    T = attack.shape[1]
    m.teams = np.array([f"t{i:02d}" for i in range(T)])
    m._teams_dict = {t: i for i, t in enumerate(m.teams)}
    m.attack, m.defence = np.asarray(attack, float), np.asarray(defence, float)
    m.home_advantage, m.corr_coef = np.asarray(home_advantage, float), np.asarray(corr_coef, float)
    return m


def _round_robin(T):
    h, a = np.nonzero(~np.eye(T, dtype=bool))
    return h.astype(np.uint16), a.astype(np.uint16)


def _rates(m, h, a):
    """[S, fixtures] home and away rates."""
    edge = m.home_advantage[:, None] if m.home_advantage.ndim == 1 else m.home_advantage[:, h]
    return np.exp(m.attack[:, h] - m.defence[:, a] + edge), np.exp(m.attack[:, a] - m.defence[:, h])


def _posterior(kind, T=20, S=64, seed=0):
    rs = np.random.RandomState(seed)
    att, dfn = rs.normal(0, 0.3, (S, T)), rs.normal(0, 0.3, (S, T))
    if kind == "extended":
        return _model(ExtendedDixonColesMatchPredictor, att, dfn, rs.normal(0.25, 0.1, (S, T)), rs.uniform(-0.1, 0.1, S))
    m = _model(DixonColesMatchPredictor, att, dfn, rs.normal(0.25, 0.05, S), rs.uniform(-0.1, 0.1, S))
    h, a = _round_robin(T)
    lh, la = _rates(m, h, a)
    if kind == "rho_bounds":
        # every draw's rho 1e-6 inside its own bound (over the fixtures): lower bound on even draws, upper on odd
        lo = np.max(np.maximum(-1.0 / lh, -1.0 / la), axis=1)
        hi = np.min(np.minimum(1.0 / (lh * la), 1.0), axis=1)
        m.corr_coef = np.where(np.arange(S) % 2 == 0, lo + 1e-6, hi - 1e-6)
    elif kind == "clipped":
        # tau clips for some pairs: rho beyond the bounds in both directions
        m.corr_coef = np.where(np.arange(S) % 2 == 0, 0.9, -1.1)
        rho = m.corr_coef[:, None]
        clipped = (1 - lh * la * rho < 0) | (1 + lh * rho < 0) | (1 + la * rho < 0)
        assert clipped.any() and not clipped.all()
    return m


def _table(m, seed=3):
    rs = np.random.RandomState(seed)
    return {t: (int(rs.randint(0, 60)), int(rs.randint(0, 70)), int(rs.randint(0, 70))) for t in m.teams[::2]}


def _reference(m, seed, home, away, num_simulations, current_table=None, teams=None, points=(3, 1, 0)):
    h, a, table_idx, table, points, n = m._season_inputs(home, away, num_simulations, current_table, teams, points)
    return R.simulate_season(m.attack, m.defence, m.home_advantage, m.corr_coef, h, a, table_idx, table, points, n,
                             _prng_key(seed))


def _self_consistent(res, m, home, away, current_table):
    """The aggregates are the per-simulation outputs' own: counts of positions, integer sums."""
    N, n = res["points"].shape
    counts = np.zeros((n, n), dtype=np.int64)
    np.add.at(counts, (np.broadcast_to(np.arange(n), (N, n)), res["position"].astype(np.int64)), 1)
    np.testing.assert_array_equal(res["position_proba"], counts / N)
    np.testing.assert_array_equal(res["expected_points"], res["points"].astype(np.int64).sum(axis=0) / N)
    _, _, table_idx, table, _, _ = m._season_inputs(home, away, N, current_table, None, (3, 1, 0))
    slot = {int(t): i for i, t in enumerate(table_idx)}
    h, a = m._team_indices(home, away)
    gd = np.tile(table[:, 1] - table[:, 2], (N, 1))
    diff = res["home_goals"].astype(np.int64) - res["away_goals"].astype(np.int64)
    for f in range(len(h)):
        gd[:, slot[int(h[f])]] += diff[:, f]
        gd[:, slot[int(a[f])]] -= diff[:, f]
    np.testing.assert_array_equal(res["expected_goal_difference"], gd.sum(axis=0) / N)


@pytest.mark.parametrize("kind", ["basic", "extended", "rho_bounds", "clipped"])
def test_bit_exact_against_restatement(kind):
    m = _posterior(kind)
    h, a = _round_robin(20)
    table = _table(m)
    N, seed = 1000, 1234
    res = m.simulate_season(h, a, num_simulations=N, random_state=seed, current_table=table,
                            return_tables=True, return_scores=True)
    ref = _reference(m, seed, h, a, N, table)
    assert list(res["teams"]) == list(m.teams)
    keep = ~ref["flagged"]
    assert ref["flagged"].sum() <= 1e-4 * N, ref["flagged"].sum()
    for key in ("home_goals", "away_goals", "points", "position"):
        np.testing.assert_array_equal(res[key][keep], ref[key][keep], err_msg=key)
    if keep.all():
        for key in ("position_proba", "expected_points", "expected_goal_difference"):
            np.testing.assert_array_equal(res[key], ref[key], err_msg=key)
    _self_consistent(res, m, h, a, table)
    assert res["home_goals"].max() < 255 and res["points"].dtype == np.int32 and res["position"].dtype == np.uint8


def test_scoreline_frequencies_match_the_grid_kernel():
    S, T = 200, 6
    rs = np.random.RandomState(5)
    m = _model(DixonColesMatchPredictor, rs.normal(0, 0.3, (S, T)), rs.normal(0, 0.3, (S, T)),
               rs.normal(0.3, 0.05, S), rs.uniform(-0.08, 0.08, S))
    h = np.array([0, 2, 4, 1], dtype=np.uint16)
    a = np.array([1, 3, 5, 0], dtype=np.uint16)
    lh, la = _rates(m, h, a)
    rho = m.corr_coef[:, None]
    assert ((1 - lh * la * rho > 0) & (1 + lh * rho > 0) & (1 + la * rho > 0)).all()   # tau never clips: Z = 1
    N = 200_000
    res = m.simulate_season(h, a, num_simulations=N, random_state=99, return_scores=True)
    G = 15
    grid = m.predict_score_grid_proba(h, a, max_goals=G)[0]
    checked = 0
    for f in range(len(h)):
        x, y = res["home_goals"][:, f].astype(np.int64), res["away_goals"][:, f].astype(np.int64)
        inside = (x <= G) & (y <= G)
        counts = np.bincount(x[inside] * (G + 1) + y[inside], minlength=(G + 1) ** 2).reshape(G + 1, G + 1)
        p = grid[f]
        cells = N * p >= 20
        bound = 5 * np.sqrt(N * p * (1 - p)) + 1
        bad = cells & (np.abs(counts - N * p) > bound)
        assert not bad.any(), (f, np.argwhere(bad), counts[bad], (N * p)[bad])
        checked += cells.sum()
    assert checked > 100


def test_one_posterior_draw_per_season():
    # S = 2: team 0 is by far the strongest in draw 0 and the weakest in draw 1
    S, T = 2, 8
    rs = np.random.RandomState(11)
    att, dfn = rs.normal(0, 0.1, (S, T)), rs.normal(0, 0.1, (S, T))
    att[0, 0], dfn[0, 0], att[1, 0], dfn[1, 0] = 1.5, 1.5, -1.5, -1.5
    m = _model(DixonColesMatchPredictor, att, dfn, np.full(S, 0.2), np.zeros(S))
    h, a = _round_robin(T)
    N = 20_000
    res = m.simulate_season(h, a, num_simulations=N, random_state=7)
    bound = 5 * np.sqrt(0.25 / N)
    assert abs(res["position_proba"][0, 0] - 0.5) < bound
    assert abs(res["position_proba"][0, T - 1] - 0.5) < bound
    assert res["position_proba"][0, 0] + res["position_proba"][0, T - 1] > 0.999


def test_invariants_and_determinism():
    m = _posterior("extended", seed=2)
    h, a = _round_robin(20)
    kw = dict(num_simulations=3000, current_table=_table(m, 4), return_tables=True, return_scores=True)
    r1 = m.simulate_season(h, a, random_state=42, **kw)
    r2 = m.simulate_season(h, a, random_state=42, **kw)
    r3 = m.simulate_season(h, a, random_state=43, **kw)
    P = r1["position_proba"]
    np.testing.assert_allclose(P.sum(axis=0), 1.0, atol=1e-12)
    np.testing.assert_allclose(P.sum(axis=1), 1.0, atol=1e-12)
    np.testing.assert_array_equal(r1["expected_points"], r1["points"].astype(np.int64).sum(axis=0) / 3000)
    for key in r1:
        np.testing.assert_array_equal(r1[key], r2[key], err_msg=key)
    assert not np.array_equal(r1["home_goals"], r3["home_goals"])
    assert not np.array_equal(r1["position_proba"], r3["position_proba"])
    # the optional outputs change nothing else
    r4 = m.simulate_season(h, a, random_state=42, num_simulations=3000, current_table=kw["current_table"])
    assert set(r4) == {"teams", "position_proba", "expected_points", "expected_goal_difference"}
    for key in r4:
        np.testing.assert_array_equal(r1[key], r4[key], err_msg=key)


def test_zero_fixtures():
    m = _posterior("basic", T=6, S=4)
    table = {"t00": (10, 5, 5), "t01": (30, 1, 0), "t02": (20, 9, 9), "t03": (5, 0, 3)}
    res = m.simulate_season([], [], num_simulations=500, random_state=1, current_table=table)
    assert list(res["teams"]) == ["t00", "t01", "t02", "t03"]
    np.testing.assert_array_equal(res["position_proba"], np.eye(4)[[2, 0, 1, 3]])
    np.testing.assert_array_equal(res["expected_points"], [10, 30, 20, 5])
    np.testing.assert_array_equal(res["expected_goal_difference"], [0, 1, 0, -3])
    # an exact tie (points, GD, GF) splits on the random tie-break
    N = 10_000
    tie = {"t01": (12, 4, 2), "t04": (12, 4, 2)}
    res = m.simulate_season([], [], num_simulations=N, random_state=2, current_table=tie)
    assert abs(res["position_proba"][0, 0] - 0.5) < 5 * np.sqrt(0.25 / N)
    np.testing.assert_allclose(res["position_proba"].sum(axis=0), 1.0)


def test_context_state_and_argument_errors():
    ctx = HipContext(0)
    try:
        args = ([0], [1], [0, 1], np.zeros((2, 3)), (3, 1, 0), 10, (0, 1))
        with pytest.raises(BplHipError) as e:
            ctx.simulate_season(*args)
        assert e.value.code == BPLHIP_ESTATE
        S, T = 4, 3
        tabs = [np.zeros((S, T)) for _ in range(6)]
        ctx.predict_set_posterior_venue(*tabs, np.zeros(S))
        with pytest.raises(BplHipError) as e:
            ctx.simulate_season(*args)
        assert e.value.code == BPLHIP_ESTATE
        ctx.predict_set_posterior(np.zeros((S, T)), np.zeros((S, T)), np.zeros(S), np.zeros(S))
        for bad in (([0], [0], [0, 1]), ([0], [2], [0, 1]), ([0], [1], [0, 5]), ([0], [1], [0, 0])):
            with pytest.raises(BplHipError) as e:
                ctx.simulate_season(*bad, np.zeros((len(bad[2]), 3)), (3, 1, 0), 10, (0, 1))
            assert e.value.code == BPLHIP_EINVAL
        for table, points, n in ((-np.ones((2, 3)), (3, 1, 0), 10), (np.zeros((2, 3)), (3, -1, 0), 10),
                                 (np.zeros((2, 3)), (3, 1, 0), 0), (np.zeros((2, 3)), (3, 1, 0), 2 ** 31)):
            with pytest.raises(BplHipError) as e:
                ctx.simulate_season([0], [1], [0, 1], table, points, n, (0, 1))
            assert e.value.code == BPLHIP_EINVAL
        out = ctx.simulate_season([0], [1], [0, 1], np.zeros((2, 3)), (3, 1, 0), 10, (0, 1))
        assert out["counts"].sum() == 20
    finally:
        ctx.close()


def test_large_run():
    m = _posterior("basic", S=1000, seed=9)
    h, a = _round_robin(20)
    N, seed, K = 100_000, 31337, 2000
    res = m.simulate_season(h, a, num_simulations=N, random_state=seed, return_tables=True, return_scores=True)
    assert res["points"].shape == (N, 20) and res["home_goals"].shape == (N, 380)
    np.testing.assert_allclose(res["position_proba"].sum(axis=1), 1.0, atol=1e-12)
    ref = _reference(m, seed, h, a, K)
    keep = ~ref["flagged"]
    assert ref["flagged"].sum() <= 1e-4 * K
    for key in ("home_goals", "away_goals", "points", "position"):
        np.testing.assert_array_equal(res[key][:K][keep], ref[key][keep], err_msg=key)
