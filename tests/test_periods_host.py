"""predict_periods without a GPU (bpl/periods.py): every builder's weights against a brute-force quadruple loop
over the cells, the partitions the builders must form, `first_goal` of bpl/markets.py, result keys, shapes and
dtypes for each class through a stand-in context whose `period_summary` is the numpy restatement
(tests/periods_ref.py), the restatement's own identities, and every argument check, made on the host before a
device context is touched."""
import itertools

import numpy as np
import pytest

import loglik_ref as LR
import markets_ref as MR
import periods_ref as PR
import scores_ref as SR
from bpl import markets as MK
from bpl import periods as PD
from fake_ctx import FakePredictCtx

GS = (0, 1, 4)
PICKS = {"home": lambda x, y: x > y, "draw": lambda x, y: x == y, "away": lambda x, y: x < y}


def _brute(G, cell):
    """[G+1]^4 of cell(a, b, x, y) on the readable cells, 0 elsewhere."""
    w = np.zeros((G + 1,) * 4)
    for a, b, x, y in itertools.product(range(G + 1), repeat=4):
        if a <= x and b <= y:
            w[a, b, x, y] = float(cell(a, b, x, y))
    return w


def _same(market, G, cell):
    got = market.weights(G)
    assert got.shape == (G + 1,) * 4 and got.dtype == np.float64 and got.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(np.where(PR.readable(G), got, 0.0), _brute(G, cell), err_msg=repr(market))


@pytest.mark.parametrize("G", GS)
def test_builders_against_a_quadruple_loop(G):
    for pick, won in PICKS.items():
        _same(PD.first_period(pick), G, lambda a, b, x, y: won(a, b))
        _same(PD.second_period(pick), G, lambda a, b, x, y: won(x - a, y - b))
        _same(PD.full_time(pick), G, lambda a, b, x, y: won(x, y))
    _same(PD.first_period(MK.total_over(0.5)), G, lambda a, b, x, y: a + b > 0.5)
    _same(PD.first_period(MK.goals("away")), G, lambda a, b, x, y: b)
    _same(PD.second_period(MK.correct_score(1, 0)), G, lambda a, b, x, y: x - a == 1 and y - b == 0)
    _same(PD.second_period(MK.total_goals()), G, lambda a, b, x, y: x - a + y - b)
    _same(PD.full_time(MK.btts()), G, lambda a, b, x, y: x > 0 and y > 0)
    _same(PD.full_time(MK.handicap(-1.5, "home")), G, lambda a, b, x, y: x - 1.5 > y)
    for first, final in itertools.product(PICKS, repeat=2):
        _same(PD.ht_ft(first, final), G, lambda a, b, x, y: PICKS[first](a, b) and PICKS[final](x, y))
    for side, s in (("home", 1), ("away", -1)):
        _same(PD.win_both_periods(side), G, lambda a, b, x, y: s * (a - b) > 0 and s * ((x - a) - (y - b)) > 0)
        _same(PD.win_either_period(side), G, lambda a, b, x, y: s * (a - b) > 0 or s * ((x - a) - (y - b)) > 0)
        _same(PD.comeback(side), G, lambda a, b, x, y: s * (a - b) < 0 and s * (x - y) > 0)
    _same(PD.score_in_both_periods("home"), G, lambda a, b, x, y: a > 0 and x - a > 0)
    _same(PD.score_in_both_periods("away"), G, lambda a, b, x, y: b > 0 and y - b > 0)
    _same(PD.highest_scoring_period("first"), G, lambda a, b, x, y: a + b > x - a + y - b)
    _same(PD.highest_scoring_period("second"), G, lambda a, b, x, y: a + b < x - a + y - b)
    _same(PD.highest_scoring_period("equal"), G, lambda a, b, x, y: a + b == x - a + y - b)


@pytest.mark.parametrize("G", GS)
def test_all_of_is_the_product_and_partitions(G):
    one, two, three = PD.first_period("home"), PD.full_time(MK.goals("home")), PD.second_period(MK.total_under(2))
    np.testing.assert_array_equal(PD.all_of(one, two, three).weights(G),
                                  one.weights(G) * two.weights(G) * three.weights(G))
    np.testing.assert_array_equal(PD.all_of(one).weights(G), one.weights(G))
    # the nine half-time/full-time cells partition the readable cells; so do the three highest-scoring periods
    total = sum(PD.ht_ft(first, final).weights(G) for first, final in itertools.product(PICKS, repeat=2))
    assert (total[PR.readable(G)] == 1.0).all()
    total = sum(PD.highest_scoring_period(w).weights(G) for w in ("first", "second", "equal"))
    assert (total[PR.readable(G)] == 1.0).all()
    # first_goal: one side scores first unless nobody scores
    np.testing.assert_array_equal(MK.first_goal("home").weights(G) + MK.first_goal("away").weights(G)
                                  + MK.correct_score(0, 0).weights(G), np.ones((G + 1, G + 1)))
    x, y = np.meshgrid(np.arange(G + 1), np.arange(G + 1), indexing="ij")
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(MK.first_goal("home").weights(G), np.where(x + y > 0, x / (x + y), 0.0))


def test_builder_arguments():
    for bad in ("left", None, 0, "draw"):
        for builder in (PD.win_both_periods, PD.win_either_period, PD.score_in_both_periods, PD.comeback,
                        MK.first_goal):
            with pytest.raises(ValueError):
                builder(bad)
    for bad in ("home_win", None, 1, np.ones((2, 2)), PD.first_period("home")):
        for builder in (PD.first_period, PD.second_period, PD.full_time):
            with pytest.raises(ValueError):
                builder(bad)
    for bad in (("home", "x"), ("x", "home"), (MK.draw(), "home"), (None, None)):
        with pytest.raises(ValueError):
            PD.ht_ft(*bad)
    for bad in ("third", None, 1):
        with pytest.raises(ValueError):
            PD.highest_scoring_period(bad)
    for bad in ((), (MK.draw(),), (PD.first_period("home"), "home")):
        with pytest.raises(ValueError):
            PD.all_of(*bad)


@pytest.mark.parametrize("G", [0, 1, 2, 8])
def test_restatement_sums_to_the_grid(G):
    # sum_{a, b} p(a, b, x, y) = q(x, y) for every split: the law is the one predict_markets uses
    rs = np.random.RandomState(G)
    lh, la, rho = rs.uniform(0.2, 3.0, (5, 6)), rs.uniform(0.2, 3.0, (5, 6)), rs.uniform(-0.2, 0.2, 5)
    f = np.array([0.0, 1.0 / 9.0, 0.5, 1.0, rs.uniform(), 0.9])
    p = PR.joint(lh, la, rho, f, G)
    assert not np.isnan(p).any() and (p >= 0.0).all()
    np.testing.assert_allclose(p.sum(axis=(2, 3)), SR.grid(lh, la, rho, G), rtol=0, atol=1e-15)
    assert (p[~np.broadcast_to(PR.readable(G), p.shape)] == 0.0).all()
    assert (p[:, 0, 1:] == 0.0).all() and (p[:, 0, :, 1:] == 0.0).all()            # split 0: nothing before it
    off = ~np.eye(G + 1, dtype=bool)
    q = p[:, 3].transpose(0, 1, 3, 2, 4)                                             # [S, a, x, b, y]
    assert (q[:, off] == 0.0).all() and (q[:, :, :, off] == 0.0).all()               # split 1: a = x and b = y


class FailCtx:
    """A device context that must never be touched."""

    def __getattr__(self, name):
        raise AssertionError(f"device call {name} before the host checks finished")


class PeriodCtx(FakePredictCtx):
    """FakePredictCtx plus `period_summary`, computed by the restatement from the uploaded posterior."""

    def __init__(self):
        self.calls = []

    def period_summary(self, home_idx, away_idx, split, max_goals, weights, quantiles=(), neutral=None, conf=None,
                       return_draws=False, workspace_bytes=0):
        h, a = np.asarray(home_idx, int), np.asarray(away_idx, int)
        self.calls.append(h.size)
        assert np.shape(split) == (h.size,)
        eh, ea = self._log_rates(h, a, neutral, conf)
        return PR.device_part(np.exp(eh), np.exp(ea), self.cc, split, weights, quantiles, max_goals, return_draws)


@pytest.mark.parametrize("kind", LR.KINDS)
def test_result_keys_shapes_and_dtypes(kind):
    m = LR.hand_model(kind, S=9, T=6, seed=1)
    d = LR.hand_data(m, n=23, seed=2)
    for k in ("home_goals", "away_goals"):
        d.pop(k)   # the goal columns are not needed
    m._predict_ctx = ctx = PeriodCtx()
    G = 3
    mk = PR.all_builders()
    mk["ft_btts"] = PD.full_time(MK.btts())
    mk["array"] = np.random.RandomState(3).uniform(-2, 2, (G + 1,) * 4)
    qs = (0.0, 0.1, 0.5, 1.0)
    split = np.random.RandomState(4).uniform(0, 1, 23)
    r = m.predict_periods(d, mk, split=split, max_goals=G, quantiles=qs, return_draws=True)
    K = len(mk)
    assert len(ctx.calls) == (len(np.unique(d["gameweek"])) if kind == "dynamic" else 1) and sum(ctx.calls) == 23
    assert set(r) == {"kind", "n", "markets", "quantiles", "split", "mean", "sd", "quantile", "draws"}
    assert r["kind"] == "periods" and r["n"] == 23 and r["markets"] == tuple(mk)
    assert r["quantiles"].dtype == np.float64 and r["quantiles"].tolist() == list(qs)
    assert r["split"].dtype == np.float64 and r["split"].shape == (23,) and (r["split"] == split).all()
    for key, shape in (("mean", (K, 23)), ("sd", (K, 23)), ("quantile", (K, 4, 23)), ("draws", (9, K, 23))):
        assert r[key].shape == shape and r[key].dtype == np.float64, key
    # the per-fixture splits reach their fixtures through the groups' positions
    ref = PR.predict_periods(m, d, mk, split, G, qs)
    for key in ("mean", "sd", "quantile", "draws"):
        np.testing.assert_allclose(r[key], ref[key], rtol=1e-12, atol=1e-14, err_msg=key)
    # one number serves every fixture; without return_draws there are no draws; Q = 0 is allowed
    r2 = m.predict_periods(LR.hand_data(m, n=23, seed=2), mk, split=0.25, max_goals=G, quantiles=())
    assert "draws" not in r2 and r2["quantile"].shape == (K, 0, 23) and r2["quantiles"].shape == (0,)
    assert (r2["split"] == 0.25).all() and r2["split"].shape == (23,)
    np.testing.assert_allclose(r2["mean"], PR.predict_periods(m, d, mk, 0.25, G, ())["mean"], rtol=1e-12, atol=1e-14)
    # a market of the final score alone has predict_markets' value, whatever the split
    full = MR.predict_markets(m, d, {"home_win": MK.home_win(), "btts": MK.btts()}, G, qs)
    i = {name: k for k, name in enumerate(mk)}
    np.testing.assert_allclose(r["draws"][:, [i["ft_home"], i["ft_btts"]]], full["draws"], rtol=0, atol=1e-14)


def _raises(m, data, markets, **kwargs):
    m._predict_ctx = FailCtx()
    with pytest.raises(ValueError):
        m.predict_periods(data, markets, **kwargs)


@pytest.mark.parametrize("kind", LR.KINDS)
def test_argument_checks_run_on_the_host(kind):
    m = LR.hand_model(kind, S=16)
    good = LR.hand_data(m, n=6)
    ok = {"ht_home": PD.first_period("home")}
    _raises(m, {k: [] for k in good}, ok)                              # no fixture
    for g in (-1, 32, 2.0, True, None, "15"):
        _raises(m, good, ok, max_goals=g)
    for split in (-0.1, 1.5, np.nan, np.inf, "half", None, True, [0.5] * 5, [0.5] * 7, [[0.5] * 6],
                  [0.5, 0.5, np.nan, 0.5, 0.5, 0.5], [0.5, 0.5, 0.5, 0.5, 0.5, 1.0 + 1e-12]):
        _raises(m, good, ok, split=split)
    _raises(m, good, {})                                               # K = 0
    _raises(m, good, [PD.first_period("home")])                        # not a dict
    _raises(m, good, {f"m{k}": PD.first_period(MK.correct_score(k, 0)) for k in range(33)}, max_goals=1)   # K = 33
    _raises(m, good, {"ft": MK.home_win()}, max_goals=2)               # a full-time market, not wrapped
    _raises(m, good, ok, quantiles=np.linspace(0, 1, 17))              # Q = 17
    for q in (1.5, -0.1, np.nan):
        _raises(m, good, ok, quantiles=(0.5, q))
    w = np.ones((3, 3, 3, 3))
    for bad in (np.inf, -np.inf, np.nan):
        v = w.copy()
        v[1, 0, 2, 1] = bad
        _raises(m, good, {"w": v}, max_goals=2)                        # a non-finite weight
    _raises(m, good, {"w": np.ones((3, 3, 3, 2))}, max_goals=2)        # shape
    _raises(m, good, {"w": np.ones((3, 3))}, max_goals=2)
    _raises(m, good, {"w": w}, max_goals=3)
    _raises(m, good, {"w": "ht_home"}, max_goals=2)
    _raises(m, dict(good, home_team=["nope"] + list(good["home_team"][1:])), ok, max_goals=2)   # unknown team
    _raises(m, dict(good, away_team=list(good["away_team"][:-1])), ok, max_goals=2)
    if kind == "dynamic":
        d = dict(good)
        d.pop("gameweek")
        _raises(m, d, ok, max_goals=2)


def test_draw_limit_runs_on_the_host():
    big = LR.hand_model("neutral", S=65537, T=2)
    _raises(big, LR.hand_data(big, n=2), {"ht_draw": PD.first_period("draw")}, max_goals=1)
