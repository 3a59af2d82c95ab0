"""predict_markets without a GPU (bpl/markets.py): every builder's weights against a brute-force double loop
over the cells, the partitions the builders must form, result keys, shapes and dtypes for each class through a
stand-in context whose `market_summary` is the numpy restatement (tests/markets_ref.py), and every argument
check, made on the host before a device context is touched."""
import numpy as np
import pytest

import loglik_ref as LR
import markets_ref as MR
from bpl import markets as MK
from fake_ctx import FakePredictCtx

GS = (0, 1, 6)
LINES = (-1.5, -1, 0, 2, 2.5)


def _brute(G, cell):
    w = np.zeros((G + 1, G + 1))
    for x in range(G + 1):
        for y in range(G + 1):
            w[x, y] = float(cell(x, y))
    return w


def _same(market, G, cell):
    got = market.weights(G)
    assert got.shape == (G + 1, G + 1) and got.dtype == np.float64 and got.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(got, _brute(G, cell), err_msg=repr(market))


@pytest.mark.parametrize("G", GS)
def test_builders_against_a_double_loop(G):
    _same(MK.home_win(), G, lambda x, y: x > y)
    _same(MK.draw(), G, lambda x, y: x == y)
    _same(MK.away_win(), G, lambda x, y: x < y)
    _same(MK.btts(), G, lambda x, y: x > 0 and y > 0)
    _same(MK.clean_sheet("home"), G, lambda x, y: y == 0)
    _same(MK.clean_sheet("away"), G, lambda x, y: x == 0)
    _same(MK.goals("home"), G, lambda x, y: x)
    _same(MK.goals("away"), G, lambda x, y: y)
    _same(MK.total_goals(), G, lambda x, y: x + y)
    for cx, cy in ((0, 0), (1, 0), (0, 1), (2, 5), (6, 6), (7, 0), (200, 3)):
        _same(MK.correct_score(cx, cy), G, lambda x, y: x == cx and y == cy)
        if cx > G or cy > G:
            assert not MK.correct_score(cx, cy).weights(G).any()   # off the grid: all zeros
    for line in LINES:
        _same(MK.total_over(line), G, lambda x, y: x + y > line)
        _same(MK.total_under(line), G, lambda x, y: x + y < line)
        _same(MK.handicap(line), G, lambda x, y: x + line > y)
        _same(MK.handicap(line, "home"), G, lambda x, y: x + line > y)
        _same(MK.handicap(line, side="away"), G, lambda x, y: y + line > x)


@pytest.mark.parametrize("G", GS)
def test_partitions(G):
    ones = np.ones((G + 1, G + 1))
    np.testing.assert_array_equal(MK.home_win().weights(G) + MK.draw().weights(G) + MK.away_win().weights(G), ones)
    x, y = np.meshgrid(np.arange(G + 1), np.arange(G + 1), indexing="ij")
    for line in LINES:
        both = MK.total_over(line).weights(G) + MK.total_under(line).weights(G)
        push = (x + y == line)   # (no cell for a fractional or negative line)
        np.testing.assert_array_equal(both, np.where(push, 0.0, 1.0))
        assert (MK.total_over(line).weights(G)[push] == 0).all() and (MK.total_under(line).weights(G)[push] == 0).all()


def test_builder_arguments():
    for bad in ("left", None, 0):
        with pytest.raises(ValueError):
            MK.clean_sheet(bad)
        with pytest.raises(ValueError):
            MK.goals(bad)
        with pytest.raises(ValueError):
            MK.handicap(1, bad)
    for bad in (np.nan, np.inf, "2.5", None, True):
        with pytest.raises(ValueError):
            MK.total_over(bad)
        with pytest.raises(ValueError):
            MK.total_under(bad)
        with pytest.raises(ValueError):
            MK.handicap(bad)
    for bad in (-1, 1.0, None):
        with pytest.raises(ValueError):
            MK.correct_score(bad, 0)


class FailCtx:
    """A device context that must never be touched."""

    def __getattr__(self, name):
        raise AssertionError(f"device call {name} before the host checks finished")


class MarketCtx(FakePredictCtx):
    """FakePredictCtx plus `market_summary`, computed by the restatement from the uploaded posterior."""

    def __init__(self):
        self.calls = []

    def market_summary(self, home_idx, away_idx, max_goals, weights, quantiles=(), neutral=None, conf=None,
                       return_draws=False, workspace_bytes=0):
        h, a = np.asarray(home_idx, int), np.asarray(away_idx, int)
        self.calls.append(h.size)
        eh, ea = self._log_rates(h, a, neutral, conf)
        return MR.device_part(np.exp(eh), np.exp(ea), self.cc, weights, quantiles, max_goals, return_draws)


@pytest.mark.parametrize("kind", LR.KINDS)
def test_result_keys_shapes_and_dtypes(kind):
    m = LR.hand_model(kind, S=9, T=6, seed=1)
    d = LR.hand_data(m, n=23, seed=2)
    for k in ("home_goals", "away_goals"):
        d.pop(k)   # the goal columns are not needed
    m._predict_ctx = ctx = MarketCtx()
    G = 5
    mk = MR.all_builders()
    mk["array"] = np.random.RandomState(3).uniform(-2, 2, (G + 1, G + 1))
    qs = (0.0, 0.1, 0.5, 1.0)
    r = m.predict_markets(d, mk, max_goals=G, quantiles=qs, return_draws=True)
    K = len(mk)
    assert len(ctx.calls) == (len(np.unique(d["gameweek"])) if kind == "dynamic" else 1) and sum(ctx.calls) == 23
    assert set(r) == {"kind", "n", "markets", "quantiles", "mean", "sd", "quantile", "draws"}
    assert r["kind"] == "markets" and r["n"] == 23 and r["markets"] == tuple(mk)
    assert r["quantiles"].dtype == np.float64 and r["quantiles"].tolist() == list(qs)
    for key, shape in (("mean", (K, 23)), ("sd", (K, 23)), ("quantile", (K, 4, 23)), ("draws", (9, K, 23))):
        assert r[key].shape == shape and r[key].dtype == np.float64, key
    ref = MR.predict_markets(m, d, mk, G, qs)
    for key in ("mean", "sd", "quantile", "draws"):
        np.testing.assert_allclose(r[key], ref[key], rtol=1e-12, atol=1e-14, err_msg=key)
    # with the goal columns present the result is the same; without return_draws there are no draws; Q = 0 is allowed
    full = LR.hand_data(m, n=23, seed=2)
    r2 = m.predict_markets(full, mk, max_goals=G, quantiles=())
    assert "draws" not in r2 and r2["quantile"].shape == (K, 0, 23) and r2["quantiles"].shape == (0,)
    np.testing.assert_array_equal(r2["mean"], r["mean"])
    # a quantile of a sum is not the sum of the quantiles, a mean is
    i = {name: k for k, name in enumerate(mk)}
    np.testing.assert_allclose(r["mean"][i["total_goals"]], r["mean"][i["goals_home"]] + r["mean"][i["goals_away"]],
                               rtol=1e-12)
    assert (np.abs(r["quantile"][i["total_goals"], 1] - r["quantile"][i["goals_home"], 1]
                   - r["quantile"][i["goals_away"], 1]) > 1e-6).any()


def _raises(m, data, markets, **kwargs):
    m._predict_ctx = FailCtx()
    with pytest.raises(ValueError):
        m.predict_markets(data, markets, **kwargs)


@pytest.mark.parametrize("kind", LR.KINDS)
def test_argument_checks_run_on_the_host(kind):
    m = LR.hand_model(kind, S=16)
    good = LR.hand_data(m, n=6)
    ok = {"home_win": MK.home_win()}
    _raises(m, {k: [] for k in good}, ok)                              # no fixture
    for g in (-1, 64, 2.0, True, None, "15"):
        _raises(m, good, ok, max_goals=g)
    _raises(m, good, {})                                               # K = 0
    _raises(m, good, [MK.home_win()])                                  # not a dict
    _raises(m, good, {f"m{k}": MK.correct_score(k, 0) for k in range(65)})   # K = 65
    _raises(m, good, ok, quantiles=np.linspace(0, 1, 17))              # Q = 17
    for q in (1.5, -0.1, np.nan, np.inf):
        _raises(m, good, ok, quantiles=(0.5, q))
    _raises(m, good, ok, quantiles=[[0.5]])
    _raises(m, good, ok, quantiles=("a",))
    w = np.ones((16, 16))
    for bad in (np.inf, -np.inf, np.nan):
        _raises(m, good, {"w": np.where(np.eye(16) > 0, bad, w)})      # a non-finite weight
    _raises(m, good, {"w": np.ones((16, 15))})                         # shape
    _raises(m, good, {"w": np.ones((7, 7))})
    _raises(m, good, {"w": np.ones((16, 16))}, max_goals=6)
    _raises(m, good, {"w": "home_win"})
    _raises(m, dict(good, home_team=["nope"] + list(good["home_team"][1:])), ok)   # unknown team
    _raises(m, dict(good, away_team=list(good["away_team"][:-1])), ok)
    if kind in ("neutral", "wc", "dynamic"):
        _raises(m, dict(good, neutral_venue=[2] + list(good["neutral_venue"][1:])), ok)
    if kind == "wc":
        _raises(m, dict(good, home_conf=["nope"] + list(good["home_conf"][1:])), ok)
    if kind == "dynamic":
        d = dict(good)
        d.pop("gameweek")
        _raises(m, d, ok)
        m._predict_ctx = FailCtx()
        with pytest.raises(IndexError):
            m.predict_markets(dict(good, gameweek=[m.num_gameweeks] + list(good["gameweek"][1:])), ok)


def test_draw_limit_runs_on_the_host():
    big = LR.hand_model("neutral", S=65537, T=2)
    _raises(big, LR.hand_data(big, n=2), {"draw": MK.draw()})
