"""predict_slate without a GPU (bpl/slate.py): every builder's table against a brute-force double loop over the
cells, `prediction_points`' precedence and argument checks, every argument check of `predict_slate`, made on the
host before a device context is touched, and result keys, shapes and dtypes for each class through a stand-in
context whose `slate_summary` is the numpy restatement (tests/slate_ref.py)."""
import numpy as np
import pytest

import loglik_ref as LR
import slate_ref as SLR
from bpl import markets as MK
from bpl import slate as SL
from fake_ctx import FakePredictCtx

GS = (0, 1, 6)


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


def _sign(v):
    return (v > 0) - (v < 0)


def _points(px, py, exact, gd, result):
    def cell(x, y):
        if (x, y) == (px, py):
            return exact
        if gd is not None and x - y == px - py:
            return gd
        return result if _sign(x - y) == _sign(px - py) else 0
    return cell


@pytest.mark.parametrize("G", GS)
def test_builders_against_a_double_loop(G):
    _same(SL.pick("home"), G, lambda x, y: x > y)
    _same(SL.pick("draw"), G, lambda x, y: x == y)
    _same(SL.pick("away"), G, lambda x, y: x < y)
    for cap in (1, 3, 7):
        _same(SL.capped(MK.total_goals(), cap), G, lambda x, y: min(x + y, cap))
        _same(SL.capped(MK.goals("away"), cap), G, lambda x, y: min(y, cap))
        _same(SL.capped(MK.btts(), cap), G, lambda x, y: x > 0 and y > 0)
    for px, py in ((0, 0), (2, 1), (1, 1), (0, 3), (9, 0)):
        _same(SL.prediction_points(px, py), G, _points(px, py, 3, None, 1))
        _same(SL.prediction_points(px, py, exact=5, goal_difference=2, result=1), G, _points(px, py, 5, 2, 1))
        _same(SL.prediction_points(px, py, exact=7, goal_difference=7, result=0), G, _points(px, py, 7, 7, 0))
        _same(SL.prediction_points(px, py, exact=0, result=0), G, lambda x, y: 0)


def test_prediction_points_precedence():
    w = SL.prediction_points(2, 1, exact=5, goal_difference=3, result=1).weights(6)
    assert w[2, 1] == 5                       # the exact score, not its goal difference or result
    assert w[1, 0] == 3 and w[3, 2] == 3      # the goal difference, not the result
    assert w[2, 0] == 1 and w[6, 0] == 1      # the result alone
    assert w[1, 1] == 0 and w[0, 1] == 0
    d = SL.prediction_points(1, 1, exact=4, goal_difference=2, result=1).weights(6)
    assert d[1, 1] == 4 and d[0, 0] == 2 and d[3, 3] == 2 and d[1, 0] == 0   # every draw has the goal difference 0
    assert SL.prediction_points(1, 1).weights(6)[2, 2] == 1                  # without it a draw is the right result


def test_builder_arguments():
    for bad in ("left", None, 0, "Home"):
        with pytest.raises(ValueError):
            SL.pick(bad)
    for bad in (0, 8, 2.0, True, None):
        with pytest.raises(ValueError):
            SL.capped(MK.total_goals(), bad)
    with pytest.raises(ValueError):
        SL.capped(np.ones((3, 3)), 2)
    for kwargs in ({"exact": 8}, {"exact": -1}, {"exact": 2.0}, {"result": 4}, {"result": -1}, {"result": True},
                   {"goal_difference": 4}, {"goal_difference": 0}, {"goal_difference": 1.5},
                   {"exact": 3, "goal_difference": 2, "result": 3}):
        with pytest.raises(ValueError):
            SL.prediction_points(1, 0, **kwargs)
    for bad in (-1, 1.0, None):
        with pytest.raises(ValueError):
            SL.prediction_points(bad, 0)
        with pytest.raises(ValueError):
            SL.prediction_points(0, bad)


class FailCtx:
    """A device context that must never be touched."""

    def __getattr__(self, name):
        raise AssertionError(f"device call {name} before the host checks finished")


class SlateCtx(FakePredictCtx):
    """FakePredictCtx plus `slate_summary`, computed by the restatement from the uploaded posterior."""

    def __init__(self):
        self.calls = []

    def slate_summary(self, home_idx, away_idx, max_goals, tables, leg_table, start, quantiles=(), neutral=None,
                      conf=None, return_draws=False, workspace_bytes=0):
        h, a = np.asarray(home_idx, int), np.asarray(away_idx, int)
        start = np.asarray(start)
        assert start[0] == 0 and start[-1] == h.size and (np.diff(start) > 0).all()
        self.calls.append(h.size)
        eh, ea = self._log_rates(h, a, neutral, conf)
        return SLR.device_part(np.exp(eh), np.exp(ea), self.cc, tables, leg_table, start, quantiles, max_goals,
                               return_draws)


def _without_goals(m, n, seed):
    d = LR.hand_data(m, n=n, seed=seed)
    for k in ("home_goals", "away_goals"):
        d.pop(k)
    return d


def _mixed_legs(n, G, seed=0):
    rs = np.random.RandomState(seed)
    kinds = [SL.pick("home"), SL.pick("away"), MK.btts(), MK.total_over(2.5), SL.capped(MK.total_goals(), 3),
             SL.prediction_points(2, 1, exact=3, goal_difference=2, result=1), SL.prediction_points(1, 1),
             rs.randint(0, 3, (G + 1, G + 1))]
    return [kinds[i % len(kinds)] for i in range(n)]


@pytest.mark.parametrize("kind", LR.KINDS)
def test_result_keys_shapes_and_dtypes(kind):
    m = LR.hand_model(kind, S=9, T=6, seed=1)
    n, G = 12, 5
    d = _without_goals(m, n, 2)
    labels = np.array([7, -2, 7, 7, 30, -2, 30, 7, 30, 30, 7, 30])
    if kind == "dynamic":
        d["gameweek"] = np.where(labels == 7, 1, 0)   # slate 7 in gameweek 1, the others in gameweek 0
    m._predict_ctx = ctx = SlateCtx()
    legs = _mixed_legs(n, G)
    qs = (0.0, 0.1, 0.5, 1.0)
    r = m.predict_slate(d, legs, slate=labels, max_goals=G, quantiles=qs, return_draws=True)
    assert len(ctx.calls) == (2 if kind == "dynamic" else 1) and sum(ctx.calls) == n
    ref = SLR.predict_slate(m, d, legs, labels, G, qs)
    J, P, Q = 3, int(ref["max_total"].max()), 4
    shapes = {"pmf": (J, P + 1), "pmf_sd": (J, P + 1), "pmf_quantile": (J, Q, P + 1), "at_least": (J, P + 1),
              "at_least_sd": (J, P + 1), "at_least_quantile": (J, Q, P + 1), "expected": (J,), "expected_sd": (J,),
              "expected_quantile": (J, Q), "mass": (J,), "top_proba": (J,), "leg_proba": (n, 8),
              "independent_pmf": (J, P + 1), "independent_at_least": (J, P + 1), "pmf_draws": (9, J, P + 1)}
    assert set(r) == set(shapes) | {"kind", "n", "slates", "size", "max_total", "totals", "quantiles"}
    assert r["kind"] == "slate" and r["n"] == n
    assert r["slates"].tolist() == [-2, 7, 30] and r["size"].tolist() == [2, 5, 5]
    np.testing.assert_array_equal(r["max_total"], ref["max_total"])
    np.testing.assert_array_equal(r["totals"], np.arange(P + 1))
    assert r["quantiles"].dtype == np.float64 and r["quantiles"].tolist() == list(qs)
    for key, shape in shapes.items():
        assert r[key].shape == shape and r[key].dtype == np.float64, key
        np.testing.assert_allclose(r[key], ref[key], rtol=1e-12, atol=1e-15, err_msg=key)
    for j in range(J):
        assert (r["pmf"][j, r["max_total"][j] + 1:] == 0.0).all() and (r["pmf_draws"][:, j, r["max_total"][j] + 1:] == 0.0).all()
        assert r["top_proba"][j] == r["pmf"][j, r["max_total"][j]]
    # the host-formed comparison: the posterior means of the legs' laws convolved in list order
    for j, label in enumerate(r["slates"]):
        want = np.ones(1)
        for i in np.nonzero(labels == label)[0]:
            want = np.convolve(want, r["leg_proba"][i])
        want = want[:P + 1]
        np.testing.assert_allclose(r["independent_pmf"][j, :want.size], want, rtol=0, atol=1e-15)
        np.testing.assert_allclose(r["independent_at_least"][j], np.cumsum(r["independent_pmf"][j][::-1])[::-1],
                                   rtol=0, atol=1e-15)
    # a nested list is one leg for every fixture, as the same ndarray is
    table = legs[7]
    as_list = m.predict_slate(d, table.tolist(), slate=labels, max_goals=G, quantiles=qs)
    as_array = m.predict_slate(d, table, slate=labels, max_goals=G, quantiles=qs)
    assert as_list["pmf"].tobytes() == as_array["pmf"].tobytes() and as_list["max_total"].tolist() == [4, 10, 10]
    # one leg for all, one slate, no draws, no quantiles
    r2 = m.predict_slate(dict(d, gameweek=np.zeros(n, dtype=int)) if kind == "dynamic" else d, SL.pick("home"),
                         max_goals=G, quantiles=())
    assert "pmf_draws" not in r2 and r2["pmf"].shape == (1, n + 1) and r2["pmf_quantile"].shape == (1, 0, n + 1)
    assert r2["slates"].tolist() == [0] and r2["size"].tolist() == [n] and r2["max_total"].tolist() == [n]
    assert r2["top_proba"][0] == r2["pmf"][0, n]


def _fresh(m):
    """A new stand-in context for `m`, which uploads its posterior to it on the next call."""
    m._predict_ctx = ctx = SlateCtx()
    m.invalidate_predict_cache()
    return ctx


def _raises(m, data, legs, **kwargs):
    m._predict_ctx = FailCtx()
    with pytest.raises(ValueError) as e:
        m.predict_slate(data, legs, **kwargs)
    return str(e.value)


@pytest.mark.parametrize("kind", LR.KINDS)
def test_argument_checks_run_on_the_host(kind):
    m = LR.hand_model(kind, S=16)
    good = _without_goals(m, 6, 1)
    if kind == "dynamic":
        good["gameweek"] = np.zeros(6, dtype=int)
    ok = SL.pick("home")
    _raises(m, {k: [] for k in good}, ok)                               # n = 0
    for g in (-1, 64, 2.0, True, None, "15"):
        _raises(m, good, ok, max_goals=g)
    _raises(m, good, ok, quantiles=np.linspace(0, 1, 17))
    for q in (1.5, -0.1, np.nan, np.inf):
        _raises(m, good, ok, quantiles=(0.5, q))
    _raises(m, good, ok, quantiles=[[0.5]])
    _raises(m, good, ok, quantiles=("a",))
    # the legs
    _raises(m, good, np.full((16, 16), 0.5))                            # non-integer weights
    _raises(m, good, MK.handicap(0.5).weights(15) * 1.5)
    _raises(m, good, -np.ones((16, 16)))
    _raises(m, good, np.where(np.eye(16) > 0, np.nan, 1.0))
    _raises(m, good, np.full((16, 16), 8))                              # values above 7
    msg = _raises(m, good, [ok, ok, ok, MK.goals("home"), ok, ok])
    assert "fixture 3" in msg and "cap" in msg                          # names the fixture, says to cap it
    assert "fixture 0" in _raises(m, good, MK.total_goals())
    _raises(m, good, [ok] * 5)                                          # a wrong leg count
    _raises(m, good, [ok] * 7)
    _raises(m, good, [])
    _raises(m, good, 3)
    _raises(m, good, [ok, ok, ok, "home", ok, ok])
    _raises(m, good, [[0, 1], [1]])                                     # a ragged nested list
    _raises(m, good, np.ones((16, 15), dtype=int))                      # shape
    _raises(m, good, np.ones((7, 7), dtype=int))
    _raises(m, good, np.ones((16, 16), dtype=int), max_goals=6)
    # the slates
    _raises(m, good, ok, slate=[0, 1, 2])                               # labels of the wrong length
    _raises(m, good, ok, slate=[0, 0, 0, 0, 0, 0.5])                    # or type
    _raises(m, good, ok, slate=["a"] * 6)
    _raises(m, good, ok, slate=[[0] * 6])
    _raises(m, good, ok, slate=3)
    big = {k: (list(v) * 171)[:1025] for k, v in good.items()}          # more than 1024 legs in a slate
    _raises(m, big, np.zeros((16, 16), dtype=int))
    ctx = _fresh(m)
    assert m.predict_slate({k: v[:130] for k, v in big.items()}, np.zeros((2, 2), dtype=int), max_goals=1,
                           slate=[0] * 129 + [1], quantiles=())["pmf"].shape == (2, 1) and ctx.calls == [130]
    many = {k: (list(v) * 22)[:128] for k, v in good.items()}           # sum m_i > 127
    _raises(m, many, ok)
    _raises(m, {k: v[:19] for k, v in many.items()}, SL.capped(MK.total_goals(), 7))   # 19 x 7 = 133
    _raises(m, many, ok, slate=[0] * 128)
    _fresh(m)
    assert m.predict_slate(many, ok, slate=[0] * 127 + [1], max_goals=1, quantiles=())["max_total"].tolist() == [127, 1]
    # the data
    _raises(m, dict(good, home_team=["nope"] + list(good["home_team"][1:])), ok)
    _raises(m, dict(good, away_team=list(good["away_team"][:-1])), ok)
    if kind in ("neutral", "wc", "dynamic"):
        _raises(m, dict(good, neutral_venue=[2] + list(good["neutral_venue"][1:])), ok)
    if kind == "wc":
        _raises(m, dict(good, home_conf=["nope"] + list(good["home_conf"][1:])), ok)
    if kind == "dynamic":
        d = dict(good)
        d.pop("gameweek")
        _raises(m, d, ok)
        across = dict(good, gameweek=[0, 0, 0, 1, 1, 1])
        assert "gameweek" in _raises(m, across, ok)                     # one slate across two gameweeks
        assert "gameweek" in _raises(m, across, ok, slate=[0, 0, 1, 0, 1, 1])
        _fresh(m)
        assert m.predict_slate(across, ok, slate=[5, 5, 5, 2, 2, 2], max_goals=3)["slates"].tolist() == [2, 5]


def test_draw_limit_runs_on_the_host():
    big = LR.hand_model("neutral", S=65537, T=2)
    d = _without_goals(big, 2, 1)
    _raises(big, d, SL.pick("draw"))
