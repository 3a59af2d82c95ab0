"""forecast_scores / compare_scores without a GPU: result keys, shapes and dtypes for each class through a
stand-in context whose `outcome_scores` is the numpy restatement (tests/scores_ref.py), the three rules
against hand-worked values, the standard errors, the reliability table on constructed forecasts, and every
argument check, made on the host before a device context is touched."""
import math

import numpy as np
import pytest

import loglik_ref as LR
import scores_ref as SR
from bpl import compare_scores
from bpl.scoring import calibration_table, rules
from fake_ctx import FakePredictCtx


class FailCtx:
    """A device context that must never be touched."""

    def __getattr__(self, name):
        raise AssertionError(f"device call {name} before the host checks finished")


class ScoreCtx(FakePredictCtx):
    """FakePredictCtx plus `outcome_scores`, computed by the restatement from the uploaded posterior."""

    def __init__(self):
        self.calls = []

    def outcome_scores(self, home_idx, away_idx, home_goals, away_goals, max_goals, neutral=None, conf=None):
        h, a = np.asarray(home_idx, int), np.asarray(away_idx, int)
        self.calls.append(h.size)
        eh, ea = self._log_rates(h, a, neutral, conf)
        return SR.device_part(np.exp(eh), np.exp(ea), self.cc, home_goals, away_goals, max_goals)


class FixedCtx:
    """A context that returns given forecasts for fixtures in data order."""

    def __init__(self, proba, draws):
        self.proba, self.draws = np.asarray(proba, dtype=np.float64), draws

    def predict_set_posterior(self, *args, **kwargs):
        pass

    def outcome_scores(self, home_idx, away_idx, home_goals, away_goals, max_goals, neutral=None, conf=None):
        return {"proba": self.proba, "draw_sums": np.zeros((self.draws, 3))}


@pytest.mark.parametrize("kind", LR.KINDS)
def test_result_keys_shapes_and_dtypes(kind):
    m = LR.hand_model(kind, S=9, T=6, seed=1)
    d = LR.hand_data(m, n=23, seed=2)
    m._predict_ctx = ctx = ScoreCtx()
    r = m.forecast_scores(d, max_goals=7, bins=5)
    assert len(ctx.calls) == (len(np.unique(d["gameweek"])) if kind == "dynamic" else 1) and sum(ctx.calls) == 23
    assert r["kind"] == "scores" and r["n"] == 23
    assert r["outcome"].dtype == np.uint8 and r["outcome"].shape == (23,)
    np.testing.assert_array_equal(r["outcome"], SR.outcome_of(d["home_goals"], d["away_goals"]))
    assert r["outcome_proba"].shape == (23, 3) and r["outcome_proba"].dtype == np.float64
    for name in ("log_score", "brier", "rps"):
        assert r[f"{name}_i"].shape == (23,) and r[f"{name}_i"].dtype == np.float64
        assert r[f"{name}_draws"].shape == (9,) and r[f"{name}_draws"].dtype == np.float64
        assert isinstance(r[name], float) and isinstance(r[f"{name}_se"], float)
    cal = r["calibration"]
    assert cal["bin_edges"].shape == (6,) and cal["count"].shape == (3, 5) and cal["count"].dtype == np.int64
    assert cal["mean_proba"].shape == (3, 5) and cal["observed"].shape == (3, 5)
    assert (cal["count"].sum(axis=1) == 23).all()
    assert set(r) == {"kind", "n", "outcome", "outcome_proba", "calibration"} | {
        f"{name}{suffix}" for name in ("log_score", "brier", "rps") for suffix in ("", "_i", "_se", "_draws")}
    # the host side adds nothing to the restatement beyond rounding
    ref = SR.scores(m, d, 7)
    for k, v in ref.items():
        if k != "p_draws":
            np.testing.assert_allclose(r[k], v, rtol=1e-12, atol=1e-14, err_msg=k)
    # the score of the mean forecast is not the mean score of the draws (Jensen: it is better)
    assert r["log_score"] > r["log_score_draws"].mean() and r["brier"] < r["brier_draws"].mean()


def test_rules_by_hand():
    m = LR.hand_model("basic", S=4, T=3)
    d = {"home_team": ["t00"], "away_team": ["t01"], "home_goals": [2], "away_goals": [1]}
    m._predict_ctx = FixedCtx([[0.5, 0.3, 0.2]], 4)
    r = m.forecast_scores(d)
    # home win: rps = ((0.5 - 1)^2 + (0.8 - 1)^2) / 2, brier = 0.25 + 0.09 + 0.04, log = log 0.5
    assert r["outcome"][0] == 0
    assert abs(r["rps"] - 0.145) < 1e-15 and abs(r["brier"] - 0.38) < 1e-15
    assert abs(r["log_score"] - math.log(0.5)) < 1e-15 and abs(r["log_score"] + 0.6931471805599453) < 1e-15
    assert r["rps_se"] == 0.0 and r["brier_se"] == 0.0 and r["log_score_se"] == 0.0      # n = 1
    # the same forecast against a draw and an away win
    got = rules(np.tile([0.5, 0.3, 0.2], (3, 1)), np.array([0, 1, 2]))
    np.testing.assert_allclose(got["rps"], [0.145, (0.25 + 0.04) / 2, (0.25 + 0.64) / 2], rtol=0, atol=1e-15)
    np.testing.assert_allclose(got["brier"], [0.38, 0.25 + 0.49 + 0.04, 0.25 + 0.09 + 0.64], rtol=0, atol=1e-15)
    np.testing.assert_allclose(got["log_score"], np.log([0.5, 0.3, 0.2]), rtol=0, atol=1e-15)


def test_standard_errors_and_zero_probability():
    m = LR.hand_model("basic", S=4, T=4)
    d = {"home_team": ["t00", "t01", "t02"], "away_team": ["t01", "t02", "t03"], "home_goals": [1, 0, 255],
         "away_goals": [0, 0, 3]}
    P = np.array([[0.6, 0.3, 0.1], [0.2, 0.5, 0.3], [0.25, 0.25, 0.5]])
    m._predict_ctx = FixedCtx(P, 4)
    r = m.forecast_scores(d)
    for name in ("log_score", "brier", "rps"):
        assert abs(r[f"{name}_se"] - np.std(r[f"{name}_i"], ddof=1) / math.sqrt(3)) < 1e-15
        assert abs(r[name] - r[f"{name}_i"].mean()) < 1e-15
    P[1] = [0.5, 0.0, 0.5]   # the draw that happened was given no chance
    r = m.forecast_scores(d)
    assert r["log_score_i"][1] == -math.inf and r["log_score"] == -math.inf and r["log_score_se"] == math.inf
    assert math.isfinite(r["brier"]) and math.isfinite(r["rps_se"])
    assert not any(np.isnan(np.asarray(v, dtype=np.float64)).any() for k, v in r.items()
                   if k not in ("kind", "calibration"))


def test_calibration_table():
    # class 0: p = 0, 0.05 | 0.3 | 1, 1 over four bins [0, .25) [.25, .5) [.5, .75) [.75, 1]; bin 2 is empty
    P = np.array([[0.0, 0.5, 0.5], [0.05, 0.25, 0.7], [0.3, 0.3, 0.4], [1.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    o = np.array([1, 0, 2, 0, 0], dtype=np.uint8)
    cal = calibration_table(P, o, bins=4)
    np.testing.assert_array_equal(cal["bin_edges"], [0.0, 0.25, 0.5, 0.75, 1.0])
    np.testing.assert_array_equal(cal["count"][0], [2, 1, 0, 2])          # p = 1 falls in the last bin
    np.testing.assert_allclose(cal["mean_proba"][0], [0.025, 0.3, np.nan, 1.0], rtol=0, atol=1e-15)
    np.testing.assert_allclose(cal["observed"][0], [0.5, 0.0, np.nan, 1.0], rtol=0, atol=1e-15)
    # class 1: p = 0, 0 | .25 (an edge: the bin above), .3, .5 (an edge again)
    np.testing.assert_array_equal(cal["count"][1], [2, 2, 1, 0])
    np.testing.assert_allclose(cal["observed"][1], [0.0, 0.0, 1.0, np.nan], rtol=0, atol=1e-15)
    assert np.isnan(cal["mean_proba"][1, 3])
    np.testing.assert_array_equal(cal["count"].sum(axis=1), [5, 5, 5])
    one = calibration_table(P, o, bins=1)
    np.testing.assert_array_equal(one["count"], [[5], [5], [5]])
    np.testing.assert_allclose(one["observed"][:, 0], [0.6, 0.2, 0.2], rtol=0, atol=1e-15)


def _raises(m, data, **kwargs):
    m._predict_ctx = FailCtx()
    with pytest.raises(ValueError):
        m.forecast_scores(data, **kwargs)


@pytest.mark.parametrize("kind", LR.KINDS)
def test_argument_checks_run_on_the_host(kind):
    m = LR.hand_model(kind, S=16)
    good = LR.hand_data(m, n=6)
    _raises(m, {k: [] for k in good})                       # no fixture
    for g in (-1, 64, 2.0, True, None, "15"):
        _raises(m, good, max_goals=g)
    for b in (0, 1001, -5, 10.0, True, None):
        _raises(m, good, bins=b)
    _raises(m, dict(good, home_team=["nope"] + list(good["home_team"][1:])))
    _raises(m, dict(good, away_goals=list(good["away_goals"][:-1])))
    _raises(m, dict(good, home_goals=[256] + list(good["home_goals"][1:])))
    _raises(m, dict(good, away_goals=[-1] + list(good["away_goals"][1:])))
    d = dict(good)
    d.pop("home_goals")
    _raises(m, d)
    if kind in ("neutral", "wc", "dynamic"):
        _raises(m, dict(good, neutral_venue=[2] + list(good["neutral_venue"][1:])))
    if kind == "wc":
        _raises(m, dict(good, home_conf=["nope"] + list(good["home_conf"][1:])))
    if kind == "dynamic":
        m._predict_ctx = FailCtx()
        with pytest.raises(IndexError):
            m.forecast_scores(dict(good, gameweek=[m.num_gameweeks] + list(good["gameweek"][1:])))


def test_draw_limit_runs_on_the_host():
    big = LR.hand_model("neutral", S=65537, T=2)
    _raises(big, LR.hand_data(big, n=2))


def _result(rs, n, outcome, loc):
    r = {"kind": "scores", "n": n, "outcome": outcome}
    for name in ("rps", "brier", "log_score"):
        v = rs.normal(-loc if name == "log_score" else loc, 0.1, n)
        r.update({f"{name}_i": v, name: float(v.mean()), f"{name}_se": float(np.std(v, ddof=1) / math.sqrt(n))})
    return r


@pytest.mark.parametrize("rule", ["rps", "brier", "log_score"])
def test_compare_scores_orders_each_rule(rule):
    rs = np.random.RandomState(0)
    o = rs.randint(0, 3, 40).astype(np.uint8)
    res = {"worst": _result(rs, 40, o, 0.9), "best": _result(rs, 40, o, 0.3), "middle": _result(rs, 40, o, 0.6)}
    out = compare_scores(res, rule=rule)
    assert list(out) == ["best", "middle", "worst"] and [v["rank"] for v in out.values()] == [0, 1, 2]
    assert out["best"]["diff"] == 0.0 and out["best"]["se_diff"] == 0.0
    sign = -1.0 if rule == "log_score" else 1.0
    for name in ("middle", "worst"):
        v = out[name]
        assert v["score"] == res[name][rule] and v["se"] == res[name][f"{rule}_se"]
        assert v["diff"] > 0 and abs(v["diff"] - sign * (res[name][rule] - res["best"][rule])) < 1e-15
        want = np.std(res[name][f"{rule}_i"] - res["best"][f"{rule}_i"], ddof=1) / math.sqrt(40)
        assert abs(v["se_diff"] - want) < 1e-15
    assert list(compare_scores(res)) == list(compare_scores(res, rule="rps"))


def test_compare_scores_refusals():
    rs = np.random.RandomState(1)
    o = rs.randint(0, 3, 30).astype(np.uint8)
    a, b = _result(rs, 30, o, 0.4), _result(rs, 30, o, 0.5)
    with pytest.raises(ValueError):
        compare_scores({})
    with pytest.raises(ValueError):
        compare_scores({"a": a, "b": b}, rule="elpd")
    with pytest.raises(ValueError):
        compare_scores({"a": a, "b": dict(b, kind="loo")})
    with pytest.raises(ValueError):
        compare_scores({"a": a, "b": _result(rs, 29, o[:29], 0.5)})
    other = o.copy()
    other[7] = (other[7] + 1) % 3
    with pytest.raises(ValueError):
        compare_scores({"a": a, "b": dict(b, outcome=other)})      # not the same matches
    # an infinite log score: ranked last, infinite difference, nothing NaN
    worse = dict(b)
    worse["log_score_i"] = b["log_score_i"].copy()
    worse["log_score_i"][3] = -math.inf
    worse.update(log_score=-math.inf, log_score_se=math.inf)
    out = compare_scores({"w": worse, "a": a}, rule="log_score")
    assert list(out) == ["a", "w"] and out["w"]["diff"] == math.inf and out["w"]["se_diff"] == math.inf
