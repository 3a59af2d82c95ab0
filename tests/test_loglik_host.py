"""log_likelihood / waic / loo without a GPU: the PSIS restatement (tests/loglik_ref.py) on known
cases, compare_elpd, and every argument check, all made on the host before a device context exists."""
import math

import numpy as np
import pytest
from scipy.stats import genpareto

import loglik_ref as R
from bpl import compare_elpd
from bpl.elpd import LOGLIK_MAX_TAIL, tail_size


@pytest.mark.parametrize("k", [0.2, 0.5, 0.9])
def test_gpd_fit_recovers_k(k):
    # L = 200 exceedances; the fit's prior pulls k toward 0.5 by 10 / 210 of the gap.  Sampling sd of
    # the estimate is about (1 + k) / sqrt(L) ~ 0.1: the mean over 20 samples is within 0.1
    est = []
    for seed in range(20):
        z = np.sort(genpareto.rvs(c=k, scale=1.0, size=200, random_state=seed))
        khat, sigma = R.gpdfit(z)
        assert sigma > 0
        est.append(khat)
    assert abs(np.mean(est) - k) < 0.1, (k, np.mean(est))


def test_equal_ll_gives_lppd_and_uniform_weights():
    for S in (1, 2, 5, 100, 4096):
        ll = np.full(S, -2.75)
        elpd, k, L, lw = R.psis(ll, return_lw=True)
        assert L == 0 and k == math.inf
        np.testing.assert_allclose(lw, np.full(S, -math.log(S)), rtol=0, atol=1e-12)
        s = R.summary(ll[:, None])
        assert abs(elpd - s["lppd"][0]) < 1e-12


def test_short_tail_has_infinite_k():
    # S = 20: M = ceil(min(4, 3 sqrt 20)) = 4, so L <= 4
    ll = np.random.RandomState(0).normal(-3, 0.5, 20)
    assert tail_size(20, 1.0) == 4
    elpd, k, L = R.psis(ll)
    assert L <= 4 and k == math.inf and np.isfinite(elpd)


def test_minus_inf_and_single_draw():
    ll = np.array([-1.0, -np.inf, -2.0, -1.5, -1.2, -0.9])
    assert R.psis(ll) == (-math.inf, math.inf, 0)
    s = R.summary(ll[:, None])
    assert s["var"][0] == math.inf and s["mean"][0] == -math.inf and np.isfinite(s["lppd"][0])
    s1 = R.summary(np.array([[-1.25]]))
    assert s1["var"][0] == 0 and s1["pareto_k"][0] == math.inf and s1["elpd_loo"][0] == -1.25


def test_tail_size_limits():
    assert tail_size(1, 1.0) == 0
    assert tail_size(65536, 1.0) == 768
    assert tail_size(65536, 0.3) > LOGLIK_MAX_TAIL
    assert tail_size(4096, 0.3) == 351


def _result(kind, pointwise):
    pointwise = np.asarray(pointwise, dtype=np.float64)
    e = float(pointwise.sum())
    return {"kind": kind, f"elpd_{kind}": e, f"p_{kind}": 1.0, "se": 0.0, f"elpd_{kind}_i": pointwise,
            "warning": False}


def test_compare_elpd_ranks_and_refuses_mismatches():
    rs = np.random.RandomState(0)
    a, b = rs.normal(-1.0, 0.3, 40), rs.normal(-1.1, 0.3, 40)
    out = compare_elpd({"worse": _result("loo", b), "better": _result("loo", a)})
    assert list(out) == ["better", "worse"]
    assert out["better"]["rank"] == 0 and out["better"]["elpd_diff"] == 0 and out["better"]["se_diff"] == 0
    assert abs(out["worse"]["elpd_diff"] - (a.sum() - b.sum())) < 1e-12
    assert abs(out["worse"]["se_diff"] - math.sqrt(40) * np.std(a - b, ddof=1)) < 1e-12
    with pytest.raises(ValueError):
        compare_elpd({"x": _result("loo", a), "y": _result("loo", b[:30])})
    with pytest.raises(ValueError):
        compare_elpd({"x": _result("loo", a), "y": _result("waic", b)})
    with pytest.raises(ValueError):
        compare_elpd({})


def _raises(m, exc, method, data, **kwargs):
    with pytest.raises(exc):
        getattr(m, method)(data, **kwargs)
    assert m._predict_ctx is None   # no device context was ever made


@pytest.mark.parametrize("kind", R.KINDS)
def test_argument_checks_run_on_the_host(kind):
    m = R.hand_model(kind, S=16)
    good = R.hand_data(m, n=6)
    for method in ("log_likelihood", "waic", "loo"):
        d = dict(good, home_team=["nope"] + list(good["home_team"][1:]))
        _raises(m, ValueError, method, d)
        d = dict(good, away_goals=list(good["away_goals"][:-1]))
        _raises(m, ValueError, method, d)
        d = dict(good, home_goals=[256] + list(good["home_goals"][1:]))
        _raises(m, ValueError, method, d)
        d = dict(good, away_goals=[-1] + list(good["away_goals"][1:]))
        _raises(m, ValueError, method, d)
        d = dict(good)
        d.pop("home_goals")
        _raises(m, ValueError, method, d)
    for r_eff in (0.0, -1.0, float("nan"), float("inf"), "1"):
        _raises(m, ValueError, "loo", good, r_eff=r_eff)
    if kind in ("neutral", "wc", "dynamic"):
        _raises(m, ValueError, "loo", dict(good, neutral_venue=[2] + list(good["neutral_venue"][1:])))
    if kind == "wc":
        _raises(m, ValueError, "waic", dict(good, home_conf=["nope"] + list(good["home_conf"][1:])))
        _raises(m, ValueError, "waic", dict(good, away_conf=list(good["away_conf"][:-1])))
    if kind == "dynamic":
        _raises(m, IndexError, "loo", dict(good, gameweek=[m.num_gameweeks] + list(good["gameweek"][1:])))
        _raises(m, IndexError, "log_likelihood", dict(good, gameweek=[-1] + list(good["gameweek"][1:])))


def test_tail_and_draw_limits_run_on_the_host():
    m = R.hand_model("basic", S=8192, T=4)
    d = R.hand_data(m, n=3)
    assert tail_size(8192, 0.01) > LOGLIK_MAX_TAIL
    _raises(m, ValueError, "loo", d, r_eff=0.01)
    big = R.hand_model("neutral", S=65537, T=2)
    d = R.hand_data(big, n=2)
    for method in ("log_likelihood", "waic", "loo"):
        _raises(big, ValueError, method, d)
