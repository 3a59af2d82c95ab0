"""The log-likelihood path on the device (csrc/dc_loglik.hip.h) against the numpy restatement
(tests/loglik_ref.py) for the five predictor classes, against the separately tested pointwise predict
kernel, and on determinism, edge cases and the host error of a tail beyond the limit."""
import numpy as np
import pytest

import loglik_ref as R
from bpl import DixonColesMatchPredictor, ExtendedDixonColesMatchPredictor, compare_elpd
from bpl._ffi import BPLHIP_EINVAL, BPLHIP_ESTATE, BplHipError, HipContext
from bpl.elpd import LOGLIK_MAX_TAIL, tail_size

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _close(got, ref, tol):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert not np.isnan(got).any()
    inf = ~np.isfinite(ref)
    np.testing.assert_array_equal(got[inf], ref[inf])
    err = np.abs(got[~inf] - ref[~inf]) / (1.0 + np.abs(ref[~inf]))
    assert err.size == 0 or err.max() <= tol, err.max()


def _check(m, d, r_eff=1.0):
    """The matrix within 1e-12 (1 + |ll|); lppd, mean, var within 1e-10; elpd_loo and k within 1e-9
    (DESIGN.md section 12); the tail set exactly (same L as the restatement's PSIS on the device's own ll)."""
    ll = m.log_likelihood(d)
    ref = R.ll_matrix(m, d)
    assert ll.shape == ref.shape
    _close(ll, ref, 1e-12)
    psis = tail_size(ll.shape[0], r_eff) <= LOGLIK_MAX_TAIL
    got = m._loglik_summary(d, psis=True, r_eff=r_eff) if psis else m._loglik_summary(d, psis=False)
    want = R.summary(ref, r_eff, psis_on=psis)
    for k in ("lppd", "mean", "var"):
        _close(got[k], want[k], 1e-10)
    if psis:
        _close(got["elpd_loo"], want["elpd_loo"], 1e-9)
        _close(got["pareto_k"], want["pareto_k"], 1e-9)
        own = R.summary(ll, r_eff)
        np.testing.assert_array_equal(got["tail_len"], own["tail_len"])
        np.testing.assert_array_equal(got["tail_len"], want["tail_len"])
    return ll, got


@pytest.mark.parametrize("kind", R.KINDS)
def test_all_classes_against_restatement(kind):
    m = R.hand_model(kind, S=257, T=8, seed=3)
    d = R.hand_data(m, n=70, seed=4)
    d["home_goals"][:5] = [0, 1, 0, 1, 70]
    d["away_goals"][:5] = [0, 0, 1, 1, 90]      # the four tau scorelines, and x, y > 63
    d["home_goals"][5] = 255
    for r_eff in (1.0, 0.3):
        _check(m, d, r_eff)
    w, lo = m.waic(d), m.loo(d)
    ref = R.ll_matrix(m, d)
    rw, rl = R.waic(ref), R.loo(ref)
    assert abs(w["elpd_waic"] - rw["elpd_waic"]) < 1e-8 and abs(w["p_waic"] - rw["p_waic"]) < 1e-8
    assert abs(lo["elpd_loo"] - rl["elpd_loo"]) < 1e-7 and abs(lo["p_loo"] - rl["p_loo"]) < 1e-7
    assert w["waic"] == -2 * w["elpd_waic"] and lo["looic"] == -2 * lo["elpd_loo"]


@pytest.mark.parametrize("S", [1, 2, 5, 63, 64, 65, 1000, 4096, 65536])
@pytest.mark.parametrize("kind", ["basic", "wc"])
def test_draw_counts(S, kind):
    m = R.hand_model(kind, S=S, T=6, seed=S)
    d = R.hand_data(m, n=8 if S == 65536 else 24, seed=5)
    for r_eff in (1.0, 0.3):
        if tail_size(S, r_eff) > LOGLIK_MAX_TAIL:
            with pytest.raises(ValueError):
                m.loo(d, r_eff=r_eff)
            # the library refuses it as well
            groups, _ = m._loglik_groups(d)
            _, device, kw = groups[0]
            with pytest.raises(BplHipError) as e:
                device().loglik_summary(**kw, r_eff=r_eff)
            assert e.value.code == BPLHIP_EINVAL
            continue
        _check(m, d, r_eff)


def test_duplicated_draws_tie_at_the_cutoff():
    base = R.hand_model("neutral", S=100, T=6, seed=8)
    for nm in ("attack", "defence", "home_attack", "away_attack", "home_defence", "away_defence"):
        setattr(base, nm, np.repeat(getattr(base, nm), 8, axis=0))
    base.corr_coef = np.repeat(base.corr_coef, 8)
    d = R.hand_data(base, n=40, seed=9)
    for r_eff in (1.0, 0.3):
        _, got = _check(base, d, r_eff)
        assert (got["tail_len"] % 8 == 0).all()   # whole groups of equal draws, never part of one


def test_clipped_tau_gives_minus_inf_not_nan():
    m = R.hand_model("basic", S=64, T=4, seed=2)
    m.corr_coef = np.where(np.arange(64) % 3 == 0, 5.0, 0.01)   # 1 - rho lh la < 0 and 1 - rho < 0 on some draws
    d = {"home_team": ["t00", "t01", "t02", "t03"], "away_team": ["t01", "t02", "t03", "t00"],
         "home_goals": [0, 1, 2, 1], "away_goals": [0, 1, 2, 0]}
    ll, got = _check(m, d)
    assert np.isneginf(ll[:, 1]).any() and np.isfinite(ll[:, 2]).all()
    assert got["elpd_loo"][1] == -np.inf and got["pareto_k"][1] == np.inf and got["var"][1] == np.inf
    w = m.waic(d)
    assert w["p_waic_i"][1] == np.inf and not np.isnan(w["elpd_waic_i"]).any()


@pytest.mark.parametrize("kind", R.KINDS)
def test_exp_lppd_is_predict_score_proba(kind):
    m = R.hand_model(kind, S=500, T=8, seed=11)
    d = R.hand_data(m, n=64, seed=12, max_goals=9)
    groups, _ = m._loglik_groups(d)
    for _, device, kw in groups:
        dev = device()
        p = dev.predict_score_proba(**kw)
        lppd = dev.loglik_summary(**kw, psis=False)["lppd"]
        np.testing.assert_allclose(np.exp(lppd), p, rtol=1e-12, atol=0)


def test_two_calls_are_bit_identical():
    m = R.hand_model("wc", S=4096, T=12, seed=13)
    d = R.hand_data(m, n=300, seed=14)
    a1, a2 = m.log_likelihood(d), m.log_likelihood(d)
    assert a1.tobytes() == a2.tobytes()
    s1, s2 = m._loglik_summary(d, True, 1.0), m._loglik_summary(d, True, 1.0)
    for k in s1:
        assert s1[k].tobytes() == s2[k].tobytes(), k


def test_dynamic_mixed_weeks_equal_per_week_calls():
    m = R.hand_model("dynamic", S=300, T=8, seed=15, G=4)
    d = R.hand_data(m, n=90, seed=16)
    full_ll, full = m.log_likelihood(d), m.loo(d)
    ll = np.empty_like(full_ll)
    elpd = np.empty(90)
    for g in range(4):
        pos = np.nonzero(np.asarray(d["gameweek"]) == g)[0]
        sub = {k: [v[i] for i in pos] for k, v in d.items()}
        ll[:, pos] = m.log_likelihood(sub)
        elpd[pos] = m.loo(sub)["elpd_loo_i"]
    assert ll.tobytes() == full_ll.tobytes()
    assert elpd.tobytes() == full["elpd_loo_i"].tobytes()


def test_context_errors():
    ctx = HipContext(0)
    h = np.array([0, 1], dtype=np.uint16)
    with pytest.raises(BplHipError) as e:
        ctx.loglik_summary(h, h[::-1], h, h)
    assert e.value.code == BPLHIP_ESTATE
    rs = np.random.RandomState(0)
    ctx.predict_set_posterior(rs.normal(0, 0.2, (10, 2)), rs.normal(0, 0.2, (10, 2)), rs.normal(0, 0.1, 10),
                              rs.uniform(-0.05, 0.05, 10))
    with pytest.raises(BplHipError) as e:
        ctx.loglik_matrix(h, h[::-1], h, h, neutral=[0, 1])
    assert e.value.code == BPLHIP_ESTATE
    with pytest.raises(BplHipError) as e:
        ctx.loglik_summary(h, h[::-1] + 5, h, h)
    assert e.value.code == BPLHIP_EINVAL
    for r_eff in (0.0, float("nan"), -2.0):
        with pytest.raises(BplHipError) as e:
            ctx.loglik_summary(h, h[::-1], h, h, r_eff=r_eff)
        assert e.value.code == BPLHIP_EINVAL
    assert ctx.loglik_summary(h, h[::-1], h, h, r_eff=float("nan"), psis=False)["lppd"].shape == (2,)
    ctx.close()


def test_compare_elpd_on_fitted_models(dummy_data):
    fits = {"dixon_coles": DixonColesMatchPredictor().fit(dummy_data, num_warmup=100, num_samples=200),
            "extended": ExtendedDixonColesMatchPredictor().fit(dummy_data, num_warmup=100, num_samples=200)}
    loos = {name: m.loo(dummy_data) for name, m in fits.items()}
    for name, r in loos.items():
        assert r["n"] == 380 and np.isfinite(r["elpd_loo"]) and np.isfinite(r["pareto_k"]).any()
        ref = R.loo(R.ll_matrix(fits[name], dummy_data))
        assert abs(r["elpd_loo"] - ref["elpd_loo"]) < 1e-6
    table = compare_elpd(loos)
    assert sorted(table) == sorted(loos) and [v["rank"] for v in table.values()] == [0, 1]
    assert all(v["elpd_diff"] >= 0 and np.isfinite(v["se_diff"]) for v in table.values())
    waics = {name: m.waic(dummy_data) for name, m in fits.items()}
    assert list(compare_elpd(waics))[0] in fits
