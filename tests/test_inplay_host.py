"""predict_in_play without a GPU (bpl/inplay.py, tests/inplay_ref.py): the derivation
itself (total probability over the states reproduces the kick-off market), the closed form of Z against the wide
grid, the kick-off limit, the weighted quantile rule against numpy's inverted CDF, the flag count of the GPU
tests' configurations, result keys, shapes and dtypes for each class through a stand-in context whose
`inplay_summary` is the restatement, and every argument check, made on the host before a device context is
touched."""
import numpy as np
import pytest

import inplay_ref as IR
import loglik_ref as LR
import markets_ref as MR
from bpl import markets as MK
from bpl.inplay import INPLAY_MAX_DRAWS
from fake_ctx import FakePredictCtx


def _hand_rates(S=4, seed=0):
    rs = np.random.RandomState(seed)
    return np.exp(rs.normal(0.3, 0.3, S)), np.exp(rs.normal(0.0, 0.3, S)), rs.uniform(-0.1, 0.1, S)


@pytest.mark.parametrize("t", [0.3, 0.9])
def test_total_probability_over_the_states_is_the_kick_off_market(t):
    """sum over (a, b) of P(state) E[W | state] = E[W]: with l = log(Pois Pois Z) and val = (sum W p~) / Z that is
    sum_{a, b <= 40} exp(l) val = sum W q of markets_ref, per draw.  It pins the derivation, not just the code."""
    G = 40
    lh, la, rho = _hand_rates()
    mk = {"home_win": MK.home_win(), "over_2.5": MK.total_over(2.5), "btts": MK.btts(), "score_1_1": MK.correct_score(1, 1),
          "score_0_0": MK.correct_score(0, 0), "goals_home": MK.goals("home"),
          "random": np.random.RandomState(1).uniform(-2.0, 2.0, (G + 1, G + 1))}
    W = MR.weights_of(mk, G)
    total = np.zeros((lh.size, len(mk)))
    for a in range(G + 1):
        for b in range(G + 1):
            val, lev, _, _ = IR.one_fixture(lh, la, rho, a, b, t, W, G)
            total += np.exp(lev)[:, None] * val
    want = MR.values_from_rates(lh[:, None], la[:, None], rho, W, G)[:, :, 0]
    err = np.abs(total - want).max()
    print(f"t={t}: total probability against the kick-off value {err:.3e}")
    assert err <= 1e-12


def test_wide_grid_Z_is_the_closed_form():
    lh, la, _ = _hand_rates(S=6, seed=2)
    for rho in (np.linspace(-0.1, 0.1, 6), np.array([5.0, 0.01, -3.0, 1.0, 0.3, -0.2])):   # unclipped; clipped cells
        for a in range(3):
            for b in range(3):
                for t in (0.0, 0.25, 0.5, 0.999):
                    if t == 0.0 and (a or b):
                        continue
                    _, _, Z, A = IR.one_fixture(lh, la, rho, a, b, t, np.ones((1, 4, 4)), 3)
                    Zc = IR.closed_form_Z(lh, la, rho, a, b, t)
                    assert (Z > 0.0).all() and (Zc > 0.0).all()
                    # both sides add a few dozen terms of size <= 1 + A, each a few roundings off
                    assert (np.abs(Z - Zc) <= 256 * IR.EPS * (1.0 + A)).all(), (a, b, t, np.abs(Z - Zc).max())
                    if a >= 2 or b >= 2:
                        assert (A == 0.0).all() and (Zc == 1.0).all()   # no tau cell is reachable
    # unclipped tau sums to one at kick-off: Z = 1 up to rounding
    _, _, Z, _ = IR.one_fixture(lh, la, np.linspace(-0.1, 0.1, 6), 0, 0, 0.0, np.ones((1, 4, 4)), 3)
    assert np.abs(Z - 1.0).max() <= 64 * IR.EPS


def test_kick_off_is_markets_ref_over_Z():
    G = 15
    lh, la, rho = _hand_rates(S=8, seed=3)
    rho[::2] = 4.0   # clipped draws: Z differs from 1 there
    W = MR.weights_of(MR.all_builders(), G)
    val, lev, Z, _ = IR.one_fixture(lh, la, rho, 0, 0, 0.0, W, G)
    want = MR.values_from_rates(lh[:, None], la[:, None], rho, W, G)[:, :, 0] / Z[:, None]
    assert np.abs(val - want).max() <= 1e-13 * 30
    np.testing.assert_array_equal(lev, np.log(Z))
    assert np.abs(Z[1::2] - 1.0).max() <= 64 * IR.EPS and np.abs(Z[::2] - 1.0).min() > 1e-3


@pytest.mark.parametrize("S", [1, 2, 64, 257, 1000])
def test_equal_weights_are_numpys_inverted_cdf(S):
    rs = np.random.RandomState(S)
    v = rs.normal(size=S)
    v[rs.randint(0, S, S // 4)] = v[0]   # ties
    qs = (0.0, 0.05, 0.3, 0.5, 0.95, 1.0) if S != 1000 else (0.0, 0.0513, 0.4999, 1.0)
    got, flag, _ = IR.weighted_quantiles(v, np.ones(S), qs)
    np.testing.assert_array_equal(got, np.quantile(v, qs, method="inverted_cdf"))
    # unequal weights against a replicated sample: integer weights w are w copies of the draw
    w = rs.randint(1, 5, S)
    got, _, _ = IR.weighted_quantiles(v, w.astype(np.float64), (0.0, 0.37, 0.81, 1.0))
    np.testing.assert_array_equal(got, np.quantile(np.repeat(v, w), (0.0, 0.37, 0.81, 1.0), method="inverted_cdf"))


@pytest.mark.parametrize("kind", ["basic", "dynamic"])
def test_the_gpu_configurations_flag_no_cell(kind):
    """tests/test_gpu_inplay.py: S = 257 with QS; random weights (reweight), equal weights and a log-weight row."""
    m = LR.hand_model(kind, S=257, T=8, seed=3)
    d = IR.with_states(LR.hand_data(m, n=40, seed=4), 15, seed=5)
    mk = {"home_win": MK.home_win(), "over_2.5": MK.total_over(2.5), "goals_home": MK.goals("home")}
    lw = np.random.RandomState(6).normal(0.0, 1.0, 257)
    for kwargs in ({}, {"reweight": False}, {"reweight": False, "log_weights": lw}, {"log_weights": lw}):
        ref = IR.predict_in_play(m, d, mk, 15, IR.QS, **kwargs)
        assert ref["flag"].sum() == 0, kwargs
        assert (ref["ess"] <= 257 * (1 + 1e-12)).all() and (ref["ess"] >= 1.0).all()
        if kwargs == {"reweight": False}:
            np.testing.assert_allclose(ref["ess"], 257.0, rtol=1e-13)
            np.testing.assert_array_equal(ref["quantile"],
                                          np.quantile(ref["draws"], IR.QS, axis=0, method="inverted_cdf").transpose(1, 0, 2))
        assert (IR.gates(ref)["draws"] < 1e-10).all() and (IR.gates(ref)["draw_log_evidence"] < 1e-12).all()


class FailCtx:
    """A device context that must never be touched."""

    def __getattr__(self, name):
        raise AssertionError(f"device call {name} before the host checks finished")


class InPlayCtx(FakePredictCtx):
    """FakePredictCtx plus `inplay_summary`, computed by the restatement from the uploaded posterior."""

    def __init__(self):
        self.calls = []

    def inplay_summary(self, home_idx, away_idx, home_goals, away_goals, elapsed, max_goals, weights, quantiles=(),
                       reweight=True, log_weights=None, neutral=None, conf=None, return_draws=False, workspace_bytes=0):
        h, a = np.asarray(home_idx, int), np.asarray(away_idx, int)
        self.calls.append(h.size)
        eh, ea = self._log_rates(h, a, neutral, conf)
        return IR.device_part(np.exp(eh), np.exp(ea), self.cc, home_goals, away_goals, elapsed, weights, quantiles,
                              max_goals, reweight, log_weights, return_draws)


@pytest.mark.parametrize("kind", LR.KINDS)
def test_result_keys_shapes_and_dtypes(kind):
    m = LR.hand_model(kind, S=9, T=6, seed=1)
    G = 5
    d = IR.with_states(LR.hand_data(m, n=23, seed=2), G, seed=3)
    m._predict_ctx = ctx = InPlayCtx()
    mk = MR.all_builders()
    mk["array"] = np.random.RandomState(3).uniform(-2, 2, (G + 1, G + 1))
    qs = (0.0, 0.1, 0.5, 1.0)
    r = m.predict_in_play(d, mk, max_goals=G, quantiles=qs, return_draws=True)
    K = len(mk)
    assert len(ctx.calls) == (len(np.unique(d["gameweek"])) if kind == "dynamic" else 1) and sum(ctx.calls) == 23
    assert set(r) == {"kind", "n", "markets", "quantiles", "mean", "sd", "quantile", "ess", "log_evidence", "draws",
                      "draw_log_evidence"}
    assert r["kind"] == "in_play" and r["n"] == 23 and r["markets"] == tuple(mk)
    assert r["quantiles"].dtype == np.float64 and r["quantiles"].tolist() == list(qs)
    for key, shape in (("mean", (K, 23)), ("sd", (K, 23)), ("quantile", (K, 4, 23)), ("ess", (23,)),
                       ("log_evidence", (23,)), ("draws", (9, K, 23)), ("draw_log_evidence", (9, 23))):
        assert r[key].shape == shape and r[key].dtype == np.float64, key
    ref = IR.predict_in_play(m, d, mk, G, qs)
    for key in ("mean", "sd", "quantile", "ess", "log_evidence", "draws", "draw_log_evidence"):
        np.testing.assert_allclose(r[key], ref[key], rtol=1e-12, atol=1e-14, err_msg=key)
    # the conditional law is a law: the three outcomes sum to the mass on the grid, at most 1
    i = {name: k for k, name in enumerate(mk)}
    total = r["draws"][:, i["home_win"]] + r["draws"][:, i["draw"]] + r["draws"][:, i["away_win"]]
    assert (total <= 1.0 + 1e-12).all() and (total > 0.5).all()
    # a side that leads cannot lose a clean sheet it has already lost: final goals >= current goals
    assert (r["mean"][i["goals_home"]] >= d["home_goals"] * (1 - 1e-9) * total.min()).all()
    # without return_draws there are none; Q = 0 is allowed; other weights, same values
    lw = np.random.RandomState(4).normal(size=9)
    r2 = m.predict_in_play(d, mk, max_goals=G, quantiles=(), reweight=False, log_weights=lw)
    assert "draws" not in r2 and "draw_log_evidence" not in r2 and r2["quantile"].shape == (K, 0, 23)
    ref2 = IR.predict_in_play(m, d, mk, G, (), reweight=False, log_weights=lw)
    np.testing.assert_allclose(r2["mean"], ref2["mean"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(r2["log_evidence"], r["log_evidence"], rtol=1e-12)   # from l alone
    assert np.abs(r2["mean"] - r["mean"]).max() > 1e-6


def _raises(m, data, markets, **kwargs):
    m._predict_ctx = FailCtx()
    with pytest.raises(ValueError):
        m.predict_in_play(data, markets, **kwargs)


@pytest.mark.parametrize("kind", LR.KINDS)
def test_argument_checks_run_on_the_host(kind):
    m = LR.hand_model(kind, S=16)
    good = IR.with_states(LR.hand_data(m, n=6), 15, seed=1)
    ok = {"home_win": MK.home_win()}
    m._predict_ctx = ctx = InPlayCtx()
    assert m.predict_in_play(good, ok)["mean"].shape == (1, 6)             # the good call is good
    _raises(m, {k: [] for k in good}, ok)                                  # no fixture
    for g in (-1, 64, 2.0, True, None, "15"):
        _raises(m, good, ok, max_goals=g)
    _raises(m, good, {})
    _raises(m, good, [MK.home_win()])
    _raises(m, good, {f"m{k}": MK.correct_score(k, 0) for k in range(65)})
    _raises(m, good, ok, quantiles=np.linspace(0, 1, 17))
    for q in (1.5, -0.1, np.nan, np.inf):
        _raises(m, good, ok, quantiles=(0.5, q))
    _raises(m, good, {"w": np.where(np.eye(16) > 0, np.nan, 1.0)})
    _raises(m, good, {"w": np.ones((16, 15))})
    # the state
    no_t = dict(good)
    no_t.pop("elapsed")
    _raises(m, no_t, ok)
    for key in ("home_goals", "away_goals"):
        d = dict(good)
        d.pop(key)
        _raises(m, d, ok)
        _raises(m, dict(good, **{key: [16] + list(good[key][1:])}), ok)                     # beyond max_goals = 15
        _raises(m, dict(good, **{key: [3] + list(good[key][1:])}), ok, max_goals=2)
        _raises(m, dict(good, **{key: [-1] + list(good[key][1:])}), ok)
        _raises(m, dict(good, **{key: [0.5] + list(good[key][1:])}), ok)
        _raises(m, dict(good, **{key: [1] + list(good[key][1:]), "elapsed": [0.0] + list(good["elapsed"][1:])}), ok)
    for bad in (1.0, -0.01, 1.5, np.nan, np.inf):
        _raises(m, dict(good, elapsed=[bad] + list(good["elapsed"][1:])), ok)
    _raises(m, dict(good, elapsed=list(good["elapsed"][1:])), ok)                           # one value short
    _raises(m, dict(good, elapsed=["a"] * 6), ok)
    # the log weights
    _raises(m, good, ok, log_weights=np.zeros(15))
    _raises(m, good, ok, log_weights=np.zeros((16, 1)))
    for bad in (np.nan, np.inf, -np.inf):
        _raises(m, good, ok, log_weights=np.where(np.arange(16) == 3, bad, 0.0))
    _raises(m, good, ok, log_weights="weights")
    # the fixtures, as predict_markets
    _raises(m, dict(good, home_team=["nope"] + list(good["home_team"][1:])), ok)
    if kind in ("neutral", "wc", "dynamic"):
        _raises(m, dict(good, neutral_venue=[2] + list(good["neutral_venue"][1:])), ok)
    if kind == "dynamic":
        d = dict(good)
        d.pop("gameweek")
        _raises(m, d, ok)
    # 0-0 at kick-off is a state
    m._predict_ctx = ctx   # (the one that holds the posterior)
    zero = dict(good, home_goals=[0] * 6, away_goals=[0] * 6, elapsed=[0.0] * 6)
    assert np.isfinite(m.predict_in_play(zero, ok)["mean"]).all()


def test_draw_limit_runs_on_the_host():
    big = LR.hand_model("neutral", S=INPLAY_MAX_DRAWS + 1, T=2)
    _raises(big, IR.with_states(LR.hand_data(big, n=2), 15, seed=1), {"draw": MK.draw()})
    assert INPLAY_MAX_DRAWS == 12288

