"""Power-scaling sensitivity without a GPU: the numpy restatement (tests/sensitivity_ref.py) against its anchor, its
symmetries and the method's sanity; the Python layer (bpl/sensitivity.py) on a stand-in backend that calls the
restatement -- the ValueErrors, the diagnosis strings, the threshold, format_summary, the class method; the
per-draw likelihood sums through a stand-in context; and, with the float64 oracle, that what `prior_sensitivity`
calls the prior does not depend on the data."""
import math

import numpy as np
import pytest

import bpl
import loglik_ref as LR
import sensitivity_ref as R
import sequential_ref as QR
from bpl import sensitivity as SN
from bpl.sequential import SEQ_MAX_BLOCKS
from fake_ctx import FakePredictCtx


@pytest.fixture
def ref_backend(monkeypatch):
    monkeypatch.setattr(SN, "_backend", R.backend)


# ---- the restatement
def test_the_four_draw_anchor():
    b, f, r = R.shift_parts([0.0, 1.0, 2.0, 4.0], [0.1, 0.2, 0.3, 0.4])
    assert abs(b - 3.85) <= 1e-12
    assert abs(f - 0.02817019145416) <= 1e-12 and abs(r - 0.02033736311853) <= 1e-12
    assert abs(R.cjs_sq([0.0, 1.0, 2.0, 4.0], [0.1, 0.2, 0.3, 0.4]) - 0.02817019145416) <= 1e-12
    # the order of the draws plays no part, the scale of the weights neither
    assert R.cjs_sq([4.0, 0.0, 2.0, 1.0], [4.0, 1.0, 3.0, 2.0]) == pytest.approx(0.02817019145416, abs=1e-12)


@pytest.mark.parametrize("S", [64, 1000, 12288])
def test_symmetries_of_the_restatement(S):
    v, l = R.gaussian_case(S, seed=S)
    x = v[:, 0]
    for ratio in R.power_ratios(l, l, 0.01)[:2]:
        w = np.exp(QR.psis_row(ratio)[0])
        base = R.cjs_sq(x, w)
        assert base > 0.0
        assert abs(R.cjs_sq(-x, w) - base) <= 1e-15
        assert abs(R.cjs_sq(3.0 * x + 7.0, w) - base) <= 1e-15


def test_uniform_weights_move_nothing():
    x = np.random.RandomState(2).normal(size=1000)
    assert R.cjs_sq(x, np.full(1000, 1.0 / 1000)) <= 4e-17
    assert math.isnan(R.cjs_sq(np.full(16, 1.5), np.ones(16))) and math.isnan(R.cjs_sq([0.0] * 7 + [np.inf], np.ones(8)))
    mean, sd = R.weighted_moments(np.full(16, 1.5), np.arange(1.0, 17.0))
    assert mean == 1.5 and sd == 0.0


@pytest.mark.parametrize("S", [1000, 4000])
def test_the_method_finds_the_column_the_likelihood_is_about(S):
    v, l = R.gaussian_case(S, seed=1)
    out = R.powerscale(v, np.zeros(S), l, 0.01)
    assert 0.05 <= out["likelihood"][0] <= 0.12, out["likelihood"]
    assert out["likelihood"][1] < 0.05
    assert np.all(out["prior"] <= 1e-6)     # a flat prior: constant ratios, uniform weights


# ---- the Python layer on the restatement
def test_weighted_shift_shapes_and_nan_rules(ref_backend):
    rs = np.random.RandomState(0)
    v = rs.normal(size=(40, 2, 3))
    v[:, 0, 1] = 4.0
    v[5, 1, 2] = np.nan
    ratios = rs.normal(size=(3, 40))
    out = SN.weighted_shift(v, ratios)
    assert set(out) == {"cjs", "cjs_sq", "mean", "sd", "log_weights", "pareto_k", "ess", "tail_len"}
    for nm in ("cjs", "cjs_sq", "mean", "sd"):
        assert out[nm].shape == (3, 2, 3), nm
    assert out["log_weights"].shape == (3, 40) and out["pareto_k"].shape == (3,) and out["tail_len"].dtype == np.int32
    nan = np.isnan(out["cjs_sq"])
    assert nan[:, 0, 1].all() and nan[:, 1, 2].all() and nan.sum() == 6
    assert np.array_equal(np.isnan(out["cjs"]), nan)
    assert np.allclose(out["mean"][:, 0, 1], 4.0, rtol=0, atol=1e-14) and np.all(out["sd"][:, 0, 1] <= 1e-14)
    ok = ~nan
    assert np.array_equal(out["cjs"][ok], np.sqrt(out["cjs_sq"][ok]))
    one = SN.weighted_shift(v, ratios[1])
    assert one["cjs_sq"].shape == (1, 2, 3) and np.array_equal(one["cjs_sq"][0], out["cjs_sq"][1], equal_nan=True)
    none = SN.weighted_shift(np.empty((40, 0)), ratios)
    assert none["cjs"].shape == (3, 0) and np.array_equal(none["pareto_k"], out["pareto_k"])


def test_argument_checks_run_before_any_backend_call(monkeypatch):
    def fail(*a, **k):
        raise AssertionError("backend call before the host checks finished")

    monkeypatch.setattr(SN, "_backend", fail)
    v, l = np.zeros((16, 2)), np.zeros(16)
    for bad in (dict(delta=0.0), dict(delta=-0.1), dict(delta=math.nan), dict(delta=True), dict(r_eff=0.0),
                dict(r_eff=None), dict(threshold=math.nan)):
        with pytest.raises(ValueError):
            bpl.powerscale_sensitivity(v, l, l, **bad)
    for lp, ll in ((np.zeros(15), l), (l, np.zeros(17)), (np.full(16, np.nan), l), (l, np.full(16, -np.inf)),
                   (np.zeros((16, 1)), l)):
        with pytest.raises(ValueError):
            bpl.powerscale_sensitivity(v, lp, ll)
    with pytest.raises(ValueError, match="at least 8"):
        bpl.powerscale_sensitivity(np.zeros((7, 2)), np.zeros(7), np.zeros(7))
    with pytest.raises(ValueError, match="at most 65536"):
        bpl.powerscale_sensitivity(np.zeros((65537, 1)), np.zeros(65537), np.zeros(65537))
    with pytest.raises(ValueError):
        bpl.powerscale_sensitivity(v, np.full(16, 1e308), l, delta=10.0)   # the ratio overflows
    for ratios in (np.zeros((9, 16)), np.zeros((0, 16)), np.zeros((2, 15)), np.full((1, 16), np.inf), np.zeros((1, 2, 16))):
        with pytest.raises(ValueError):
            SN.weighted_shift(v, ratios)
    with pytest.raises(ValueError):
        SN.weighted_shift(np.float64(1.0), np.zeros((1, 16)))


def test_powerscale_result_and_the_formula(ref_backend):
    v, l = R.gaussian_case(500, seed=3, Q_extra=2)
    lp = -np.abs(v[:, 1])
    out = bpl.powerscale_sensitivity(v.reshape(500, 3, 1), lp, l, delta=0.02)
    assert set(out) == {"prior", "likelihood", "diagnosis", "cjs", "mean", "sd", "pareto_k", "ess", "alpha", "delta",
                        "threshold", "warnings"}
    assert out["prior"].shape == (3, 1) and out["diagnosis"].shape == (3, 1) and out["cjs"].shape == (4, 3, 1)
    assert out["pareto_k"].shape == (4,) and out["ess"].shape == (4,)
    assert np.array_equal(out["alpha"], [1.0 / 1.02, 1.02]) and out["delta"] == 0.02 and out["threshold"] == 0.05
    ref = R.powerscale(v, lp, l, 0.02)
    assert np.array_equal(out["prior"].ravel(), ref["prior"]) and np.array_equal(out["likelihood"].ravel(), ref["likelihood"])
    assert np.array_equal(out["cjs"].reshape(4, 3), ref["cjs"])
    assert out["likelihood"][0, 0] >= 0.05 and out["prior"][1, 0] >= 0.05 and out["likelihood"][2, 0] < 0.05
    assert out["warnings"] == []
    # a heavy-tailed ratio row is reported, and its numbers still returned
    heavy = np.random.RandomState(5).standard_cauchy(500) * 40.0
    bad = bpl.powerscale_sensitivity(v, heavy, l, delta=0.5)
    assert bad["pareto_k"][:2].max() > 0.7 and len(bad["warnings"]) >= 1 and "pareto_k" in bad["warnings"][0]
    assert bad["warnings"][0].startswith("prior") and np.all(np.isfinite(bad["prior"]))


def test_diagnosis_strings_and_the_threshold():
    prior = np.array([0.05, 0.2, 0.049, np.nan, 0.06, 0.3])
    like = np.array([0.05, 0.01, 0.9, 0.9, np.nan, 0.3])
    assert SN.diagnose(prior, like).tolist() == ["prior-data conflict", "prior dominates", "", "", "prior dominates",
                                                  "prior-data conflict"]
    assert SN.diagnose(prior, like, threshold=0.25).tolist() == ["", "", "", "", "", "prior-data conflict"]
    assert SN.diagnose(np.zeros((2, 0)), np.zeros((2, 0))).shape == (2, 0)
    assert (SN.CONFLICT, SN.DOMINATES, SN.THRESHOLD) == ("prior-data conflict", "prior dominates", 0.05)


# ---- the class method
def _with_info(m, S, seed=0):
    rs = np.random.RandomState(seed)
    D = sum(int(np.prod(shape)) for _, shape in m._latent_sites())
    m.mcmc_info_ = {"num_chains": 2, "unconstrained": rs.normal(0, 0.5, (S, D)),
                    "potential_energy": rs.normal(300.0, 4.0, S)}
    return m


def test_prior_sensitivity_on_a_hand_built_model(ref_backend, monkeypatch):
    S, T = 64, 8
    m = _with_info(LR.hand_model("basic", S=S, T=T, seed=2), S)
    data = LR.hand_data(m, n=40, seed=1)
    ll = np.random.RandomState(4).normal(-120.0, 3.0, S)
    seen = []
    monkeypatch.setattr(m, "_loglik_draw_sums", lambda d, w: (seen.append((d, w)), ll)[1], raising=False)
    out = m.prior_sensitivity(data, delta=0.05)
    assert seen == [(data, None)]
    assert set(out) == {"attack", "defence", "home_advantage", "corr_coef", "pareto_k", "ess", "warnings", "log_prior",
                        "log_likelihood", "delta", "threshold"}
    for site, shape in (("attack", (T,)), ("defence", (T,)), ("home_advantage", ()), ("corr_coef", ())):
        assert set(out[site]) == {"prior", "likelihood", "diagnosis"}
        for nm in out[site]:
            assert out[site][nm].shape == shape, (site, nm)
    assert out["pareto_k"].shape == (4,) and out["delta"] == 0.05 and out["log_likelihood"] is ll
    lp = -m.mcmc_info_["potential_energy"] - ll - R.log_jacobian(m._latent_sites(), m.mcmc_info_["unconstrained"])
    assert np.array_equal(out["log_prior"], lp)
    ref = R.powerscale(np.column_stack([m.attack, m.defence, m.home_advantage, m.corr_coef]), lp, ll, 0.05)
    assert np.array_equal(out["attack"]["prior"], ref["prior"][:T])
    assert np.array_equal(out["corr_coef"]["likelihood"], ref["likelihood"][2 * T + 1])
    # the unconstrained space: the latent sites; explicit weights reach the likelihood sums
    w = np.linspace(0.5, 1.5, 40)
    un = m.prior_sensitivity(data, weights=w, space="unconstrained")
    assert un["attack_decentered"]["prior"].shape == (T,) and un["std_attack"]["prior"].shape == (1,)
    assert seen[-1][1] is w
    text = SN.format_summary(out, worst=3)
    lines = text.splitlines()
    assert lines[0].split()[:3] == ["quantity", "prior", "likelihood"] and len(lines) == 1 + 3 + 2 + len(out["warnings"])
    assert f"{2 * T + 2} quantities" in lines[4] and lines[5].startswith("pareto_k: prior- ")
    worst = max((float(np.max(out[s]["prior"])), s) for s in ("attack", "defence", "home_advantage", "corr_coef"))
    assert lines[1].startswith(worst[1])
    assert SN.format_summary(out, worst=0).splitlines()[1].endswith("at or above the threshold 0.05")


def test_prior_sensitivity_refuses_what_it_cannot_split(ref_backend, monkeypatch):
    S = 32
    m = LR.hand_model("extended", S=S, T=5, seed=2)
    for nm in ("rho", "mean_defence", "std_defence", "std_attack", "mean_home_advantage", "std_home_advantage"):
        setattr(m, nm, np.random.RandomState(1).uniform(0.1, 0.9, S))
    data = LR.hand_data(m, n=20, seed=1)
    monkeypatch.setattr(m, "_loglik_draw_sums", lambda d, w: np.full(S, -50.0) + np.arange(S) * 0.1, raising=False)
    with pytest.raises(ValueError, match="bpl.powerscale_sensitivity"):       # a hand-built posterior
        m.prior_sensitivity(data)
    _with_info(m, S)
    del m.mcmc_info_["potential_energy"]
    with pytest.raises(ValueError, match="bpl.powerscale_sensitivity"):
        m.prior_sensitivity(data)
    _with_info(m, S)
    assert m.prior_sensitivity(data)["attack"]["prior"].shape == (5,)
    np.random.seed(0)
    m.add_new_team("promoted")                                               # the latent sites no longer match
    with pytest.raises(ValueError, match="latent sites"):
        m.prior_sensitivity(data)
    m = _with_info(LR.hand_model("basic", S=S, T=5, seed=2), S)
    bad = np.full(S, -50.0)
    bad[3] = -np.inf
    monkeypatch.setattr(m, "_loglik_draw_sums", lambda d, w: bad, raising=False)
    with pytest.raises(ValueError, match="not finite"):
        m.prior_sensitivity(LR.hand_data(m, n=20, seed=1))


class _SumCtx(FakePredictCtx):
    """FakePredictCtx plus block_loglik, computed by the restatement from the uploaded posterior."""

    def __init__(self):
        self.blocks = []

    def block_loglik(self, home_idx, away_idx, home_goals, away_goals, block_idx, n_blocks, neutral=None, conf=None):
        assert np.asarray(block_idx).dtype == np.int32 and 1 <= n_blocks <= SEQ_MAX_BLOCKS
        self.blocks.append(n_blocks)
        eh, ea = self._log_rates(np.asarray(home_idx, int), np.asarray(away_idx, int), neutral, conf)
        ll = LR.ll_from_rates(np.exp(eh), np.exp(ea), home_goals, away_goals, self.cc)
        return QR.block_sums(ll, np.asarray(block_idx), n_blocks)


@pytest.mark.parametrize("kind", LR.KINDS)
def test_the_likelihood_sums_without_the_matrix(kind):
    m = QR.narrowed(LR.hand_model(kind, S=33, T=6, seed=1), 0.1)
    d = LR.hand_data(m, n=60, seed=2)
    m._predict_ctx = ctx = _SumCtx()
    ll = LR.ll_matrix(m, d)
    w = np.random.RandomState(3).choice([0.0, 0.25, 1.0, 2.5], 60)
    for weights, ref in ((None, ll.sum(axis=1)), (w, (ll * w).sum(axis=1)), (np.arange(60) / 7.0, (ll * (np.arange(60) / 7.0)).sum(axis=1))):
        got = m._loglik_draw_sums(d, weights)
        assert got.shape == (33,) and np.abs(got - ref).max() <= 1e-12 * (1.0 + np.abs(ref).max())
    assert ctx.blocks[0] == 2 and max(ctx.blocks) == 61     # one block per distinct weight, and the parking block
    for bad in (np.ones(59), np.full(60, np.nan), np.ones((60, 1))):
        with pytest.raises(ValueError):
            m._loglik_draw_sums(d, bad)


def test_the_fit_weights_hooks():
    d = {"home_goals": [1, 2, 0], "time_diff": np.array([0.0, 1.0, 2.0]), "game_weights": np.array([1.0, 2.0, 0.5])}
    assert bpl.DixonColesMatchPredictor()._fit_weights(d) is None
    m = bpl.ExtendedDixonColesMatchPredictor()
    assert m._fit_weights(d) is None
    m.epsilon, m.time_diff, m.rescale_weights = 0.5, d["time_diff"], True
    w = np.exp(-0.5 * d["time_diff"])
    assert np.array_equal(m._fit_weights(d), w * (3 / w.sum()))
    m = bpl.NeutralDixonColesMatchPredictor()
    assert np.array_equal(m._fit_weights(d), d["game_weights"])
    m.epsilon = 0.5
    assert np.array_equal(m._fit_weights(d), w * d["game_weights"])
    m = bpl.NeutralDixonColesMatchPredictorWC()
    m.epsilon, m.rescale_weights = 0.5, True
    ww = w * d["game_weights"]
    assert np.array_equal(m._fit_weights(d), 3 * ww / ww.sum())
    from bpl.dynamic_dixon_coles import DynamicNeutralDixonColesMatchPredictor

    assert DynamicNeutralDixonColesMatchPredictor()._fit_weights(d) is None


# ---- the decomposition: potential(z) + sum_i w_i ll_i(theta(z)) is -log prior(z) - logJ(z), whatever the data
@pytest.mark.parametrize("kind", ["basic", "extended"])
def test_the_prior_does_not_depend_on_the_data(oracle, kind):
    T = 8
    model = oracle.MODEL_BASIC if kind == "basic" else oracle.MODEL_EXTENDED
    m = LR.hand_model(kind, S=1, T=T, seed=0)
    rs = np.random.RandomState(21)
    for trial in range(3):
        z = rs.uniform(-0.7, 0.7, oracle.latent_dim(model, T))
        values = []
        for seed, n in ((1, 50), (2, 90)):
            data = LR.hand_data(m, n=n, seed=seed + 10 * trial)
            w = np.exp(-0.4 * rs.uniform(0.0, 3.0, n)) if kind == "extended" else None
            fx, teams = oracle.fixtures_from_training_data(data, weights=w)
            assert list(teams) == list(m.teams)
            U, _, aux = oracle.potential_and_grad(model, fx, z)
            m.attack, m.defence = aux["attack"][None, :], aux["defence"][None, :]
            m.home_advantage = np.atleast_1d(aux["home_advantage"]) if kind == "basic" else aux["home_advantage"][None, :]
            m.corr_coef = np.array([aux["corr_coef"]])
            ll = LR.ll_matrix(m, data)[0]
            assert np.all(np.isfinite(ll))
            values.append(U + float(np.sum(ll if w is None else w * ll)))
        assert abs(values[0] - values[1]) <= 1e-9 * (1.0 + abs(values[0])), (kind, values)
