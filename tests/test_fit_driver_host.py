"""The one chain driver (bpl/_mcmc.py:sample_chains) under all five model classes, and the shared
reductions of the scoreline grid (bpl/base.py), without a GPU: the fits run on the recording stub
context of tests/fake_ctx.py, whose draws are a fixed function of each chain's key and start point."""
import warnings

import numpy as np
import pytest

import bpl._ffi as ffi
from bpl import (DixonColesMatchPredictor, ExtendedDixonColesMatchPredictor, NeutralDixonColesMatchPredictor,
                 NeutralDixonColesMatchPredictorWC)
from bpl import _mcmc
from bpl._ffi import BPLHIP_EINVAL, BPLHIP_EUNSUPPORTED, BplHipError, prng_key, threefry_split
from bpl.base import draw_scores, draw_winners, goal_marginal, goals_wanted, outcome_from_grid, score_grid
from bpl.dynamic_dixon_coles import DynamicNeutralDixonColesMatchPredictor
from bpl.dynamic_dixon_coles import latent_sites as dynamic_sites
from bpl.neutral_dixon_coles import latent_sites as neutral_sites
from fake_ctx import FakePredictCtx, RecordingCtx

T, G, N = 5, 3, 30
RUN = {"num_warmup": 4, "num_samples": 6}
KEPT = 6
CLASSES = {"basic": DixonColesMatchPredictor, "extended": ExtendedDixonColesMatchPredictor,
           "neutral": NeutralDixonColesMatchPredictor, "wc": NeutralDixonColesMatchPredictorWC,
           "dynamic": DynamicNeutralDixonColesMatchPredictor}
DIM = {"basic": 2 * T + 5, "extended": 3 * T + 7, "neutral": 6 * T + 13, "wc": 6 * T + 2 + 13,
       "dynamic": 7 * G * T + 10 * G + 2}
KINDS = sorted(CLASSES)


def _data():
    rs = np.random.RandomState(1)
    h = rs.randint(0, T, N)
    a = (h + 1 + rs.randint(0, T - 1, N)) % T
    names = np.array([str(i) for i in range(T)])
    gw = np.sort(rs.randint(0, G, N))
    gw[-1] = G - 1
    conf = np.array(["A", "B"])[np.arange(T) % 2]
    return {"home_team": names[h], "away_team": names[a], "home_goals": rs.poisson(1.4, N),
            "away_goals": rs.poisson(1.1, N), "time_diff": rs.uniform(0, 3, N), "game_weights": rs.uniform(0.5, 2.0, N),
            "neutral_venue": rs.randint(0, 2, N), "gameweek": gw, "home_conf": conf[h], "away_conf": conf[a]}


@pytest.fixture
def stub(monkeypatch):
    monkeypatch.setattr(ffi, "HipContext", RecordingCtx)   # (the driver looks the class up per call)
    RecordingCtx.reset()
    yield RecordingCtx
    RecordingCtx.reset()


def _fit(kind, seed=42, **kwargs):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return CLASSES[kind]().fit(_data(), random_state=seed, **RUN, **kwargs)


def _calls(stub, name):
    return [payload for nm, payload in stub.log if nm == name]


def _names(stub):
    return [nm for nm, _ in stub.log]


def _expected_z(keys, starts, dim):
    cfg = ffi.default_nuts_cfg()
    cfg.num_samples, cfg.thinning = RUN["num_samples"], 1
    return np.concatenate([RecordingCtx.stub_draws(cfg, k, z0, dim)[0] for k, z0 in zip(keys, starts)])


# ---------------------------------------------------------------------------- keys, start points, order
@pytest.mark.parametrize("kind", KINDS)
def test_single_chain_runs_with_the_key_itself(stub, kind):
    m = _fit(kind, seed=7)
    (cfg, key, z0), = _calls(stub, "nuts_run")
    assert key == prng_key(7) and z0 is None and not _calls(stub, "nuts_run_chains")
    assert dict(cfg)["num_warmup"] == 4 and dict(cfg)["num_samples"] == 6 and dict(cfg)["thinning"] == 1
    assert np.array_equal(m.mcmc_info_["unconstrained"], _expected_z([key], [None], DIM[kind]))
    assert _names(stub)[0] == "create" and _names(stub)[-1] == "close"


@pytest.mark.parametrize("kind", KINDS)
def test_chain_c_gets_split_key_c_and_start_row_c_chain_major(stub, kind):
    n, dim = 3, DIM[kind]
    keys = threefry_split(prng_key(5), n)
    one_point = kind == "dynamic"   # (the dynamic class hands ONE point to every chain: a known gap)
    init = 0.01 * np.arange(dim if one_point else n * dim, dtype=np.float64)
    rows = [init] * n if one_point else list(init.reshape(n, dim))
    m = _fit(kind, seed=5, mcmc_kwargs={"num_chains": n, "chain_method": "sequential"}, run_kwargs={"init_params": init})
    runs = _calls(stub, "nuts_run")
    assert [r[1] for r in runs] == keys and not _calls(stub, "nuts_run_chains")
    assert all(np.array_equal(r[2], row) for r, row in zip(runs, rows))
    z = m.mcmc_info_["unconstrained"]
    assert z.shape == (n * KEPT, dim) and np.array_equal(z, _expected_z(keys, rows, dim))
    assert m.mcmc_info_["num_chains"] == n and m.mcmc_info_["accept_prob"].shape == (n * KEPT,)
    # per-chain scalars summed, per-draw statistics chain-major, as the league classes always had them
    cfg = ffi.default_nuts_cfg()
    cfg.num_samples, cfg.thinning = RUN["num_samples"], 1
    stats = [RecordingCtx.stub_draws(cfg, k, z0, dim)[1] for k, z0 in zip(keys, rows)]
    assert m.mcmc_info_["total_leapfrogs"] == sum(s["total_leapfrogs"] for s in stats)
    assert m.mcmc_info_["divergences"] == sum(s["total_divergences"] for s in stats)
    for nm in ("potential_energy", "accept_prob", "step_size", "num_steps", "diverging", "corr_coef"):
        assert np.array_equal(m.mcmc_info_[nm], np.concatenate([s[nm] for s in stats])), nm


# ---------------------------------------------------------------------------- lock step
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method", ["parallel", "vectorized", "sequential"])
def test_lock_step_is_tried_exactly_when_it_should(stub, kind, method):
    _fit(kind, mcmc_kwargs={"num_chains": 2, "chain_method": method})
    tried = len(_calls(stub, "nuts_run_chains"))
    assert tried == (1 if method != "sequential" and kind != "dynamic" else 0)
    assert len(_calls(stub, "nuts_run")) == (0 if tried else 2)
    if tried:
        (_, keys, z0), = _calls(stub, "nuts_run_chains")
        assert keys == threefry_split(prng_key(42), 2) and z0 is None


@pytest.mark.parametrize("kind", ["basic", "extended", "neutral", "wc"])
def test_lock_step_unsupported_falls_back_other_errors_propagate(stub, kind):
    stub.reset(lockstep_code=BPLHIP_EUNSUPPORTED)
    m = _fit(kind, mcmc_kwargs={"num_chains": 2})
    keys = threefry_split(prng_key(42), 2)
    assert len(_calls(stub, "nuts_run_chains")) == 1 and [r[1] for r in _calls(stub, "nuts_run")] == keys
    assert np.array_equal(m.mcmc_info_["unconstrained"], _expected_z(keys, [None, None], DIM[kind]))
    stub.reset(lockstep_code=BPLHIP_EINVAL)
    with pytest.raises(BplHipError):
        _fit(kind, mcmc_kwargs={"num_chains": 2})
    assert not _calls(stub, "nuts_run") and _names(stub)[-1] == "close"


# ---------------------------------------------------------------------------- the context is always closed
@pytest.mark.parametrize("kind", KINDS)
def test_context_closed_after_a_failure_anywhere(stub, kind):
    bind = {"basic": "set_fixtures", "extended": "set_fixtures", "neutral": "set_fixtures_neutral",
            "wc": "set_fixtures_neutral", "dynamic": "set_fixtures_dynamic"}[kind]
    finish = {"basic": "constrain", "extended": "constrain", "dynamic": "constrain_dynamic"}.get(kind)
    for where in (bind, "nuts_run", finish):
        if where is None:   # (the neutral classes have no device-side constrain step)
            continue
        stub.reset(fail={where: RuntimeError("boom in " + where)})
        with pytest.raises(RuntimeError, match="boom in " + where):
            _fit(kind)
        assert _names(stub).count("create") == 1 and _names(stub)[-1] == "close", where
    stub.reset()
    _fit(kind)
    assert _names(stub).count("close") == 1 and _names(stub)[-1] == "close"


# ---------------------------------------------------------------------------- constrained sites
def _transform(name, v):
    if name.startswith("std_"):
        return np.exp(v)
    if name in ("u", "corr_coef_raw"):
        return np.clip(1.0 / (1.0 + np.exp(-v)), np.finfo(np.float32).tiny, 1.0 - np.finfo(np.float32).eps)
    return v


def test_scalar_sites_are_exactly_the_size_one_sites_that_are_not_vectors():
    """With one covariate, one confederation and two teams the only other size-1 sites are the
    coefficient blocks and the confederation strengths, which stay [draws, 1]."""
    for sites in (_mcmc.latent_sites(ffi.MODEL_BASIC, 2, 0), _mcmc.latent_sites(ffi.MODEL_EXTENDED, 2, 1),
                  neutral_sites(2, 1, 1)):
        ones = {name for name, size in sites if size == 1}
        assert ones - _mcmc.SCALAR_SITES <= {"attack_coefficients", "defence_coefficients",
                                             "confederation_strength_decentered"}
        assert {name for name, _ in sites} & _mcmc.SCALAR_SITES <= ones


def test_constrain_sites_three_layouts():
    z = np.random.RandomState(0).normal(size=(4, 40))
    for sites in (_mcmc.latent_sites(ffi.MODEL_EXTENDED, 3, 2), neutral_sites(2, 1, 1), dynamic_sites(1, 2, 0)):
        dim = sum(int(np.prod(s)) for _, s in sites)
        out, o = _mcmc.constrain_sites(sites, z[:, :dim]), 0
        assert list(out) == [n for n, _ in sites]
        for name, shape in sites:
            size = int(np.prod(shape))
            want = _transform(name, z[:, o:o + size])
            o += size
            scalar = shape == () or (not isinstance(shape, tuple) and name in _mcmc.SCALAR_SITES)
            want = want[:, 0] if scalar else want.reshape((4,) + (shape if isinstance(shape, tuple) else (shape,)))
            assert out[name].shape == want.shape and np.array_equal(out[name], want), name


@pytest.mark.parametrize("kind", KINDS)
def test_fitted_sites_are_the_transforms_of_the_draws(stub, kind):
    m = _fit(kind, mcmc_kwargs={"num_chains": 2})
    z = m.mcmc_info_["unconstrained"]
    if kind in ("basic", "extended"):
        assert np.array_equal(m.attack, z[:, :T]) and np.array_equal(m.corr_coef, 0.05 * np.tanh(z[:, -1]))
        if kind == "extended":
            sites = _mcmc.constrain_sites(_mcmc.latent_sites(ffi.MODEL_EXTENDED, T, 0), z)
            assert np.array_equal(m.rho, 2.0 * sites["u"] - 1.0) and np.array_equal(m.std_attack, np.exp(z[:, 3 * T + 3]))
        return
    sites = dynamic_sites(G, T, 0) if kind == "dynamic" else neutral_sites(T, 0, 2 if kind == "wc" else 0)
    lat = _mcmc.constrain_sites(sites, z)
    for name in ("std_attack", "mean_home_attack", "standardised_defence", "u"):
        assert np.array_equal(getattr(m, name), lat[name]), name
    assert np.array_equal(m.rho, 2.0 * lat["u"] - 1.0)
    assert np.array_equal(m.corr_coef, m.mcmc_info_["corr_coef"]) and m.corr_coef.shape == (2 * KEPT,)
    if kind == "dynamic":
        assert m.attack.shape == (2 * KEPT, G, T) and np.array_equal(m.attack, z[:, :G * T].reshape(-1, G, T))
        assert m.u.shape == (2 * KEPT, G, T) and m.std_attack.shape == (2 * KEPT, G)
    else:
        assert np.array_equal(m.attack, lat["standardised_attack"] * lat["std_attack"][:, None])
        assert np.array_equal(m.home_attack, lat["mean_home_attack"][:, None]
                              + lat["std_home_attack"][:, None] * lat["home_attack_decentered"])
        if kind == "wc":
            assert np.array_equal(m.confederation_strength, lat["confederation_strength_decentered"])


def test_standardise_covariates():
    by_team = {"a": [1.0, 2.0], "b": [3.0, 6.0], "c": [5.0, 1.0]}
    table, mean, std = _mcmc.standardise_covariates(by_team, ["a", "b", "c"])
    raw = np.array([by_team[t] for t in "abc"])
    assert np.array_equal(mean, raw.mean(axis=0)) and np.array_equal(std, raw.std(axis=0))
    assert np.array_equal(table, (raw - mean) / std)
    assert _mcmc.standardise_covariates(None, ["a"]) == (None, None, None)
    assert _mcmc.standardise_covariates({}, ["a"]) == (None, None, None)
    with pytest.raises(ValueError, match="must contain all the teams"):
        _mcmc.standardise_covariates(by_team, ["a", "b"])


# ---------------------------------------------------------------------------- keyword and init_params rules
@pytest.mark.parametrize("kind", ["basic", "extended", "neutral", "wc"])
def test_shared_keyword_checks(stub, kind):
    for kwargs, exc, text in (
            ({"mcmc_kwargs": {"nonsense": 1}}, TypeError, "MCMC got unexpected keyword"),
            ({"run_kwargs": {"nonsense": 1}}, TypeError, "MCMC.run got unexpected keyword"),
            ({"mcmc_kwargs": {"num_chains": 0}}, ValueError, "num_chains and thinning must be >= 1"),
            ({"mcmc_kwargs": {"thinning": 0}}, ValueError, "num_chains and thinning must be >= 1"),
            ({"mcmc_kwargs": {"chain_method": "bogus"}}, ValueError, "Only supporting the following methods")):
        with pytest.raises(exc, match=text):
            _fit(kind, **kwargs)
        assert not stub.log   # (checked before a context exists)


@pytest.mark.parametrize("kind", ["basic", "extended"])
def test_league_classes_check_postprocess_fn_and_extra_fields(stub, kind):
    with pytest.raises(NotImplementedError, match="postprocess_fn"):
        _fit(kind, mcmc_kwargs={"postprocess_fn": abs})
    with pytest.raises(ValueError, match="extra_fields"):
        _fit(kind, run_kwargs={"extra_fields": ("energy",)})
    m = _fit(kind, run_kwargs={"extra_fields": ("num_steps",)})
    assert np.array_equal(m.mcmc_info_["extra_fields"]["num_steps"], m.mcmc_info_["num_steps"])


@pytest.mark.parametrize("kind", ["basic", "extended"])
def test_mean_accept_prob_is_the_running_mean_per_chain(stub, kind):
    """numpyro's `mean_accept_prob` is the mean of accept_prob over the post-warmup iterations so far, per chain
    (hmc.py: mean_accept_prob += (accept_prob - mean_accept_prob) / n) -- not the per-draw accept_prob it used to be
    an alias of.  Thinned runs have dropped the iterations in between and are refused, as `energy` is."""
    n = 3
    m = _fit(kind, mcmc_kwargs={"num_chains": n}, run_kwargs={"extra_fields": ("mean_accept_prob", "accept_prob")})
    acc = m.mcmc_info_["accept_prob"].reshape(n, KEPT)
    got = m.mcmc_info_["extra_fields"]["mean_accept_prob"].reshape(n, KEPT)
    assert np.array_equal(m.mcmc_info_["extra_fields"]["accept_prob"], m.mcmc_info_["accept_prob"])
    for c in range(n):
        mean = 0.0
        for i in range(KEPT):   # the recurrence of numpyro and of nuts.hpp ChainDriver::end
            mean += (acc[c, i] - mean) / (i + 1)
            assert abs(got[c, i] - mean) <= 4e-16
        assert got[c, 0] == acc[c, 0] and abs(got[c, -1] - acc[c].mean()) <= 4e-16
    assert np.abs(got - acc).max() > 1e-3   # (and it is not the per-draw column)
    with pytest.raises(ValueError, match="mean_accept_prob"):
        _fit(kind, mcmc_kwargs={"num_chains": 2, "thinning": 2}, run_kwargs={"extra_fields": ("mean_accept_prob",)})
    m = _fit(kind, mcmc_kwargs={"thinning": 2}, run_kwargs={"extra_fields": ("accept_prob",)})   # (still fine)
    assert m.mcmc_info_["extra_fields"]["accept_prob"].shape == (KEPT // 2,)


@pytest.mark.parametrize("kind", KINDS)
def test_final_step_sizes_are_kept_beside_the_per_draw_ones(stub, kind):
    n = 3
    keys = threefry_split(prng_key(42), n)
    m = _fit(kind, mcmc_kwargs={"num_chains": n})
    info = m.mcmc_info_
    assert np.array_equal(info["final_step_size"], [0.25 + 1e-3 * (k[1] % 7) for k in keys])
    assert len(set(info["final_step_size"].tolist())) > 1
    assert np.array_equal(info["step_size"], np.full(n * KEPT, 0.25))   # per draw, chain-major, as before


@pytest.mark.parametrize("kind", ["neutral", "wc"])
def test_neutral_classes_ignore_postprocess_fn_and_extra_fields(stub, kind):
    """A known gap: accepted and dropped, as before the shared driver."""
    m = _fit(kind, mcmc_kwargs={"postprocess_fn": abs}, run_kwargs={"extra_fields": ("energy",)})
    assert "extra_fields" not in m.mcmc_info_ and m.attack.shape == (KEPT, T)


def test_dynamic_class_checks_no_keyword(stub):
    """A known gap: nothing is checked, chain_method is not even read."""
    m = _fit("dynamic", mcmc_kwargs={"chain_method": "bogus", "nonsense": 1, "postprocess_fn": abs},
             run_kwargs={"nonsense": 2, "extra_fields": ("energy",)})
    assert m.attack.shape == (KEPT, G, T) and len(_calls(stub, "nuts_run")) == 1


@pytest.mark.parametrize("kind", ["basic", "extended"])
def test_league_init_params_rules(stub, kind):
    dim = DIM[kind]
    model = ffi.MODEL_BASIC if kind == "basic" else ffi.MODEL_EXTENDED
    as_dict = {nm: np.full(sz, 0.01 * i) for i, (nm, sz) in enumerate(_mcmc.latent_sites(model, T, 0))}
    flat = np.concatenate([as_dict[nm] for nm, _ in _mcmc.latent_sites(model, T, 0)])
    _fit(kind, mcmc_kwargs={"num_chains": 2}, run_kwargs={"init_params": as_dict})   # a dict: one point, every chain
    (_, _, z0), = _calls(stub, "nuts_run_chains")
    assert np.array_equal(z0, np.stack([flat, flat]))
    with pytest.raises(KeyError, match="missing site"):
        _fit(kind, run_kwargs={"init_params": {k: v for k, v in as_dict.items() if k != "mean_defence"}})
    with pytest.raises(ValueError, match=r"init_params\['mean_defence'\] has size 2, expected 1"):
        _fit(kind, run_kwargs={"init_params": {**as_dict, "mean_defence": np.zeros(2)}})
    stub.reset()
    _fit(kind, mcmc_kwargs={"num_chains": 2}, run_kwargs={"init_params": np.arange(2.0 * dim)})   # num_chains * D values
    (_, _, z0), = _calls(stub, "nuts_run_chains")
    assert np.array_equal(z0, np.arange(2.0 * dim).reshape(2, dim))
    with pytest.raises(ValueError, match=rf"init_params must have shape \(2, {dim}\)"):   # (the context's own check)
        _fit(kind, mcmc_kwargs={"num_chains": 2}, run_kwargs={"init_params": np.zeros(dim + 1)})


@pytest.mark.parametrize("kind", ["neutral", "wc"])
def test_neutral_init_params_rules(stub, kind):
    dim = DIM[kind]
    sites = neutral_sites(T, 0, 2 if kind == "wc" else 0)
    _fit(kind, mcmc_kwargs={"num_chains": 2}, run_kwargs={"init_params": np.arange(1.0 * dim)})
    (_, _, z0), = _calls(stub, "nuts_run_chains")
    assert np.array_equal(z0, np.stack([np.arange(1.0 * dim)] * 2))
    with pytest.raises(ValueError, match=f"init_params must have {dim} or 2x{dim} entries, got {dim + 1}"):
        _fit(kind, mcmc_kwargs={"num_chains": 2}, run_kwargs={"init_params": np.zeros(dim + 1)})
    # a dict is concatenated unchecked (a known gap): a site of the wrong size passes when the total fits
    as_dict = {nm: np.zeros(sz) for nm, sz in sites}
    as_dict["mean_defence"], as_dict["u"] = np.zeros(2), np.zeros(0)
    stub.reset()
    _fit(kind, run_kwargs={"init_params": as_dict})
    assert _calls(stub, "nuts_run")[0][2].shape == (dim,)


def test_dynamic_init_params_rules(stub):
    dim = DIM["dynamic"]
    sites = dynamic_sites(G, T, 0)
    as_dict = {nm: np.full(int(np.prod(shape)), 0.5) for nm, shape in sites}   # concatenated unchecked
    _fit("dynamic", mcmc_kwargs={"num_chains": 2}, run_kwargs={"init_params": as_dict})
    assert all(np.array_equal(r[2], np.full(dim, 0.5)) for r in _calls(stub, "nuts_run")) and len(_calls(stub, "nuts_run")) == 2
    with pytest.raises(ValueError, match=rf"init_params must have shape \({dim},\)"):   # one point only (a known gap)
        _fit("dynamic", mcmc_kwargs={"num_chains": 2}, run_kwargs={"init_params": np.zeros((2, dim))})


# ---------------------------------------------------------------------------- the reductions, by hand
GRID = np.array([[[0.10, 0.05, 0.02],
                  [0.20, 0.15, 0.03],
                  [0.25, 0.12, 0.08]]])   # rows: home goals 0..2, columns: away goals 0..2; sums to 1


def test_outcome_from_grid_by_hand():
    out = outcome_from_grid(GRID)
    assert list(out) == ["home_win", "draw", "away_win"]
    assert out["home_win"][0] == pytest.approx(0.20 + 0.25 + 0.12, abs=1e-15)
    assert out["draw"][0] == pytest.approx(0.10 + 0.15 + 0.08, abs=1e-15)
    assert out["away_win"][0] == pytest.approx(0.05 + 0.02 + 0.03, abs=1e-15)
    ko = outcome_from_grid(GRID, knockout=True)
    assert list(ko) == ["home_win", "away_win"]
    assert ko["home_win"][0] == pytest.approx(0.57 / 0.67, abs=1e-15) and ko["away_win"][0] == pytest.approx(0.10 / 0.67, abs=1e-15)


def test_goal_marginal_by_hand():
    wanted = goals_wanted([0, 1, 2])
    assert wanted.dtype == np.int64 and goals_wanted(2).shape == (1,)
    home = goal_marginal(GRID[0], wanted, 2, own_axis=0)       # row sums: the home side's goals
    away = goal_marginal(GRID[0], wanted, 2, own_axis=1)       # column sums
    assert home == pytest.approx([0.17, 0.38, 0.45], abs=1e-15) and away == pytest.approx([0.55, 0.32, 0.13], abs=1e-15)
    assert goal_marginal(GRID[0], goals_wanted(2), 1, own_axis=0) == pytest.approx([0.25 + 0.12], abs=1e-15)   # other side 0..1 only
    with pytest.raises(ValueError, match="n must be >= 0"):
        goals_wanted(-1)


def test_marginal_grid_is_as_deep_as_the_largest_n_asked_for():
    class DepthCtx(FakePredictCtx):
        depths = []

        def predict_score_grid(self, h, a, max_goals, neutral=None, conf=None):
            self.depths.append(max_goals)
            return super().predict_score_grid(h, a, max_goals, neutral, conf)

    rs = np.random.RandomState(0)
    m = DixonColesMatchPredictor()
    m.teams, m._teams_dict = np.array(["a", "b"]), {"a": 0, "b": 1}
    m.attack, m.defence = rs.normal(0, 0.1, (8, 2)), rs.normal(0, 0.1, (8, 2))
    m.home_advantage, m.corr_coef = rs.normal(0.2, 0.05, 8), rs.uniform(-0.05, 0.03, 8)
    m._predict_ctx = DepthCtx()
    deep = m.predict_score_n_proba(18, "a", "b", max_goals=5)
    m.predict_concede_n_proba([0, 3], "a", "b", home=False, max_goals=5)
    assert DepthCtx.depths == [18, 5]
    assert deep[0] == pytest.approx(m._predict_ctx.predict_score_grid([0], [1], 18)[0][18, :6].sum(), abs=1e-18)
    with pytest.raises(KeyError):   # (the team lookup comes before the depth, as it always did)
        m.predict_score_n_proba([], "nobody", "b")


def test_draws_from_a_certain_grid():
    sure = np.zeros((2, 3, 3))
    sure[0, 2, 1] = sure[1, 0, 2] = 1.0
    s = draw_scores(sure, 2, 5, random_state=3)
    assert s["home_score"].dtype == np.uint8 and s["home_score"].shape == (2, 5)
    assert (s["home_score"] == [[2], [0]]).all() and (s["away_score"] == [[1], [2]]).all()
    teams = np.array(["x", "y", "z"])
    w = draw_winners(outcome_from_grid(sure), np.array([0, 1]), np.array([2, 0]), teams, 4, random_state=3)
    assert (w == [["x"], ["x"]]).all()
    level = np.zeros((1, 3, 3))
    level[0, 1, 1] = 1.0
    assert (draw_winners(outcome_from_grid(level), [0], [2], teams, 4, random_state=1) == "Draw").all()
    half = np.zeros((1, 3, 3))
    half[0, 1, 0] = half[0, 0, 1] = 0.25
    half[0, 1, 1] = 0.5
    assert set(draw_winners(outcome_from_grid(half, knockout=True), [0], [2], teams, 200, random_state=1).ravel()) == {"x", "z"}


def test_score_grid_checks_depth_before_the_device_and_goes_pointwise_past_63():
    def no_device():
        raise AssertionError("the device must not be touched")

    with pytest.raises(ValueError, match="max_goals must be >= 0"):
        score_grid(no_device, np.array([0]), np.array([1]), -1)
    ctx = FakePredictCtx()
    rs = np.random.RandomState(0)
    ctx.predict_set_posterior(rs.normal(0, 0.1, (8, 3)), rs.normal(0, 0.1, (8, 3)), rs.normal(0.2, 0.05, 8), rs.uniform(-0.05, 0.03, 8))
    h, a = np.array([0, 1]), np.array([2, 0])
    deep, direct = score_grid(lambda: ctx, h, a, 64), ctx.predict_score_grid(h, a, 64)
    assert deep.shape == (2, 65, 65) and np.allclose(deep, direct, rtol=0, atol=1e-15)


# ---------------------------------------------------------------------------- league against neutral
def test_league_and_neutral_classes_agree_without_venue_effects():
    rs = np.random.RandomState(3)
    S, teams = 50, np.array([str(i) for i in range(T)])
    league, neutral = DixonColesMatchPredictor(), NeutralDixonColesMatchPredictor()
    for m in (league, neutral):
        m.teams, m._teams_dict = teams, {t: i for i, t in enumerate(teams)}
        m._predict_ctx = FakePredictCtx()
    league.attack = neutral.attack = rs.normal(0, 0.2, (S, T))
    league.defence = neutral.defence = rs.normal(0, 0.2, (S, T))
    league.corr_coef = neutral.corr_coef = rs.uniform(-0.05, 0.03, S)
    league.home_advantage = np.zeros(S)
    for nm in ("home_attack", "away_attack", "home_defence", "away_defence"):
        setattr(neutral, nm, np.zeros((S, T)))
    H, A, nv = ["0", "1", "2"], ["3", "4", "0"], [0, 0, 0]
    tol = {"rtol": 0, "atol": 1e-12}
    assert np.allclose(league.predict_score_proba(H, A, [1, 0, 2], [0, 0, 1]),
                       neutral.predict_score_proba(H, A, [1, 0, 2], [0, 0, 1], nv), **tol)
    for depth in (4, 15, 64):
        gl, gn = league.predict_score_grid_proba(H[:1], A[:1], depth), neutral.predict_score_grid_proba(H[:1], A[:1], nv[:1], depth)
        assert all(np.allclose(x, y, **tol) for x, y in zip(gl, gn))
    ol, on = league.predict_outcome_proba(H, A), neutral.predict_outcome_proba(H, A, nv)
    assert list(ol) == list(on) and all(np.allclose(ol[k], on[k], **tol) for k in ol)
    n = np.arange(7)
    for home in (True, False):
        assert np.allclose(league.predict_score_n_proba(n, "0", "1", home=home),
                           neutral.predict_score_n_proba(n, "0", "1", home=home), **tol)
        assert np.allclose(league.predict_concede_n_proba(n, "0", "1", home=home, max_goals=4),
                           neutral.predict_concede_n_proba(n, "0", "1", home=home, max_goals=4), **tol)
    sl, sn = league.sample_score(H, A, 25, random_state=8), neutral.sample_score(H, A, nv, 25, random_state=8)
    assert all(np.array_equal(sl[k], sn[k]) for k in ("home_score", "away_score"))
    assert np.array_equal(league.sample_outcome(H, A, 25, random_state=8),
                          neutral.sample_outcome(H, A, nv, num_samples=25, random_state=8))
