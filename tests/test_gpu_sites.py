"""The map from unconstrained draws to posterior sites against the float64 oracles:

  a. bplhip_constrain (team_params, the rho bounds over the unique pairs with the rate clip, clipped_sigmoid) against
     dc_oracle.potential_and_grad's constrained sites at SURVEY.md section 8c's points and at corr_coef_raw = +-40
     and +-100, where the clips of the sigmoid bind (the upper one from +40, the lower one only past -87);
  b. bplhip_constrain_dynamic (the [draws, G, T] walk, random_walk both ways) against dc_dynamic_oracle's;
  c. logp_grad's aux (rho, LB, UB) against constrain's corr_coef: the kernel and the host tell the same story;
  d. the error paths of the two entry points;
  e. one small fit per model class: every posterior attribute is the oracle's site at
     mcmc_info_["unconstrained"][i], `corr_coef[i]` the oracle's rho and `potential_energy[i]` the oracle's U at
     draw i -- which a wrong chain-major reshape or gather of the statistics would break.

Both sides of a. and b. are float64 and use the same formulas, so they differ by rounding only: the gates are 16 times
the largest relative error (max |got - want| / max |want| per site) measured over the listed points
(profiles/draw_stats/gpu_tests.txt), and anything above 1e-10 would be a difference of formula."""
import ctypes as C

import numpy as np
import pytest

import cases
import dc_dynamic_oracle as DO
import dc_neutral_oracle as NO
import dc_oracle as O

pytestmark = pytest.mark.gpu
LEAGUE_CASES = [(O.MODEL_BASIC, "dummy"), (O.MODEL_EXTENDED, "dummy"), (O.MODEL_EXTENDED, "dummy_covk_1"),
                (O.MODEL_EXTENDED, "dummy_cov"), (O.MODEL_EXTENDED, "ragged_777"), (O.MODEL_EXTENDED, "wide_4000_100")]
DYNAMIC_CASES = [(k, rw) for k in (0, 3) for rw in (True, False)]
MEASURED = {"constrain": 1.85e-15, "constrain_dynamic": 2.21e-16}   # the largest relative errors seen (dummy_cov; k = 3)
GATE = {k: 16.0 * v for k, v in MEASURED.items()}
RHO_PARITY = 1e-6     # tests/test_gpu_parity.py's gate on aux[0]
DYN_TABLES = ("attack", "defence", "home_attack", "away_attack", "home_defence", "away_defence")


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    scale = np.abs(want).max()
    return float(np.abs(got - want).max() / scale) if scale > 0 else float(np.abs(got).max())


def _bind_league(ctx, model, fx):
    K = fx.k if model == O.MODEL_EXTENDED else 0
    ctx.set_fixtures(model, fx.home_idx.astype(np.uint16), fx.away_idx.astype(np.uint16),
                     fx.home_goals.astype(np.uint8), fx.away_goals.astype(np.uint8), fx.n_teams,
                     covariates_std=O.standardise_covariates(fx.covariates) if K else None)
    assert ctx.dim == O.latent_dim(model, fx.n_teams, K)


_POINTS = {}


def _league_points(model, name):
    """(fixtures, [(label, z)], the oracle's aux per point): SURVEY.md 8c's points and corr_coef_raw = +-40."""
    if (model, name) not in _POINTS:
        fx = cases.fixtures(name)
        pts = cases.golden_points(model, fx)
        ic = cases._corr_slot(model, fx)
        for raw in (+40.0, -40.0, +100.0, -100.0):   # the last four points, in this order
            z = np.random.RandomState(77).uniform(-0.5, 0.5, pts[0][1].size)
            z[ic] = raw
            pts.append((f"raw{raw:+.0f}", z))
        aux = [O.potential_and_grad(model, fx, z)[2] for _, z in pts]
        assert aux[-2]["rho"] != aux[-1]["rho"]
        _POINTS[model, name] = (fx, pts, aux)
    return _POINTS[model, name]


# ---------------------------------------------------------------------------------------------- a. bplhip_constrain
@pytest.mark.parametrize("model,name", LEAGUE_CASES)
def test_constrain_matches_the_oracle_sites(hip_ctx, model, name):
    fx, pts, aux = _league_points(model, name)
    if name == "ragged_777":
        assert set(range(fx.n_teams)) - set(fx.home_idx.tolist())   # teams that never play at home
    _bind_league(hip_ctx, model, fx)
    got = hip_ctx.constrain(np.stack([z for _, z in pts]))
    s, T = len(pts), fx.n_teams
    assert got["attack"].shape == got["defence"].shape == (s, T) and got["corr_coef"].shape == (s,)
    assert got["home_advantage"].shape == ((s,) if model == O.MODEL_BASIC else (s, T))
    worst = 0.0
    for i, (label, _) in enumerate(pts):
        errs = {site: _rel(got[site][i], aux[i][site]) for site in ("attack", "defence", "home_advantage", "corr_coef")}
        worst = max(worst, *errs.values())
        assert max(errs.values()) <= GATE["constrain"], (name, label, errs)
        assert aux[i]["LB"] <= got["corr_coef"][i] <= aux[i]["UB"]
    # the sigmoid's clips, q = tiny / 1 - eps of float32 instead of 0 / 1.  The upper one binds from +40 on (1 - 4e-18
    # rounds to 1) and keeps rho a float32 epsilon of the bounds' width below UB; the lower one binds at -100 (at -40 q
    # is still 4e-18), and either way q (UB - LB) is absorbed by LB
    p40, m40, p100, m100 = (got["corr_coef"][i] for i in (-4, -3, -2, -1))
    lo, hi = aux[-1], aux[-2]
    assert m100 == lo["LB"] + O.SIG_LO * (lo["UB"] - lo["LB"]) == lo["LB"] == m40
    assert p40 == p100 < hi["UB"] and hi["UB"] - p100 > 1e-8 * (hi["UB"] - hi["LB"])
    print(f"constrain model {model} {name}: {s} points, largest relative error {worst:.3g} (gate {GATE['constrain']:.3g})")


# -------------------------------------------------------------------------------------- b. bplhip_constrain_dynamic
@pytest.mark.parametrize("k,random_walk", DYNAMIC_CASES)
def test_constrain_dynamic_matches_the_oracle_sites(hip_ctx, k, random_walk):
    fx = DO.small_recipe(k=k) if k else DO.small_recipe()
    cov = DO.standardise_covariates(fx.covariates) if k else None
    hip_ctx.set_fixtures_dynamic(fx.home_idx, fx.away_idx, fx.home_goals, fx.away_goals, fx.gameweek, fx.neutral,
                                 fx.n_teams, fx.n_gameweeks, covariates_std=cov, random_walk=random_walk)
    D = DO.latent_dim(fx.n_gameweeks, fx.n_teams, fx.k)
    z = np.stack([np.random.RandomState(s).uniform(-sc, sc, D) for s, sc in ((1, 0.3), (2, 1.0), (3, 2.5))] + [np.zeros(D)])
    got = hip_ctx.constrain_dynamic(z)
    worst = 0.0
    for i in range(z.shape[0]):
        aux = DO.potential_and_grad(fx, z[i], random_walk)[2]
        for nm in DYN_TABLES:
            assert got[nm].shape == (z.shape[0], fx.n_gameweeks, fx.n_teams)
            err = _rel(got[nm][i], aux[nm])
            worst = max(worst, err)
            assert err <= GATE["constrain_dynamic"], (k, random_walk, i, nm, err)
        if not random_walk:   # the reference as written leaves the walk at zero; the oracle and the library follow it
            assert not got["attack"][i].any() and not got["defence"][i].any()
            assert not np.asarray(aux["attack"]).any() and not np.asarray(aux["defence"]).any()
        elif i < 3:
            assert np.abs(np.diff(got["attack"][i], axis=0)).min() > 0   # a walk: every gameweek moves every team
    print(f"constrain_dynamic k={k} random_walk={random_walk}: largest relative error {worst:.3g} "
          f"(gate {GATE['constrain_dynamic']:.3g})")


# ----------------------------------------------------------------------------------- c. the kernel against the host
@pytest.mark.parametrize("model,name", LEAGUE_CASES)
def test_logp_grad_aux_tells_constrains_story(hip_ctx, model, name):
    import torch

    fx, pts, aux = _league_points(model, name)
    _bind_league(hip_ctx, model, fx)
    z = np.stack([p for _, p in pts])
    host = hip_ctx.constrain(z)["corr_coef"]
    _, _, dev = hip_ctx.logp_grad(torch.tensor(z, dtype=torch.float64, device=hip_ctx.device))
    dev = dev.cpu().numpy()
    ic = cases._corr_slot(model, fx)
    q = np.array([O._clipped_sigmoid(float(v))[0] for v in z[:, ic]])
    rebuilt = dev[:, 1] + q * (dev[:, 2] - dev[:, 1])
    print(f"aux vs constrain model {model} {name}: max |rho - corr_coef| {np.abs(dev[:, 0] - host).max():.3g}, "
          f"max |LB + q (UB - LB) - corr_coef| {np.abs(rebuilt - host).max():.3g}")
    assert np.abs(dev[:, 0] - host).max() <= RHO_PARITY
    assert np.abs(rebuilt - host).max() <= RHO_PARITY
    assert np.abs(dev[:, 1] - [a["LB"] for a in aux]).max() <= RHO_PARITY
    assert np.abs(dev[:, 2] - [a["UB"] for a in aux]).max() <= RHO_PARITY


# --------------------------------------------------------------------------------------------------- d. error paths
def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_constrain_error_paths(hip_ctx):
    from bpl._ffi import BPLHIP_ESTATE, BplHipError

    nf = NO.synthetic_neutral(600, 8)
    hip_ctx.set_fixtures_neutral(nf.home_idx, nf.away_idx, nf.home_goals, nf.away_goals, nf.neutral, nf.n_teams,
                                 weights=nf.weights.astype(np.float32))
    with pytest.raises(BplHipError) as e:
        hip_ctx.constrain(np.zeros((2, hip_ctx.dim)))
    assert e.value.code == BPLHIP_ESTATE
    hip_ctx.n_gameweeks = 1   # (HipContext.constrain_dynamic sizes its outputs by the bound dynamic model's)
    with pytest.raises(BplHipError) as e:   # and the dynamic entry point wants the dynamic model
        hip_ctx.constrain_dynamic(np.zeros((2, hip_ctx.dim)))
    assert e.value.code == BPLHIP_ESTATE

    df = DO.small_recipe()
    hip_ctx.set_fixtures_dynamic(df.home_idx, df.away_idx, df.home_goals, df.away_goals, df.gameweek, df.neutral,
                                 df.n_teams, df.n_gameweeks)
    with pytest.raises(BplHipError) as e:
        hip_ctx.constrain(np.zeros((2, hip_ctx.dim)))
    assert e.value.code == BPLHIP_ESTATE
    D = hip_ctx.dim
    assert all(v.shape == (0, df.n_gameweeks, df.n_teams) for v in hip_ctx.constrain_dynamic(np.empty((0, D))).values())
    # NULL outputs are skipped: only home_defence asked for
    z = np.random.RandomState(4).uniform(-0.5, 0.5, (3, D))
    hd = np.full((3, df.n_gameweeks, df.n_teams), np.nan)
    rc = hip_ctx._lib.bplhip_constrain_dynamic(hip_ctx._h, _ptr(z), 3, None, None, None, None, _ptr(hd), None)
    assert rc == 0 and np.array_equal(hd, hip_ctx.constrain_dynamic(z)["home_defence"])

    fx = cases.fixtures("dummy")
    _bind_league(hip_ctx, O.MODEL_BASIC, fx)
    hip_ctx.n_gameweeks = 1
    with pytest.raises(BplHipError) as e:
        hip_ctx.constrain_dynamic(np.zeros((2, hip_ctx.dim)))
    assert e.value.code == BPLHIP_ESTATE
    empty =hip_ctx.constrain(np.empty((0, hip_ctx.dim)))
    assert empty["attack"].shape == (0, 20) and empty["corr_coef"].shape == (0,)
    z = np.random.RandomState(5).uniform(-0.5, 0.5, (3, hip_ctx.dim))
    corr = np.full(3, np.nan)
    rc = hip_ctx._lib.bplhip_constrain(hip_ctx._h, _ptr(z), 3, None, None, None, _ptr(corr))
    assert rc == 0 and np.array_equal(corr, hip_ctx.constrain(z)["corr_coef"])
    att = np.full((3, 20), np.nan)
    rc = hip_ctx._lib.bplhip_constrain(hip_ctx._h, _ptr(z), 3, _ptr(att), None, None, None)
    assert rc == 0 and np.array_equal(att, hip_ctx.constrain(z)["attack"])


# ---------------------------------------------------------------------------------------------------- e. end to end
FIT = dict(num_warmup=30, num_samples=20)
TWO = {"mcmc_kwargs": {"num_chains": 2}}


def _assert_columns(tag, m, family, n_fixtures, at, sites):
    """Every draw of a fitted model against the oracle at mcmc_info_["unconstrained"][i]: `at(z)` returns (U, aux);
    `sites`: {attribute: aux key}.  corr_coef at the sampler's parity gate, the host-mapped sites at constrain's."""
    import draw_stats_cases as DS

    info = m.mcmc_info_
    z = info["unconstrained"]
    assert z.shape[0] == 20 * info["num_chains"] and info["potential_energy"].shape == (z.shape[0],)
    U, worst = np.empty(z.shape[0]), 0.0
    for i in range(z.shape[0]):
        U[i], aux = at(z[i])
        assert abs(info["potential_energy"][i] - U[i]) <= DS.u_gate(family, n_fixtures, U[i]), (tag, i)
        assert abs(m.corr_coef[i] - aux["rho"]) <= DS.RHO_GATE[family], (tag, i)
        for attr, key in sites.items():
            err = _rel(getattr(m, attr)[i], aux[key])
            worst = max(worst, err)
            assert err <= GATE["constrain"], (tag, i, attr, err)
    half = z.shape[0] // info["num_chains"]
    if info["num_chains"] == 2:   # the chains can be told apart, row by row
        gate = max(DS.u_gate(family, n_fixtures, u) for u in U)
        assert (np.abs(U[:half] - U[half:]) > DS.SENSITIVITY * gate).mean() >= DS.MIN_FRACTION
    fu, fr = DS.sensitivity(family, n_fixtures, U[:half], np.array([at(v)[1]["rho"] for v in z[:half]]))
    print(f"{tag}: {z.shape[0]} draws, sites within {worst:.3g}; consecutive pairs apart: U {fu:.2f}, rho {fr:.2f}")
    assert fu >= DS.MIN_FRACTION and fr >= DS.MIN_FRACTION


def _league_at(model, fx):
    def at(z):
        U, _, aux = O.potential_and_grad(model, fx, z)
        return U, aux
    return at


def test_fit_basic_end_to_end():
    from bpl import DixonColesMatchPredictor

    td = O.dummy_data_recipe()
    m = DixonColesMatchPredictor().fit(td, **FIT, **TWO)
    fx, _ = O.fixtures_from_training_data(td)
    _assert_columns("basic", m, "league", fx.n, _league_at(O.MODEL_BASIC, fx),
                    {"attack": "attack", "defence": "defence", "home_advantage": "home_advantage"})


def test_fit_extended_with_covariates_end_to_end():
    from bpl import ExtendedDixonColesMatchPredictor

    td = dict(O.dummy_data_recipe())
    cov = np.random.RandomState(0).normal(size=(20, 3))
    td["team_covariates"] = {str(t): cov[t] for t in range(20)}
    m = ExtendedDixonColesMatchPredictor().fit(td, **FIT, **TWO)
    fx, teams = O.fixtures_from_training_data(td)
    fx.covariates = np.array([cov[int(t)] for t in teams])
    _assert_columns("extended", m, "league", fx.n, _league_at(O.MODEL_EXTENDED, fx),
                    {"attack": "attack", "defence": "defence", "home_advantage": "home_advantage"})


_VENUE_SITES = {nm: nm for nm in DYN_TABLES}


def _neutral_at(fx):
    fx.weights = fx.weights.astype(np.float32).astype(np.float64)   # what the device holds

    def at(z):
        U, _, aux = NO.potential_and_grad(fx, z)
        return U, aux
    return at


def test_fit_neutral_end_to_end():
    from bpl import NeutralDixonColesMatchPredictor

    dd = NO.neutral_dummy_recipe()
    # (from the origin: from a uniform(-2, 2) start 30 warm-up transitions leave the first chain rejecting three
    # proposals in four, and a column of repeated values could not be seen shifted)
    m = NeutralDixonColesMatchPredictor().fit(dd, **FIT, **TWO, run_kwargs={"init_params": np.zeros(NO.latent_dim(20))})
    fx = NO.fixtures_from_data(dd)
    _assert_columns("neutral", m, "neutral", fx.n, _neutral_at(fx), _VENUE_SITES)


def test_fit_world_cup_end_to_end():
    from bpl import NeutralDixonColesMatchPredictorWC

    dd = NO.neutral_dummy_recipe()
    m = NeutralDixonColesMatchPredictorWC().fit(dd, **FIT, **TWO)   # (the default start: 0.89 of the pairs apart)
    fx = NO.fixtures_from_data_wc(dd)
    at = _neutral_at(fx)
    _assert_columns("world cup", m, "neutral", fx.n, at, _VENUE_SITES)
    sl = NO.site_slices(fx.n_teams, 0, fx.n_conf)["confederation_strength_decentered"]
    assert np.array_equal(m.confederation_strength, m.mcmc_info_["unconstrained"][:, sl])


@pytest.mark.parametrize("random_walk", [True, False])
def test_fit_dynamic_end_to_end(random_walk):
    import warnings

    from bpl.dynamic_dixon_coles import DynamicNeutralDixonColesMatchPredictor

    fx = DO.small_recipe()
    td = {"home_team": [f"t{i}" for i in fx.home_idx], "away_team": [f"t{i}" for i in fx.away_idx],
          "home_goals": fx.home_goals, "away_goals": fx.away_goals, "gameweek": fx.gameweek, "neutral_venue": fx.neutral}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = DynamicNeutralDixonColesMatchPredictor().fit(   # (the start tests/test_gpu_dynamic.py's fit takes)
            td, **FIT, **TWO, random_walk=random_walk,
            run_kwargs={"init_params": np.zeros(DO.latent_dim(fx.n_gameweeks, fx.n_teams))})

    def at(z):
        U, _, aux = DO.potential_and_grad(fx, z, random_walk)
        return U, aux
    _assert_columns(f"dynamic rw={random_walk}", m, "dynamic", fx.n, at, _VENUE_SITES)
