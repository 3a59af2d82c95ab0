"""The host's maps from unconstrained draws to posterior sites (bpl/_mcmc.py: constrain_sites, neutral_sites,
dynamic_sites) against the float64 oracles' own constrained sites, without a GPU.  Both sides are numpy float64 with
the same formulas: they agree to a few roundings (1e-13 relative; the matrix products of the covariate means and the
cumulative sums are the only places the order of additions may differ)."""
import numpy as np
import pytest

import dc_dynamic_oracle as DO
import dc_neutral_oracle as NO
import dc_oracle as O
from bpl import _mcmc
from bpl._ffi import MODEL_BASIC, MODEL_EXTENDED
from bpl.dynamic_dixon_coles import latent_sites as dynamic_latent_sites
from bpl.neutral_dixon_coles import latent_sites as neutral_latent_sites

RTOL = 1e-13


def _close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.abs(got - want).max() <= RTOL * max(np.abs(want).max(), 1e-300)


# ------------------------------------------------------------------------------------------------ constrain_sites
def _expected_site(name, raw):
    if name.startswith("std_"):
        return np.exp(raw)
    if name in ("corr_coef_raw", "u"):
        return np.array([O._clipped_sigmoid(float(v))[0] for v in raw.reshape(-1)]).reshape(raw.shape)
    return raw


@pytest.mark.parametrize("layout", ["basic", "extended", "extended_k", "neutral", "wc", "dynamic", "dynamic_k"])
def test_constrain_sites_site_by_site(layout):
    T, G = 6, 4
    sites = {"basic": lambda: _mcmc.latent_sites(MODEL_BASIC, T, 0), "extended": lambda: _mcmc.latent_sites(MODEL_EXTENDED, T, 0),
             "extended_k": lambda: _mcmc.latent_sites(MODEL_EXTENDED, T, 3), "neutral": lambda: neutral_latent_sites(T, 2, 0),
             "wc": lambda: neutral_latent_sites(T, 0, 3), "dynamic": lambda: dynamic_latent_sites(G, T, 0),
             "dynamic_k": lambda: dynamic_latent_sites(G, T, 2)}[layout]()
    D = sum(int(np.prod(shape)) for _, shape in sites)
    S = 7
    z = np.random.RandomState(3).uniform(-3, 3, (S, D))
    z[0], z[1], z[2] = 0.0, 100.0, -100.0        # rows where the sigmoid saturates: both clips bind
    z[3] = np.random.RandomState(4).uniform(-120, 120, D)
    z[4], z[5] = 40.0, -40.0                     # the upper clip binds (1 - 4e-18 rounds to 1), the lower does not
    out = _mcmc.constrain_sites(sites, z)
    assert list(out) == [name for name, _ in sites]
    o = 0
    for name, shape in sites:
        size = int(np.prod(shape))
        raw = z[:, o:o + size]
        o += size
        if isinstance(shape, tuple):
            want_shape = (S,) + shape
        else:
            want_shape = (S,) if name in _mcmc.SCALAR_SITES else (S, size)
        assert out[name].shape == want_shape, (name, out[name].shape)
        want = _expected_site(name, raw)   # (math.exp against np.exp, and two forms of the sigmoid: a few ulps)
        assert (np.abs(out[name].reshape(S, size) - want) <= 4 * np.finfo(np.float64).eps * np.abs(want)).all(), name
        if name in ("corr_coef_raw", "u"):
            v = out[name].reshape(S, size)
            assert (v[1] == O.SIG_HI).all() and (v[2] == O.SIG_LO).all() and (v[0] == 0.5).all()
            assert (v[4] == O.SIG_HI).all() and ((v[5] > O.SIG_LO) & (v[5] < 1e-17)).all()
            assert ((v > 0) & (v < 1)).all()
        elif not name.startswith("std_"):
            assert np.array_equal(out[name].reshape(S, size), raw), name
    assert o == D


def test_scalar_sites_of_the_league_and_neutral_layouts_come_back_as_vectors():
    for sites in (_mcmc.latent_sites(MODEL_BASIC, 5, 0), _mcmc.latent_sites(MODEL_EXTENDED, 5, 2), neutral_latent_sites(5, 2, 3)):
        D = sum(n for _, n in sites)
        out = _mcmc.constrain_sites(sites, np.zeros((4, D)))
        for name, n in sites:
            assert out[name].shape == ((4,) if n == 1 and name in _mcmc.SCALAR_SITES else (4, n)), name
            assert n > 1 or name in _mcmc.SCALAR_SITES, name   # (no size-1 site is left a column by accident)


# -------------------------------------------------------------------------------------------------- neutral_sites
@pytest.mark.parametrize("k,n_conf", [(0, 0), (2, 0), (0, 3), (2, 3)])
def test_neutral_sites_match_the_oracle(k, n_conf):
    fx = NO.synthetic_neutral(600, 8, k=k, n_conf=n_conf)
    T = fx.n_teams
    sites = neutral_latent_sites(T, k, n_conf)
    assert [(n, s) for n, s in sites] == NO.site_list(T, k, n_conf)
    D = NO.latent_dim(T, k, n_conf)
    z = np.stack([np.random.RandomState(s).uniform(-sc, sc, D) for s, sc in ((1, 0.3), (2, 1.0), (3, 2.0))])
    cov_std = NO.standardise_covariates(fx.covariates) if k else None
    out = _mcmc.neutral_sites(sites, z, cov_std, n_conf)
    sl = NO.site_slices(T, k, n_conf)
    for i in range(z.shape[0]):
        aux = NO.potential_and_grad(fx, z[i])[2]
        for nm in ("attack", "defence", "home_attack", "away_attack", "home_defence", "away_defence"):
            assert out[nm].shape == (z.shape[0], T) and _close(out[nm][i], aux[nm]), (nm, i)
        u = O._clipped_sigmoid(float(z[i, sl["u"]][0]))[0]
        assert abs(out["u"][i] - u) <= 4e-16 and out["rho"][i] == 2.0 * out["u"][i] - 1.0
        assert out["std_home_attack"][i] == np.exp(z[i, sl["std_home_attack"]][0])
        assert out["mean_away_defence"][i] == z[i, sl["mean_away_defence"]][0]
    if n_conf:
        assert np.array_equal(out["confederation_strength"], z[:, sl["confederation_strength_decentered"]])
    else:
        assert out["confederation_strength"] is None
    assert (out["attack_coefficients"] is None) == (k == 0) and (out["defence_coefficients"] is None) == (k == 0)
    if k:
        assert np.array_equal(out["attack_coefficients"], z[:, sl["attack_coefficients"]])
    assert "corr_coef" not in out   # a sampler statistic, not a function of the draw the host evaluates


def test_neutral_fit_sets_exactly_the_attributes_of_neutral_sites():
    """`_fit` assigns what neutral_sites returns (and corr_coef): the attribute list of the class is the dict's."""
    from bpl import NeutralDixonColesMatchPredictor

    sites = neutral_latent_sites(4, 0, 0)
    out = _mcmc.neutral_sites(sites, np.zeros((2, NO.latent_dim(4))), None, 0)
    m = NeutralDixonColesMatchPredictor()
    assert all(hasattr(m, nm) for nm in out) and hasattr(m, "corr_coef")


# -------------------------------------------------------------------------------------------------- dynamic_sites
@pytest.mark.parametrize("k", [0, 3])
def test_dynamic_sites_match_the_oracle(k):
    fx = DO.small_recipe(k=k) if k else DO.small_recipe()
    G, T = fx.n_gameweeks, fx.n_teams
    sites = dynamic_latent_sites(G, T, k)
    assert sites == DO.site_list(G, T, k)
    D = DO.latent_dim(G, T, k)
    z = np.stack([np.random.RandomState(s).uniform(-sc, sc, D) for s, sc in ((1, 0.3), (2, 2.0))])
    out = _mcmc.dynamic_sites(sites, z)
    from bpl.dynamic_dixon_coles import DynamicNeutralDixonColesMatchPredictor

    m = DynamicNeutralDixonColesMatchPredictor()
    assert all(hasattr(m, nm) for nm in out)
    assert not set(out) & set(m._VENUE_TABLES) and "corr_coef" not in out   # (those come from the library)
    for i in range(z.shape[0]):
        p = DO.unpack(z[i], G, T, k)
        u = DO._sig(p["u"])[0]
        assert out["u"].shape == (2, G, T) and np.abs(out["u"][i] - u).max() <= 4e-16 and np.array_equal(out["rho"][i], 2.0 * out["u"][i] - 1.0)
        for nm in ("std_attack", "std_defence", "std_home_attack", "std_away_attack", "std_home_defence", "std_away_defence"):
            assert out[nm].shape == (2, G) and np.array_equal(out[nm][i], np.exp(p[nm])), nm
        for nm in ("mean_home_attack", "mean_away_attack", "mean_home_defence", "mean_away_defence"):
            assert np.array_equal(out[nm][i], p[nm]), nm
        assert out["mean_defence"].shape == (2,) and out["mean_defence"][i] == p["mean_defence"]
        for nm in ("standardised_attack", "standardised_defence"):
            assert out[nm].shape == (2, G, T) and np.array_equal(out[nm][i], p[nm])
        # the venue offsets of the oracle's aux are these sites combined: mean + std * decentered
        aux = DO.potential_and_grad(fx, z[i])[2]
        lat = _mcmc.constrain_sites(sites, z[i:i + 1])
        for nm in ("home_attack", "away_attack", "home_defence", "away_defence"):
            assert _close(out["mean_" + nm][i][:, None] + out["std_" + nm][i][:, None] * lat[nm + "_decentered"][0], aux[nm])
    assert (out["attack_coefficients"] is None) == (k == 0)
    if k:
        assert np.array_equal(out["attack_coefficients"], z[:, :k])


# -------------------------------------------------------------------------------------------------- the sampler info
def test_running_mean_accept_prob():
    a = np.random.RandomState(0).uniform(0.3, 1.0, 3 * 11)
    got = _mcmc.running_mean_accept_prob(a, 3).reshape(3, 11)
    for c in range(3):
        for i in range(11):
            assert abs(got[c, i] - a.reshape(3, 11)[c, :i + 1].mean()) <= 4e-16
