"""MCMC convergence diagnostics without a GPU: the numpy restatement (tests/diagnostics_ref.py) against theory at
fixed seeds, and the Python layer (bpl/diagnostics.py) on a stand-in backend that calls the restatement: the
ValueErrors, the NaN rules, the shapes, "r_eff", "warnings", "sampler" and format_summary."""
import math

import numpy as np
import pytest

import bpl
import diagnostics_ref as R
from bpl import diagnostics as D
from loglik_ref import KINDS, hand_model


@pytest.fixture
def ref_backend(monkeypatch):
    monkeypatch.setattr(D, "_backend", R.backend)


# ---- the restatement against theory
def test_independent_normal_chains_look_converged():
    x = np.random.RandomState(11).normal(size=4000)
    d = R.diagnose_one(x, 4)
    assert d["rhat"] < 1.01
    assert 0.8 <= d["ess_bulk"] / 4000 <= 1.25 and 0.8 <= d["ess_mean"] / 4000 <= 1.25
    assert d["mcse_mean"] == pytest.approx(d["sd"] / math.sqrt(d["ess_mean"]), rel=1e-15)


def test_ar1_chains_have_the_textbook_efficiency():
    phi = 0.7
    x = R.ar1(np.random.RandomState(5), 4, 1000, phi)[:, 0]
    ratio = R.diagnose_one(x, 4)["ess_mean"] / 4000 / ((1 - phi) / (1 + phi))
    assert 1 / 1.3 <= ratio <= 1.3


def test_a_shifted_chain_raises_rhat():
    x = np.random.RandomState(3).normal(size=(4, 1000))
    x[2] += 2.0
    assert R.diagnose_one(x.ravel(), 4)["rhat"] > 1.2


def test_a_scaled_chain_shows_in_the_folded_rhat_only():
    x = np.random.RandomState(4).normal(size=(4, 1000))
    x[1] *= 3.0
    d = R.diagnose_one(x.ravel(), 4)
    assert abs(R.rhat_of(R.split_chains(x.ravel(), 4)) - 1.0) < 0.01
    assert d["rhat_folded"] > 1.05 and d["rhat"] == d["rhat_folded"]


def test_rank_statistics_are_invariant_under_exp():
    # |x - median| is not a monotone image of itself under exp, so only the bulk half of rhat is invariant: the seed
    # is one where that half is the larger one before and after
    x = np.random.RandomState(0).normal(size=2000)
    a, b = R.diagnose_one(x, 4), R.diagnose_one(np.exp(x), 4)
    assert a["rhat"] == a["rhat_bulk"] and b["rhat"] == b["rhat_bulk"]
    for key in ("rhat", "ess_bulk", "ess_tail"):
        assert abs(a[key] - b[key]) <= 1e-12, key
    # an increasing affine image keeps the order of |x - median| too
    c = R.diagnose_one(3.0 * x + 1.0, 4)
    assert abs(a["rhat_folded"] - c["rhat_folded"]) <= 1e-12


def test_ties_share_the_mean_of_their_ranks():
    v = np.round([0.31, 0.12, 0.29, 0.52, 0.08, 0.33, 0.11, 0.47, 0.9, 0.14, 0.26, 0.5, 0.94, 0.13, 0.06, 0.88], 1)
    # sorted: 0.1 x6 (ranks 1..6 -> 3.5), 0.3 x4 (7..10 -> 8.5), 0.5 x3 (11..13 -> 12), 0.9 x3 (14..16 -> 15)
    want = {0.1: 3.5, 0.3: 8.5, 0.5: 12.0, 0.9: 15.0}
    assert sorted(set(v)) == sorted(want)
    np.testing.assert_array_equal(R.average_ranks(v), [want[x] for x in v])
    z = R.z_scale(v.reshape(2, 8))
    assert z[0, 0] == z[0, 2] and z.shape == (2, 8)
    np.testing.assert_array_equal(R.average_ranks([0.0, -0.0, 1.0]), [1.5, 1.5, 3.0])


def test_split_drops_the_middle_draw_of_an_odd_chain():
    s = R.split_chains(np.arange(18.0), 2)
    np.testing.assert_array_equal(s, [[0, 1, 2, 3], [5, 6, 7, 8], [9, 10, 11, 12], [14, 15, 16, 17]])


def test_short_chains_take_the_floor():
    d = R.diagnose_one(np.random.RandomState(1).normal(size=8), 1)
    assert d["ess_mean"] == pytest.approx(8 * math.log10(8)) and np.isfinite(d["rhat"])


# ---- the Python layer
@pytest.mark.parametrize("values, chains, kw", [
    (np.zeros((14, 2)), 2, {}),                        # N = 7
    (np.zeros((65538 + 2, 1)), 2, {}),                 # S = 65 540
    (np.zeros((33, 2)), 2, {}),                        # not a multiple
    (np.zeros((32, 2)), 2, {"quantiles": (0.0, 0.5)}),
    (np.zeros((32, 2)), 2, {"quantiles": (0.5, 1.0)}),
    (np.zeros((32, 2)), 2, {"quantiles": (float("nan"),)}),
    (np.zeros((32, 2)), 0, {}),
    (np.zeros((257 * 8, 1)), 257, {}),
])
def test_bad_arguments_raise_before_any_device_call(monkeypatch, values, chains, kw):
    def never(*a):
        raise AssertionError("the backend was called")

    monkeypatch.setattr(D, "_backend", never)
    with pytest.raises(ValueError):
        bpl.mcmc_diagnostics(values, chains, **kw)


def test_the_limit_itself_is_accepted(monkeypatch):
    monkeypatch.setattr(D, "_backend", lambda v, C, q, ws: {nm: np.zeros(v.shape[1]) for nm in D.STATISTICS})
    assert bpl.mcmc_diagnostics(np.zeros((65536, 1)), 64)["rhat"].shape == (1,)
    assert bpl.mcmc_diagnostics(np.zeros((65537, 1)), 1)["rhat"].shape == (1,)   # N odd: S = 65 536


def test_shapes_follow_the_trailing_axes(ref_backend):
    rs = np.random.RandomState(2)
    for shape in [(64,), (64, 3), (64, 2, 3)]:
        v = rs.normal(size=shape)
        out = bpl.mcmc_diagnostics(v, 2)
        assert set(out) == set(D.STATISTICS)
        flat = v.reshape(64, -1)
        for nm in D.STATISTICS:
            assert out[nm].shape == shape[1:] and out[nm].dtype == np.float64
            want = np.array([R.diagnose_one(flat[:, j], 2)[nm] for j in range(flat.shape[1])]).reshape(shape[1:])
            np.testing.assert_array_equal(out[nm], want)
    assert bpl.mcmc_diagnostics(np.zeros((64, 0)), 2)["rhat"].shape == (0,)


def test_nan_rules(ref_backend):
    rs = np.random.RandomState(8)
    v = rs.normal(size=(80, 4))
    v[17, 1] = np.nan
    v[:, 2] = 0.1
    v[3, 3] = np.inf
    out = bpl.mcmc_diagnostics(v, 2)
    others = [nm for nm in D.STATISTICS if nm not in ("mean", "sd")]
    for nm in D.STATISTICS:
        assert np.isfinite(out[nm][0]), nm
    for j in (1, 2, 3):
        assert all(np.isnan(out[nm][j]) for nm in others), j
    assert np.isnan(out["mean"][1]) and np.isnan(out["sd"][1])
    assert out["mean"][2] == pytest.approx(0.1) and out["sd"][2] == pytest.approx(0.0, abs=1e-15)
    assert out["mean"][3] == np.inf and np.isnan(out["sd"][3])
    # W = 0 without a constant quantity: every split chain constant, the chains different
    w0 = R.diagnose_one(np.repeat(np.arange(4.0), 8), 2)
    assert np.isnan(w0["rhat"]) and np.isfinite(w0["ess_mean"]) and np.isfinite(w0["ess_bulk"])
    # var_plus = 0 in one ess only: nothing lies at or below the least value's quantile but that value's ties
    assert np.isnan(R.ess_of(np.ones((2, 8)))[0])


def _with_info(m, C, rs):
    S = m.corr_coef.shape[0]
    m.mcmc_info_ = {"num_chains": C, "diverging": (rs.uniform(size=S) < 0.02).astype(np.float64),
                    "accept_prob": rs.uniform(0.6, 1.0, S), "step_size": np.repeat(rs.uniform(0.1, 0.2, C), S // C)}
    return m


@pytest.mark.parametrize("kind", KINDS)
def test_the_method_assembles_sites_r_eff_warnings_and_sampler(ref_backend, kind):
    rs = np.random.RandomState(9)
    m = hand_model(kind, S=64, T=4, seed=3, C=2, G=2)
    with pytest.raises(ValueError, match="num_chains"):
        m.mcmc_diagnostics()
    out = m.mcmc_diagnostics(num_chains=2)
    assert "sampler" not in out
    names = [k for k in out if k not in ("r_eff", "warnings")]
    assert {"attack", "defence", "corr_coef"} <= set(names)
    assert ("home_advantage" in names) == (kind in ("basic", "extended"))
    assert ("home_attack" in names) == (kind not in ("basic", "extended"))
    assert ("confederation_strength" in names) == (kind == "wc")
    ratios = []
    for nm in names:
        a = np.asarray(getattr(m, nm))
        assert out[nm]["rhat"].shape == a.shape[1:]
        flat = a.reshape(64, -1)
        want = np.array([R.diagnose_one(flat[:, j], 2)["ess_mean"] for j in range(flat.shape[1])])
        np.testing.assert_array_equal(out[nm]["ess_mean"].ravel(), want)
        ratios.append(want / 64)
    assert out["r_eff"] == pytest.approx(np.mean(np.concatenate(ratios)), rel=1e-14)
    # 32 draws per chain: every site is below 100 effective draws per chain
    assert any(w.startswith("attack: ess_bulk") for w in out["warnings"])
    assert isinstance(D.format_summary(out, worst=3), str)

    _with_info(m, 2, rs)
    out = m.mcmc_diagnostics()
    div = m.mcmc_info_["diverging"].reshape(2, 32).sum(axis=1)
    np.testing.assert_array_equal(out["sampler"]["divergences"], div)
    np.testing.assert_allclose(out["sampler"]["mean_accept_prob"], m.mcmc_info_["accept_prob"].reshape(2, 32).mean(axis=1))
    np.testing.assert_array_equal(out["sampler"]["step_size"], m.mcmc_info_["step_size"].reshape(2, 32)[:, -1])
    assert any("divergent" in w for w in out["warnings"]) == bool(div.sum())
    text = D.format_summary(out, worst=5)
    assert "quantity" in text and "r_eff" in text and len(text.splitlines()) >= 7
    with pytest.raises(ValueError):
        m.mcmc_diagnostics(space="latent")
    with pytest.raises(ValueError):
        m.mcmc_diagnostics(space="unconstrained")   # (no unconstrained draws on a hand-built posterior)


def test_unconstrained_space_is_split_by_the_latent_sites(ref_backend):
    rs = np.random.RandomState(10)
    m = _with_info(hand_model("basic", S=64, T=4, seed=3), 2, rs)
    z = rs.normal(size=(64, 2 * 4 + 5))
    z[:32, 0] += 3.0   # chain 0 of attack_decentered[0] sits elsewhere
    m.mcmc_info_["unconstrained"] = z
    out = m.mcmc_diagnostics(space="unconstrained")
    sites = [k for k in out if k not in ("r_eff", "warnings", "sampler")]
    assert sites == ["attack_decentered", "corr_coef_raw", "defence_decentered", "home_advantage", "mean_defence",
                     "std_attack", "std_defence"]
    assert out["attack_decentered"]["rhat"].shape == (4,) and out["std_attack"]["rhat"].shape == (1,)
    assert out["defence_decentered"]["mean"][1] == pytest.approx(z[:, 6].mean())
    assert out["attack_decentered"]["rhat"][0] > 1.2
    assert any(w.startswith("attack_decentered: rhat") for w in out["warnings"])
    assert "attack_decentered[0]" in D.format_summary(out, worst=1)
    m.mcmc_info_["unconstrained"] = z[:, :-1]
    with pytest.raises(ValueError, match="latent sites"):
        m.mcmc_diagnostics(space="unconstrained")


def test_dynamic_latent_sites_keep_their_shapes(ref_backend):
    from bpl.dynamic_dixon_coles import latent_sites

    rs = np.random.RandomState(12)
    m = _with_info(hand_model("dynamic", S=32, T=3, seed=3, G=2), 2, rs)
    D_ = sum(int(np.prod(s)) for _, s in latent_sites(2, 3, 0))
    m.mcmc_info_["unconstrained"] = rs.normal(size=(32, D_))
    out = m.mcmc_diagnostics(space="unconstrained")
    assert out["u"]["rhat"].shape == (2, 3) and out["mean_defence"]["rhat"].shape == () \
        and out["std_attack"]["rhat"].shape == (2,)
