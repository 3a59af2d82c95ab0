"""MCMC convergence diagnostics on the device (csrc/dc_diagnostics.hip.h) against the numpy restatement
(tests/diagnostics_ref.py).  Gate: 1e-9 (1 + |ref|) for every statistic, the gate `loo` holds for the same kind of
float64 sums over at most 65 536 terms.  Every case first asserts on the CPU that the restatement's decision margin
is at least 1e-6, so that a last-ulp difference cannot flip a truncation; a case that misses it gets another seed."""
import functools

import numpy as np
import pytest

import bpl
import diagnostics_ref as R
from bpl import diagnostics as D
from bpl._ffi import BPLHIP_EINVAL, BplHipError
from loglik_ref import KINDS, hand_data, hand_model

pytestmark = pytest.mark.gpu
GATE = 1e-9
MARGIN = 1e-6
QUANTILES = (0.05, 0.95)

# (C, N, Q, seed): every C of {1, 2, 3, 7, 64}, every N of {8, 9, 63, 64, 65, 129, 1000}, every Q of {1, 2, 65, 300};
# (64, 1000) is S = 64 000, above the 12 288 draws the sort keeps in LDS
SHAPES = [(1, 8, 300, 0), (2, 9, 65, 0), (3, 63, 2, 0), (7, 64, 1, 0), (64, 65, 2, 0), (1, 129, 65, 0), (3, 1000, 2, 0),
          (64, 1000, 1, 0)]
LIMIT = (64, 1024, 2, 0)


@functools.lru_cache(maxsize=None)
def _case(C, N, Q, seed, kind="normal"):
    rs = np.random.RandomState(1000 + seed)
    if kind == "ar99":
        v = R.ar1(rs, C, N, 0.99, Q)
    else:
        # chains of different location and scale, a heavy tail: continuous, no ties
        v = rs.standard_t(5, size=(C, N, Q)) * rs.uniform(0.5, 2.0, (C, 1, Q)) + rs.normal(0, 0.3, (C, 1, Q))
        v = v.reshape(C * N, Q)
    v.setflags(write=False)
    ref = R.diagnose(v, C, QUANTILES)
    for a in ref.values():
        a.setflags(write=False)
    return v, ref


def _compare(got, ref, label):
    worst = {}
    for nm in R.STATS:
        g, r = np.asarray(got[nm], dtype=np.float64).ravel(), np.asarray(ref[nm]).ravel()
        assert np.array_equal(np.isnan(g), np.isnan(r)), (label, nm)
        ok = ~np.isnan(r)
        err = np.abs(g[ok] - r[ok]) / (1.0 + np.abs(r[ok]))
        worst[nm] = float(err.max()) if err.size else 0.0
    print(f"{label}: worst error / (1 + |ref|): " + ", ".join(f"{nm} {e:.2e}" for nm, e in worst.items()))
    for nm, e in worst.items():
        assert e <= GATE, (label, nm, e)


@pytest.mark.parametrize("C, N, Q, seed", SHAPES)
def test_device_matches_the_restatement(hip_ctx, C, N, Q, seed):
    v, ref = _case(C, N, Q, seed)
    assert ref["margin"].min() >= MARGIN, ref["margin"].min()
    _compare(hip_ctx.mcmc_diagnostics(v, C, QUANTILES), ref, f"C={C} N={N} Q={Q}")


def test_the_limit_of_65536_split_draws(hip_ctx):
    C, N, Q, seed = LIMIT
    v, ref = _case(C, N, Q, seed)
    assert ref["margin"].min() >= MARGIN, ref["margin"].min()
    _compare(hip_ctx.mcmc_diagnostics(v, C, QUANTILES), ref, "limit 64 x 1024")


def test_slow_mixing_walks_many_lag_blocks(hip_ctx):
    v, ref = _case(4, 1000, 2, 0, "ar99")
    assert ref["margin"].min() >= MARGIN, ref["margin"].min()
    assert ref["ess_mean"].max() < 4000 / 64    # tau above 64: the truncation lies beyond the first block of lags
    _compare(hip_ctx.mcmc_diagnostics(v, 4, QUANTILES), ref, "AR(1) 0.99")


def test_tied_values_share_ranks(hip_ctx):
    v = np.round(_case(3, 129, 65, 0)[0], 1) + 0.0
    v[5, 0], v[6, 0] = 0.0, -0.0
    ref = R.diagnose(v, 3, QUANTILES)
    assert ref["margin"].min() >= MARGIN, ref["margin"].min()
    _compare(hip_ctx.mcmc_diagnostics(v, 3, QUANTILES), ref, "ties")


def test_nan_and_constant_quantities_beside_healthy_ones(hip_ctx):
    v = _case(3, 63, 2, 0)[0]
    v = np.concatenate([v, v[:, :1], np.full((v.shape[0], 1), 0.1), v[:, 1:]], axis=1)
    v[40, 2] = np.nan
    ref = R.diagnose(v, 3, QUANTILES)
    got = hip_ctx.mcmc_diagnostics(v, 3, QUANTILES)
    others = [nm for nm in R.STATS if nm not in ("mean", "sd")]
    assert all(np.isnan(got[nm][2]) and np.isnan(got[nm][3]) for nm in others)
    assert np.isnan(got["mean"][2]) and np.isnan(got["sd"][2])
    assert all(np.isfinite(got[nm][j]) for nm in R.STATS for j in (0, 1, 4))
    _compare(got, ref, "NaN and constant")


def test_runs_and_workspaces_agree_bit_for_bit(hip_ctx):
    for C, N, Q in [(3, 129, 65), (64, 1000, 1)]:
        v = _case(C, N, Q, 0)[0] if Q > 1 else np.repeat(_case(C, N, Q, 0)[0], 3, axis=1) * np.array([1.0, -1.0, 2.0])
        S = 2 * C * (N // 2)
        one = S * (16 if S <= 12288 else 28) + 2 * 8 + 8   # a single quantity (include/bplhip.h)
        a = hip_ctx.mcmc_diagnostics(v, C, QUANTILES)
        b = hip_ctx.mcmc_diagnostics(v, C, QUANTILES)
        c = hip_ctx.mcmc_diagnostics(v, C, QUANTILES, workspace_bytes=one)
        d = hip_ctx.mcmc_diagnostics(v, C, QUANTILES, workspace_bytes=2 * one + 100)
        for nm in R.STATS:
            for other in (b, c, d):
                assert a[nm].tobytes() == other[nm].tobytes(), (C, N, nm)
        with pytest.raises(BplHipError) as e:
            hip_ctx.mcmc_diagnostics(v, C, QUANTILES, workspace_bytes=one - 8)
        assert e.value.code == BPLHIP_EINVAL
        with pytest.raises(BplHipError) as e:
            hip_ctx.mcmc_diagnostics(v, C, QUANTILES, workspace_bytes=-1)
        assert e.value.code == BPLHIP_EINVAL


def test_too_many_draws_are_refused_on_the_host(hip_ctx, monkeypatch):
    def never(*a):
        raise AssertionError("the device was called")

    monkeypatch.setattr(D, "_device_call", never)
    with pytest.raises(ValueError):
        bpl.mcmc_diagnostics(np.zeros((65538, 1)), 1)
    # ... and by the entry point itself, with the other range checks
    for v, C, q in [(np.zeros((65538, 1)), 1, QUANTILES), (np.zeros((14, 1)), 2, QUANTILES),
                    (np.zeros((32, 1)), 2, (0.0,)), (np.zeros((257 * 8, 1)), 257, QUANTILES)]:
        with pytest.raises(BplHipError) as e:
            hip_ctx.mcmc_diagnostics(v, C, q)
        assert e.value.code == BPLHIP_EINVAL


def test_the_public_function_keeps_trailing_shapes(hip_ctx):
    v, ref = _case(2, 9, 65, 0)
    out = bpl.mcmc_diagnostics(v.reshape(18, 5, 13), 2)
    for nm in R.STATS:
        assert out[nm].shape == (5, 13)
    _compare({nm: out[nm].ravel() for nm in R.STATS}, ref, "public")


@pytest.mark.parametrize("kind", KINDS)
def test_the_method_on_hand_built_models(hip_ctx, kind):
    m = hand_model(kind, S=64, T=4, seed=3, C=2, G=2)
    out = m.mcmc_diagnostics(num_chains=2)
    for nm in ("attack", "defence", "corr_coef"):
        a = np.asarray(getattr(m, nm)).reshape(64, -1)
        ref = R.diagnose(a, 2, QUANTILES)
        _compare({k: out[nm][k].ravel() for k in R.STATS}, ref, f"{kind} {nm}")
    assert 0.0 < out["r_eff"] and isinstance(out["warnings"], list) and "sampler" not in out
    if kind == "basic":   # a stand-in mcmc_info_: both spaces
        rs = np.random.RandomState(2)
        m.mcmc_info_ = {"num_chains": 2, "unconstrained": rs.normal(size=(64, 13)), "diverging": np.zeros(64),
                        "accept_prob": rs.uniform(0.6, 1, 64), "step_size": np.full(64, 0.2)}
        un = m.mcmc_diagnostics(space="unconstrained")
        _compare({k: un["attack_decentered"][k] for k in R.STATS},
                 R.diagnose(m.mcmc_info_["unconstrained"][:, :4], 2, QUANTILES), "unconstrained")
        assert un["sampler"]["divergences"].tolist() == [0, 0] and m.mcmc_diagnostics()["sampler"]["step_size"][1] == 0.2


def test_a_real_short_fit(hip_ctx):
    m0 = hand_model("basic", S=8, T=8, seed=5)
    data = hand_data(m0, n=120, seed=2, max_goals=4)
    m = bpl.DixonColesMatchPredictor().fit(data, num_warmup=200, num_samples=200, mcmc_kwargs={"num_chains": 4})
    for space in ("constrained", "unconstrained"):
        out = m.mcmc_diagnostics(space=space)
        arrays = m._diagnostic_arrays(space)
        for nm, a in arrays.items():
            ref = R.diagnose(a.reshape(800, -1), 4, QUANTILES)
            _compare({k: out[nm][k].ravel() for k in R.STATS}, ref, f"fit {space} {nm}")
        assert out["sampler"]["divergences"].shape == (4,) and out["sampler"]["step_size"].shape == (4,)
        assert np.isfinite(out["r_eff"]) and 0.0 < out["r_eff"]
    print(D.format_summary(m.mcmc_diagnostics(), worst=5))
    res = m.loo(data, r_eff=m.mcmc_diagnostics()["r_eff"])
    assert np.isfinite(res["elpd_loo"])
