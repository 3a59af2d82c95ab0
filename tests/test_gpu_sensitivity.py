"""Power-scaling sensitivity on the device (csrc/dc_sensitivity.hip.h, bpl/sensitivity.py) against the numpy
restatement (tests/sensitivity_ref.py).

Gates: cjs_sq |got - ref| <= 1e-9 ref + 1e-15 -- on the square, because the rounding noise
of JS / B is about 1e-17 and a square root would turn it into some 6e-9; the absolute term is that noise with a
factor of about 25, the relative term the 1e-9 `mcmc_diagnostics` is held to.  mean, sd, log_weights, pareto_k and
ess: 1e-9 (1 + |ref|), as `psis_weights` and `mcmc_diagnostics` are held."""
import functools

import numpy as np
import pytest

import bpl
import sensitivity_ref as R
from bpl import sensitivity as SN
from bpl._ffi import BPLHIP_EINVAL, BplHipError
from loglik_ref import hand_data, hand_model, ll_matrix

pytestmark = pytest.mark.gpu
GATE = 1e-9
CJS_ABS = 1e-15
LDS_DRAWS = 12288   # csrc/dc_sensitivity.hip.h SHIFT_LDS_DRAWS: one draw more sorts through the workspace

# (S, Q, rows): every S of {8, 64, 257, 1000, 12288, 12289}, every Q of {1, 3, 70}, every row count of {1, 4, 8}
SHAPES = [(8, 70, 8), (64, 3, 4), (257, 70, 1), (1000, 3, 8), (12288, 1, 4), (12289, 3, 1)]


def _rows(lp, ll, rows):
    """rows = 8: delta = 0.5 and 0.01; 4: delta = 0.5; 1: the prior+ row of delta = 0.01."""
    if rows == 8:
        return np.concatenate([R.power_ratios(lp, ll, 0.5), R.power_ratios(lp, ll, 0.01)])
    return R.power_ratios(lp, ll, 0.5) if rows == 4 else R.power_ratios(lp, ll, 0.01)[1:2]


@functools.lru_cache(maxsize=None)
def _case(S, Q, rows):
    """Column 0 carries the likelihood (l = -x^2 / 2), column 1 (if any) the prior, the rest are independent."""
    rs = np.random.RandomState(100 + S + Q)
    v = rs.normal(size=(S, Q))
    ll = -0.5 * v[:, 0] ** 2
    lp = -np.abs(v[:, min(1, Q - 1)] - 0.5)
    ratios = _rows(lp, ll, rows)
    ref = R.weighted_shift(v, ratios)
    for a in (v, ratios) + tuple(ref.values()):
        a.setflags(write=False)
    return v, ratios, ref


def _compare(got, ref, label):
    g, r = np.asarray(got["cjs_sq"], dtype=np.float64).ravel(), np.asarray(ref["cjs_sq"]).ravel()
    assert np.array_equal(np.isnan(g), np.isnan(r)), (label, "cjs_sq")
    ok = ~np.isnan(r)
    ratio = np.abs(g[ok] - r[ok]) / (GATE * r[ok] + CJS_ABS)
    worst = {"cjs_sq (of its gate)": float(ratio.max()) if ratio.size else 0.0}
    for nm in ("mean", "sd", "log_weights", "pareto_k", "ess"):
        g, r = np.asarray(got[nm], dtype=np.float64).ravel(), np.asarray(ref[nm], dtype=np.float64).ravel()
        assert np.array_equal(np.isnan(g), np.isnan(r)), (label, nm)
        same = (g == r) | (np.isnan(g) & np.isnan(r))   # (infinite values must agree exactly)
        with np.errstate(invalid="ignore"):
            err = np.where(same, 0.0, np.abs(g - r) / (1.0 + np.abs(r)))
        assert not np.any(np.isnan(err)), (label, nm)
        worst[nm] = float(err.max()) if err.size else 0.0
    print(f"{label}: " + ", ".join(f"{nm} {e:.2e}" for nm, e in worst.items()))
    assert worst.pop("cjs_sq (of its gate)") <= 1.0, label
    for nm, e in worst.items():
        assert e <= GATE, (label, nm, e)
    assert np.array_equal(got["tail_len"], ref["tail_len"]), label


@pytest.mark.parametrize("S, Q, rows", SHAPES)
def test_device_matches_the_restatement(hip_ctx, S, Q, rows):
    v, ratios, ref = _case(S, Q, rows)
    got = hip_ctx.weighted_shift(v, ratios)
    assert got["cjs_sq"].shape == (rows, Q) and got["log_weights"].shape == (rows, S)
    _compare(got, ref, f"S={S} Q={Q} rows={rows}")


def test_the_limit_of_65536_draws(hip_ctx):
    v, ratios, ref = _case(65536, 2, 1)   # (a draw index of 65 535 still fits 16 bits; 256 positions per segment)
    _compare(hip_ctx.weighted_shift(v, ratios), ref, "limit S=65536")
    with pytest.raises(BplHipError) as e:
        hip_ctx.weighted_shift(np.zeros((65537, 1)), np.zeros((1, 65537)))
    assert e.value.code == BPLHIP_EINVAL


@functools.lru_cache(maxsize=None)
def _designed(S=257):
    rs = np.random.RandomState(7)
    x = rs.normal(size=S)
    # (the constant is a power of two: sum w x = 2 sum w in every rounding, so its mean is exact)
    cols = {"integers": rs.randint(0, 4, S).astype(np.float64), "constant": np.full(S, 2.0),
            "one_nan": rs.normal(size=S), "one_inf": rs.normal(size=S), "l": -0.5 * x * x,
            "independent": rs.normal(size=S), "x": x}
    cols["one_nan"][17] = np.nan
    cols["one_inf"][S - 3] = np.inf
    v = np.column_stack(list(cols.values()))
    spike = np.zeros(S)
    spike[int(np.argsort(x)[S // 3])] = 800.0   # every other weight underflows to 0: Q_i steps from 0 to 1
    ratios = np.stack([np.full(S, 3.0), spike, 0.5 * cols["l"], -cols["l"] / 3.0])
    ref = R.weighted_shift(v, ratios)
    return tuple(cols), v, ratios, ref


def test_designed_columns_and_rows(hip_ctx):
    names, v, ratios, ref = _designed()
    got = hip_ctx.weighted_shift(v, ratios)
    _compare(got, ref, "designed")
    col = {nm: j for j, nm in enumerate(names)}
    for nm in ("constant", "one_nan", "one_inf"):
        assert np.all(np.isnan(got["cjs_sq"][:, col[nm]])), nm
    assert np.array_equal(got["mean"][:, col["constant"]], np.full(4, 2.0))
    assert np.array_equal(got["sd"][:, col["constant"]], np.zeros(4))
    assert np.all(np.isnan(got["mean"][:, col["one_nan"]]))
    finite = [col[nm] for nm in ("integers", "l", "independent", "x")]
    # a constant ratio row: uniform weights, no quantity moves
    assert got["pareto_k"][0] == 0.0 and got["ess"][0] == v.shape[0]
    assert np.all(got["cjs_sq"][0, finite] <= 1e-15), got["cjs_sq"][0, finite]
    # the spike row: all the weight on one draw
    assert np.count_nonzero(np.exp(got["log_weights"][1])) == 1
    assert np.array_equal(got["sd"][1, finite], np.zeros(len(finite)))
    assert np.all(got["cjs_sq"][1, finite] > 0.01)
    # the likelihood's own column moves more than the independent one
    assert got["cjs_sq"][2, col["l"]] > 10.0 * got["cjs_sq"][2, col["independent"]]


def test_integer_draws_do_not_depend_on_the_tie_order(hip_ctx):
    _, v, ratios, _ = _designed()
    perm = np.random.RandomState(3).permutation(v.shape[0])
    a = hip_ctx.weighted_shift(v[:, :1], ratios[2:])
    b = hip_ctx.weighted_shift(v[perm, :1], ratios[2:, perm])
    gate = GATE * a["cjs_sq"] + CJS_ABS
    assert np.all(np.abs(a["cjs_sq"] - b["cjs_sq"]) <= gate), (a["cjs_sq"], b["cjs_sq"])


def test_two_calls_and_any_workspace_are_bit_identical(hip_ctx):
    S, Q = LDS_DRAWS + 1, 70
    rs = np.random.RandomState(11)
    v = rs.normal(size=(S, Q))
    v[:, 5] = np.round(v[:, 5])
    ratios = R.power_ratios(-np.abs(v[:, 1]), -0.5 * v[:, 0] ** 2, 0.5)
    one = hip_ctx.weighted_shift(v, ratios)
    again = hip_ctx.weighted_shift(v, ratios)
    chunked = hip_ctx.weighted_shift(v, ratios, workspace_bytes=24 * 12 * S)   # 24 quantities a chunk: 3 chunks
    for nm in one:
        assert np.array_equal(one[nm], again[nm], equal_nan=True), nm
        assert np.array_equal(one[nm], chunked[nm], equal_nan=True), nm
    assert np.all(np.isfinite(one["cjs_sq"]))
    small = hip_ctx.weighted_shift(v[:1000, :7], ratios[:, :1000])
    for ws in (1, 12 * 1000):   # up to 12 288 draws the sort needs no workspace: any size does
        other = hip_ctx.weighted_shift(v[:1000, :7], ratios[:, :1000], workspace_bytes=ws)
        assert all(np.array_equal(small[nm], other[nm]) for nm in small)


def test_limits_are_refused_before_any_launch(hip_ctx):
    v, r = np.zeros((16, 2)), np.zeros((1, 16))
    bad = [(np.zeros((7, 2)), np.zeros((1, 7)), {}), (v, np.zeros((9, 16)), {}), (v, np.zeros((0, 16)), {}),
           (v, np.full((1, 16), np.inf), {}), (v, np.full((1, 16), np.nan), {}), (v, r, {"r_eff": 0.0}),
           (v, r, {"workspace_bytes": -1}), (np.zeros((16, 0)), r, {}),
           (np.zeros((LDS_DRAWS + 1, 1)), np.zeros((1, LDS_DRAWS + 1)), {"workspace_bytes": 12 * LDS_DRAWS})]
    for values, ratios, kw in bad:
        with pytest.raises(BplHipError) as e:
            hip_ctx.weighted_shift(values, ratios, **kw)
        assert e.value.code == BPLHIP_EINVAL, (values.shape, ratios.shape, kw)
    assert hip_ctx.weighted_shift(v, r)["ess"][0] == 16.0   # the context is still usable


def test_powerscale_sensitivity_end_to_end(hip_ctx):
    v, l = R.gaussian_case(1000, seed=4)
    lp = -np.abs(v[:, 1])
    for delta in (0.01, 0.5):
        ref = R.powerscale(v, lp, l, delta)
        got = bpl.powerscale_sensitivity(v, lp, l, delta=delta)
        sq = {"cjs_sq": got["cjs"] ** 2, "mean": got["mean"], "sd": got["sd"], "pareto_k": got["pareto_k"],
              "ess": got["ess"], "log_weights": ref["log_weights"], "tail_len": ref["tail_len"]}
        _compare(sq, ref, f"powerscale delta={delta}")
        scale = 2.0 * np.log2(1.0 + delta)
        assert np.array_equal(got["prior"], (got["cjs"][0] + got["cjs"][1]) / scale)
        assert np.array_equal(got["likelihood"], (got["cjs"][2] + got["cjs"][3]) / scale)
        assert got["prior"].shape == (2,) and got["diagnosis"].shape == (2,)
    got = bpl.powerscale_sensitivity(v, lp, l)
    assert got["likelihood"][0] >= 0.05 > got["likelihood"][1]
    assert got["diagnosis"][0] in ("", SN.CONFLICT) and got["warnings"] == []


def _fit(kind):
    m0 = hand_model(kind, S=8, T=6 if kind == "dynamic" else 8, seed=5, G=3)
    data = hand_data(m0, n=120, seed=2, max_goals=4)
    rs = np.random.RandomState(9)
    kw = {"num_warmup": 150, "num_samples": 150, "mcmc_kwargs": {"num_chains": 2}}
    if kind == "basic":
        return bpl.DixonColesMatchPredictor().fit(data, **kw), data, None
    if kind == "extended":
        data["time_diff"] = rs.randint(0, 12, 120) / 4.0
        m = bpl.ExtendedDixonColesMatchPredictor().fit(data, epsilon=0.3, **kw)
        return m, data, np.exp(-0.3 * data["time_diff"])
    if kind == "neutral":
        data["game_weights"] = rs.choice([0.5, 1.0, 2.0, 3.0], 120)
        return bpl.NeutralDixonColesMatchPredictor().fit(data, **kw), data, np.asarray(data["game_weights"])
    from bpl.dynamic_dixon_coles import DynamicNeutralDixonColesMatchPredictor

    z0 = np.zeros(7 * 3 * 6 + 10 * 3 + 2)
    m = DynamicNeutralDixonColesMatchPredictor().fit(data, run_kwargs={"init_params": z0}, **kw)
    return m, data, None


@pytest.mark.filterwarnings("ignore:DynamicNeutralDixonColesMatchPredictor")
@pytest.mark.parametrize("kind", ["basic", "extended", "neutral", "dynamic"])
def test_prior_sensitivity_of_a_fitted_model(hip_ctx, kind):
    m, data, w = _fit(kind)
    S = 300
    got = m.prior_sensitivity(data)
    hook = m._fit_weights(data)
    assert (hook is None) == (w is None) and (w is None or np.array_equal(hook, w))
    ll = ll_matrix(m, data)
    ll_ref = (ll * (1.0 if w is None else w[None, :])).sum(axis=1)
    err = np.abs(got["log_likelihood"] - ll_ref) / (1.0 + np.abs(ll_ref))
    print(f"{kind}: log_likelihood worst error / (1 + |ref|) {err.max():.2e}")
    assert got["log_likelihood"].shape == (S,) and err.max() <= GATE
    info = m.mcmc_info_
    lp_ref = -info["potential_energy"] - ll_ref - R.log_jacobian(m._latent_sites(), info["unconstrained"])
    assert np.abs(got["log_prior"] - lp_ref).max() <= GATE * (1.0 + np.abs(lp_ref).max())
    sites = m._diagnostic_arrays("constrained")
    flat = np.concatenate([a.reshape(S, -1) for a in sites.values()], axis=1)
    ref = R.powerscale(flat, lp_ref, ll_ref, 0.01)
    at, worst = 0, 0.0
    scale = 2.0 * np.log2(1.01)
    for name, a in sites.items():
        size = int(np.prod(a.shape[1:]))
        assert got[name]["prior"].shape == a.shape[1:] == got[name]["diagnosis"].shape
        for comp, (i, j) in (("prior", (0, 1)), ("likelihood", (2, 3))):
            g = got[name][comp].ravel()
            c_lo, c_hi = np.sqrt(ref["cjs_sq"][i, at:at + size]), np.sqrt(ref["cjs_sq"][j, at:at + size])
            r = (c_lo + c_hi) / scale
            assert np.array_equal(np.isnan(g), np.isnan(r)), (name, comp)
            # the gate on cjs_sq carried through c -> sqrt(c) (d sqrt = d c / (2 sqrt c)) and the sum of the two
            tol = ((GATE * c_lo ** 2 + CJS_ABS) / (2.0 * c_lo) + (GATE * c_hi ** 2 + CJS_ABS) / (2.0 * c_hi)) / scale
            ok = ~np.isnan(r)
            if ok.any():
                worst = max(worst, float((np.abs(g[ok] - r[ok]) / tol[ok]).max()))
        at += size
    print(f"{kind}: {at} quantities, worst sensitivity error of its gate {worst:.2e}; pareto_k {got['pareto_k']}")
    assert worst <= 1.0
    assert np.abs(got["pareto_k"] - ref["pareto_k"]).max() <= GATE * (1.0 + np.abs(ref["pareto_k"]).max())
    assert np.abs(got["ess"] - ref["ess"]).max() <= GATE * (1.0 + np.abs(ref["ess"]).max())
    explicit = m.prior_sensitivity(data, weights=np.ones(120) if hook is None else hook)
    for name in sites:
        for comp in ("prior", "likelihood", "diagnosis"):
            assert np.array_equal(explicit[name][comp], got[name][comp], equal_nan=comp != "diagnosis"), (name, comp)
    assert np.array_equal(explicit["log_prior"], got["log_prior"])
    print(SN.format_summary(got, worst=5))
