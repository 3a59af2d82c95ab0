"""predict_markets on the device (csrc/dc_market.hip.h, bpl/markets.py) against the numpy restatement
(tests/markets_ref.py: the full scoreline grid of every draw and fixture, an einsum, np.sort and the
interpolation formula written out) for the five predictor classes, against what the project already computes,
and on shape edges, exact order statistics, clipped tau, determinism and the library's own errors.

Gates (the section 15 argument extended): a per-draw value is a sum of at most
(G+1)^2 <= 4096 terms W q whose partial sums of |W| q stay below max|W| (the grid sums to about 1), and each
term carries at most about 200 roundings (the recurrences up to depth 63, four exp), so its absolute error is
at most about (4096 + 200) 2^-53 max(1, max|W|) < 1e-12 max(1, max|W|) =: g, per market.  Per-draw values and
the mean: within g.  A quantile is 1-Lipschitz in the sup norm of the values: g plus one rounding of the
interpolation.  sd is Lipschitz with constant sqrt(S / (S - 1)): 10 g, which also covers the two-pass sum."""
import numpy as np
import pytest

import loglik_ref as LR
import markets_ref as MR
from bpl import markets as MK
from bpl._ffi import BPLHIP_EINVAL, BPLHIP_ESTATE, BplHipError, HipContext

pytestmark = pytest.mark.gpu

K_PASS = 8   # csrc/dc_market.hip.h MARKET_KPASS
QS = (0.0, 0.05, 0.5, 0.95, 1.0)
ARRAYS = ("mean", "sd", "quantile", "draws")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _markets(G, K=None, seed=0):
    """One market from every builder and random-weight arrays with entries in [-2, 2]: 15 markets, or K."""
    rs = np.random.RandomState(seed)
    mk = MR.all_builders()
    while len(mk) < (15 if K is None else K):
        mk[f"random_{len(mk)}"] = rs.uniform(-2.0, 2.0, (G + 1, G + 1))
    return dict(list(mk.items())[:K])


def _gates(markets, G):
    W = MR.weights_of(markets, G)
    return 1e-12 * np.maximum(1.0, np.abs(W).reshape(W.shape[0], -1).max(axis=1))   # g [K]


def _compare(got, ref, g, tag, draws=True):
    """`got` against the restatement `ref` within the gates; prints the measured maxima over the gate."""
    for key in ARRAYS if draws else ARRAYS[:3]:
        assert not np.isnan(got[key]).any(), key
        assert got[key].shape == ref[key].shape, key
    S = ref["draws"].shape[0]
    one = 2.0 ** -52 * np.maximum(1.0, np.abs(ref["draws"]).max(axis=(0, 2)))   # one rounding of a value, per market
    err = {"mean": (np.abs(got["mean"] - ref["mean"]).max(axis=1), g),
           "sd": (np.abs(got["sd"] - ref["sd"]).max(axis=1), 10 * g),
           "quantile": (np.abs(got["quantile"] - ref["quantile"]).reshape(len(g), -1).max(axis=1, initial=0.0), g + one)}
    if draws:
        err["draws"] = (np.abs(got["draws"] - ref["draws"]).max(axis=(0, 2)), g)
    for key, (e, gate) in err.items():
        print(f"{tag}: {key} error / gate {(e / gate).max():.3e} (S={S})")
    for key, (e, gate) in err.items():
        assert (e <= gate).all(), (key, (e / gate).max())


def _check(m, d, G, markets, quantiles=QS, tag=""):
    got = m.predict_markets(d, markets, max_goals=G, quantiles=quantiles, return_draws=True)
    ref = MR.predict_markets(m, d, markets, G, quantiles)
    assert got["kind"] == "markets" and got["n"] == len(d["home_team"]) and got["markets"] == tuple(markets)
    np.testing.assert_array_equal(got["quantiles"], np.asarray(quantiles, dtype=np.float64))
    _compare(got, ref, _gates(markets, G), tag)
    return got, ref


# 1
@pytest.mark.parametrize("G", [1, 2, 15])
@pytest.mark.parametrize("kind", LR.KINDS)
def test_all_classes_against_restatement(kind, G):
    m = LR.hand_model(kind, S=257, T=8, seed=3)
    d = LR.hand_data(m, n=130, seed=4)
    _check(m, d, G, _markets(G), tag=f"{kind} G={G}")


# 2
@pytest.mark.parametrize("G", [0, 16, 63])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65])
@pytest.mark.parametrize("kind", ["basic", "wc"])
def test_shape_edges(kind, S, n, G):
    m = LR.hand_model(kind, S=S, T=6, seed=S)
    d = LR.hand_data(m, n=n, seed=n)
    full = _markets(G, K=64, seed=G)
    # one restatement for the 64 markets; K < 64 takes its first K (the passes of K_PASS: 1, full, full + 1, all)
    ref = MR.predict_markets(m, d, full, G, QS)
    g = _gates(full, G)
    for K in (1, K_PASS, K_PASS + 1, 64):
        got = m.predict_markets(d, dict(list(full.items())[:K]), max_goals=G, quantiles=QS, return_draws=True)
        _compare(got, {"mean": ref["mean"][:K], "sd": ref["sd"][:K], "quantile": ref["quantile"][:K],
                       "draws": ref["draws"][:, :K]}, g[:K], f"{kind} S={S} n={n} G={G} K={K}")
        if S == 1:
            assert (got["sd"] == 0.0).all()
            assert (got["quantile"] == got["draws"][0][:, None, :]).all()   # every quantile is the single value
        if G == 0 and K == 64:
            # only 0-0 is on the grid: draw, the clean sheets and correct_score(0, 0) alone have mass
            mean = dict(zip(got["markets"], got["mean"]))
            for name in ("draw", "clean_sheet_home", "clean_sheet_away"):
                assert (mean[name] > 0.0).all(), name
            for name in ("home_win", "away_win", "over_2.5", "btts", "score_1_0", "handicap_home_-1",
                         "goals_home", "goals_away", "total_goals"):
                i = got["markets"].index(name)
                assert (got["draws"][:, i] == 0.0).all() and (got["quantile"][i] == 0.0).all(), name
    if G == 0:
        r = m.predict_markets(d, {"s00": MK.correct_score(0, 0), "draw": MK.draw()}, max_goals=0, return_draws=True)
        assert (r["draws"][:, 0] > 0.0).all() and r["draws"][:, 0].tobytes() == r["draws"][:, 1].tobytes()


# 3
def test_many_draws():
    # 4097 draws: 17 draw tiles of 256 in market_values, 65 values per lane in market_summary and a selection
    # that needs more than one digit
    m = LR.hand_model("neutral", S=4097, T=6, seed=31)
    d = LR.hand_data(m, n=3, seed=32)
    _check(m, d, 15, {"over_2.5": MK.total_over(2.5), "goals_home": MK.goals("home")},
           quantiles=(0.0, 0.001, 0.05, 0.25, 0.5, 0.75, 0.95, 0.999, 1.0), tag="S=4097")


# 4
@pytest.mark.parametrize("S", [1, 257, 1001])
def test_exact_order_statistics(S):
    m = LR.hand_model("extended", S=S, T=8, seed=41)
    d = LR.hand_data(m, n=20, seed=42)
    G = 15
    mk = _markets(G)
    r = m.predict_markets(d, mk, max_goals=G, quantiles=(0.0, 0.5, 1.0), return_draws=True)
    srt = np.sort(r["draws"], axis=0)
    for i, at in enumerate((0, (S - 1) // 2, S - 1)):
        assert r["quantile"][:, i].tobytes() == srt[at].tobytes(), (i, at)
    # the device mean is a sum of the same S values in another order: within S 2^-53 max|v|
    vmax = np.abs(r["draws"]).max(axis=0)
    err = np.abs(r["mean"] - r["draws"].mean(axis=0))
    print(f"S={S}: mean against the mean of the returned draws, error / (S 2^-53 max|v|) "
          f"{(err / np.maximum(S * 2.0 ** -53 * vmax, 1e-300)).max():.3e}")
    assert (err <= S * 2.0 ** -53 * vmax).all()
    # interpolated quantiles from the returned draws, the formula written out
    qs = (0.05, 0.3, 0.95)
    r2 = m.predict_markets(d, mk, max_goals=G, quantiles=qs)
    want = MR.summarise(r["draws"], qs)["quantile"]
    assert np.abs(r2["quantile"] - want).max() <= 2.0 ** -52 * np.abs(r["draws"]).max()


# 5
def test_clipped_tau_agrees_and_has_no_nan():
    m = LR.hand_model("basic", S=64, T=4, seed=2)
    m.corr_coef = np.where(np.arange(64) % 3 == 0, 5.0, 0.01)   # 1 - rho lh la < 0 and 1 - rho < 0 on some draws
    d = {"home_team": ["t00", "t01", "t02", "t03"], "away_team": ["t01", "t02", "t03", "t00"]}
    for G in (0, 1, 15):
        mk = MR.all_builders()
        mk["score_0_0"], mk["score_1_1"], mk["score_0_1"] = (MK.correct_score(0, 0), MK.correct_score(1, 1),
                                                             MK.correct_score(0, 1))
        got, _ = _check(m, d, G, mk, tag=f"clipped G={G}")
        for key in ARRAYS:
            assert (got[key] >= 0.0).all(), key   # non-negative weights: nothing negative
        i = got["markets"].index("score_1_1")
        if G >= 1:
            assert (got["draws"][::3, i] == 0.0).all()   # a clipped cell is an exact 0


# 6
@pytest.mark.parametrize("kind", LR.KINDS)
def test_against_forecast_scores_and_the_grid(kind):
    m = LR.hand_model(kind, S=300, T=8, seed=11)
    d = LR.hand_data(m, n=64, seed=12)
    G = 15
    cells = ((0, 0), (1, 0), (1, 1), (2, 1), (0, 3), (5, 5))
    mk = {"home_win": MK.home_win(), "draw": MK.draw(), "away_win": MK.away_win(), "over_2": MK.total_over(2),
          "under_2": MK.total_under(2), "over_2.5": MK.total_over(2.5), "under_2.5": MK.total_under(2.5)}
    x, y = np.meshgrid(np.arange(G + 1), np.arange(G + 1), indexing="ij")
    mk["push_2"] = (x + y == 2).astype(np.float64)
    for cx, cy in cells:
        mk[f"score_{cx}_{cy}"] = MK.correct_score(cx, cy)
    r = m.predict_markets(d, mk, max_goals=G, quantiles=())
    mean = dict(zip(r["markets"], r["mean"]))
    proba = m.forecast_scores(d, max_goals=G)["outcome_proba"]
    err = max(np.abs(mean[name] - proba[:, k]).max() for k, name in enumerate(("home_win", "draw", "away_win")))
    print(f"{kind}: outcome means against forecast_scores {err:.3e}")
    assert err <= 2e-12, err
    total = mean["home_win"] + mean["draw"] + mean["away_win"]
    for line, push in (("2", mean["push_2"]), ("2.5", 0.0)):
        err = np.abs(mean[f"over_{line}"] + mean[f"under_{line}"] + push - total).max()
        print(f"{kind}: over + under + push at {line} against the outcome sum {err:.3e}")
        assert err <= 4e-12, err
    # the float32 grid route: its own 3e-6 (tests/test_gpu_scores.py, from tests/test_gpu_fit.py)
    groups, _ = m._loglik_groups(d)
    worst = 0.0
    for positions, device, kw in groups:
        at = np.arange(64) if positions is None else positions
        grid = device().predict_score_grid(kw["home_idx"], kw["away_idx"], G, neutral=kw.get("neutral"),
                                           conf=kw.get("conf"))
        for cx, cy in cells:
            worst = max(worst, np.abs(mean[f"score_{cx}_{cy}"][at] - grid[:, cx, cy]).max())
    print(f"{kind}: correct_score means against predict_score_grid {worst:.3e}")
    assert worst < 3e-6, worst


# 7
def _bits_equal(a, b, keys=ARRAYS):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("kind", ["wc", "dynamic"])
def test_two_calls_and_permuted_fixtures_are_bit_identical(kind):
    m = LR.hand_model(kind, S=300, T=8, seed=15, G=4)
    d = LR.hand_data(m, n=90, seed=16)
    mk = _markets(15)
    a = m.predict_markets(d, mk, return_draws=True)
    _bits_equal(a, m.predict_markets(d, mk, return_draws=True))
    perm = np.random.RandomState(17).permutation(90)
    shuffled = {k: [v[i] for i in perm] for k, v in d.items()}
    b = m.predict_markets(shuffled, mk, return_draws=True)
    _bits_equal({k: np.ascontiguousarray(a[k][..., perm]) for k in ARRAYS}, b)


@pytest.mark.parametrize("kind", ["basic", "neutral"])
def test_chunked_workspace_is_bit_identical(kind):
    m = LR.hand_model(kind, S=257, T=8, seed=3)
    d = LR.hand_data(m, n=130, seed=4)
    G, mk = 15, _markets(15)
    W = MR.weights_of(mk, G)
    (_, device, kw), = m._fixture_groups(d, with_goals=False)[0]
    whole = device().market_summary(**kw, max_goals=G, weights=W, quantiles=QS, return_draws=True)
    per_fixture = W.shape[0] * 257 * 8
    for fixtures in (1, 7, 43, 129):   # 130, 19, 4 and 2 chunks
        part = device().market_summary(**kw, max_goals=G, weights=W, quantiles=QS, return_draws=True,
                                       workspace_bytes=fixtures * per_fixture + 5)
        _bits_equal(whole, part)
    _bits_equal(whole, m.predict_markets(d, mk, max_goals=G, quantiles=QS, return_draws=True))


# 8
def test_library_errors():
    h = np.array([0, 1], dtype=np.uint16)
    w = np.ones((2, 16, 16))
    ctx = HipContext(0)

    def fails(code, *args, **kwargs):
        with pytest.raises(BplHipError) as e:
            ctx.market_summary(*args, **kwargs)
        assert e.value.code == code, (e.value.code, args[2:], kwargs)

    fails(BPLHIP_ESTATE, h, h[::-1], 15, w)                      # no posterior
    rs = np.random.RandomState(0)
    ctx.predict_set_posterior(rs.normal(0, 0.2, (10, 2)), rs.normal(0, 0.2, (10, 2)), rs.normal(0, 0.1, 10),
                              rs.uniform(-0.05, 0.05, 10))
    fails(BPLHIP_ESTATE, h, h[::-1], 15, w, neutral=[0, 1])      # the other form's entry point
    fails(BPLHIP_EINVAL, h, h[::-1], 64, np.ones((2, 65, 65)))
    fails(BPLHIP_EINVAL, h, h[::-1], -1, np.ones((2, 0, 0)))
    fails(BPLHIP_EINVAL, h[:0], h[:0], 15, w)                    # no fixture
    fails(BPLHIP_EINVAL, h, h[::-1], 15, np.ones((0, 16, 16)))   # K = 0
    fails(BPLHIP_EINVAL, h, h[::-1], 15, np.ones((65, 16, 16)))  # K = 65
    fails(BPLHIP_EINVAL, h, h[::-1], 15, w, quantiles=np.linspace(0, 1, 17))
    fails(BPLHIP_EINVAL, h, h[::-1], 15, w, quantiles=[0.5, 1.5])
    fails(BPLHIP_EINVAL, h, h[::-1], 15, w, quantiles=[np.nan])
    bad = w.copy()
    bad[1, 3, 4] = np.inf
    fails(BPLHIP_EINVAL, h, h[::-1], 15, bad)
    fails(BPLHIP_EINVAL, h, h[::-1], 15, w, workspace_bytes=-1)
    fails(BPLHIP_EINVAL, h, h[::-1], 15, w, workspace_bytes=2 * 10 * 8 - 1)   # holds no fixture
    out = ctx.market_summary(h, h[::-1], 63, np.ones((3, 64, 64)), quantiles=[0.1, 0.9], return_draws=True)
    assert out["mean"].shape == (3, 2) and out["sd"].shape == (3, 2) and out["quantile"].shape == (3, 2, 2)
    assert out["draws"].shape == (10, 3, 2) and np.isfinite(out["draws"]).all()
    out = ctx.market_summary(h, h[::-1], 15, w, workspace_bytes=2 * 10 * 8)    # one fixture per chunk
    assert out["quantile"].shape == (2, 0, 2) and "draws" not in out
    ctx.close()
