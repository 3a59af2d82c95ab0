"""predict_periods on the device (csrc/dc_period.hip.h, bpl/periods.py) against the numpy restatement
(tests/periods_ref.py: the full [G+1]^4 joint law of every draw and fixture from closed-form pmfs, a contraction,
np.sort and the interpolation formula written out) for the five predictor classes, against predict_markets and
predict_in_play, which share its law, and on shape edges, the tau cells, determinism and the library's own errors.

Gates (the section 16 argument extended): a per-draw value is a sum of T^2 terms W p,
T = (G+1)(G+2)/2, whose partial sums of |W| p stay below max|W| (the law sums to about 1), and each term carries
at most R = 6 G + 64 roundings (four recurrences of total depth x + y <= 2 G with three roundings a step, the
rounded 1 / k among them; the log rates, six exp, the products that join the factors, the tau factor), so its
absolute error is at most g_p = (T^2 + R) 2^-53 max(1, max|W|) per market: 2.1e-12 at G = 15, 3.1e-11 at G = 31.
Per-draw values and the mean: within g_p.  A quantile is 1-Lipschitz in the sup norm of the values: g_p plus one
rounding of the interpolation.  sd is Lipschitz with constant sqrt(S / (S - 1)): 10 g_p."""
import itertools

import numpy as np
import pytest

import loglik_ref as LR
import markets_ref as MR
import periods_ref as PR
import scores_ref as SR
from bpl import markets as MK
from bpl import periods as PD
from bpl._ffi import BPLHIP_EINVAL, BPLHIP_ESTATE, BplHipError, HipContext

pytestmark = pytest.mark.gpu

K_PASS = 8    # csrc/dc_period.hip.h PERIOD_KPASS
BLOCK = 8     # csrc/dc_period.hip.h PERIOD_DB
QS = (0.0, 0.05, 0.5, 0.95, 1.0)
ARRAYS = ("mean", "sd", "quantile", "draws")
SPLITS = (0.0, 1.0 / 9.0, 0.5, 0.9, 1.0)
G_MARKETS = 1e-12   # the gate of predict_markets, times max(1, max|W|)
LARGEST = {}        # quantity -> (error / gate, case): the maxima over the module, printed by the last test


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _markets(G, K=12, seed=0):
    """One market from every builder and random-weight arrays with entries in [-2, 2]: K in all."""
    rs = np.random.RandomState(seed)
    mk = PR.all_builders()
    while len(mk) < K:
        mk[f"random_{len(mk)}"] = rs.uniform(-2.0, 2.0, (G + 1,) * 4)
    return dict(list(mk.items())[:K])


def _wmax(W, G):
    """max(1, max|W|) over the readable cells, per market."""
    return np.maximum(1.0, np.abs(np.where(PR.readable(G), W, 0.0)).reshape(W.shape[0], -1).max(axis=1))


def _gate(G):
    T = (G + 1) * (G + 2) // 2
    return (T * T + 6 * G + 64) * 2.0 ** -53


def _gates(markets, G):
    return _gate(G) * _wmax(PR.weights_of(markets, G), G)   # g_p [K]


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
        LARGEST[key] = max(LARGEST.get(key, (0.0, "")), ((e / gate).max(), tag))
    for key, (e, gate) in err.items():
        assert (e <= gate).all(), (key, (e / gate).max())


def _check(m, d, G, markets, split, quantiles=QS, tag=""):
    got = m.predict_periods(d, markets, split=split, max_goals=G, quantiles=quantiles, return_draws=True)
    ref = PR.predict_periods(m, d, markets, split, G, quantiles)
    n = len(d["home_team"])
    assert got["kind"] == "periods" and got["n"] == n and got["markets"] == tuple(markets)
    np.testing.assert_array_equal(got["quantiles"], np.asarray(quantiles, dtype=np.float64))
    np.testing.assert_array_equal(got["split"], np.broadcast_to(np.asarray(split, dtype=np.float64), (n,)))
    _compare(got, ref, _gates(markets, G), tag)
    return got, ref


# 1
@pytest.mark.parametrize("G", [1, 2, 9])
@pytest.mark.parametrize("kind", LR.KINDS)
def test_all_classes_against_restatement(kind, G):
    m = LR.hand_model(kind, S=257, T=8, seed=3)
    d = LR.hand_data(m, n=20, seed=4)
    split = np.array([SPLITS[i % len(SPLITS)] for i in range(20)])
    _check(m, d, G, _markets(G), split, tag=f"{kind} G={G}")


# 2
@pytest.mark.parametrize("G", [0, BLOCK - 1, BLOCK, BLOCK + 1])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("S", [1, 63, 64, 65])
@pytest.mark.parametrize("kind", ["basic", "wc"])
def test_shape_edges(kind, S, n, G):
    m = LR.hand_model(kind, S=S, T=6, seed=S)
    d = LR.hand_data(m, n=n, seed=n)
    split = np.array([SPLITS[(i + G) % len(SPLITS)] for i in range(n)])
    full = _markets(G, K=32, seed=G)
    # one restatement for the 32 markets; K < 32 takes its first K (the passes of K_PASS: 1, full, full + 1, all)
    ref = PR.predict_periods(m, d, full, split, G, QS)
    g = _gates(full, G)
    for K in (1, K_PASS, K_PASS + 1, 32):
        got = m.predict_periods(d, dict(list(full.items())[:K]), split=split, max_goals=G, quantiles=QS,
                                return_draws=True)
        _compare(got, {"mean": ref["mean"][:K], "sd": ref["sd"][:K], "quantile": ref["quantile"][:K],
                       "draws": ref["draws"][:, :K]}, g[:K], f"{kind} S={S} n={n} G={G} K={K}")
        if S == 1:
            assert (got["sd"] == 0.0).all()
            assert (got["quantile"] == got["draws"][0][:, None, :]).all()   # every quantile is the single value
    if G == 0:
        # only 0-0 / 0-0 is left: every market that needs a goal is exactly 0
        mk = {"draw_draw": PD.ht_ft("draw", "draw"), "s00": PD.full_time(MK.correct_score(0, 0)),
              "ht_home": PD.first_period("home"), "either": PD.win_either_period("away"),
              "score_both": PD.score_in_both_periods("home"), "second_highest": PD.highest_scoring_period("second"),
              "comeback": PD.comeback("home"), "second_goals": PD.second_period(MK.total_goals())}
        r = m.predict_periods(d, mk, split=split, max_goals=0, return_draws=True)
        assert (r["draws"][:, 0] > 0.0).all() and r["draws"][:, 0].tobytes() == r["draws"][:, 1].tobytes()
        assert (r["draws"][:, 2:] == 0.0).all() and (r["quantile"][2:] == 0.0).all()


def test_largest_grid():
    # G = 31: T^2 = 278 784 cells, four blocks of second-period away counts
    m = LR.hand_model("neutral", S=2, T=4, seed=5)
    d = LR.hand_data(m, n=2, seed=6)
    _check(m, d, 31, {"second_highest": PD.highest_scoring_period("second")}, np.array([0.45, 1.0 / 3.0]), tag="G=31")


# 3
RHOS = (-2.0, -1.0, -0.5, 0.01, 0.5, 1.0, 5.0)


def _tau_model():
    """Draws with rho below, at and above the clip of every tau cell: on the even draws the fixture t00 - t01 has
    lh = la = 1 exactly, so 1 - rho lh la and 1 - rho are 0 at rho = 1 and 1 + rho lh, 1 + rho la at rho = -1."""
    S = 70
    m = LR.hand_model("basic", S=S, T=4, seed=2)
    m.attack[:, :2] = 0.0
    m.defence[:, :2] = 0.0
    m.home_advantage = np.where(np.arange(S) % 2 == 0, 0.0, m.home_advantage)
    m.corr_coef = np.array([RHOS[s % len(RHOS)] for s in range(S)])
    return m


@pytest.mark.parametrize("f", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("G", [1, 2])
def test_tau_cells(G, f):
    m = _tau_model()
    d = {"home_team": ["t00", "t01", "t02", "t03"], "away_team": ["t01", "t02", "t03", "t00"]}
    combos = [(a, b, x, y) for a, b, x, y in itertools.product(range(2), repeat=4) if a <= x and b <= y]
    assert len(combos) == 9
    mk = {f"{a}{b}_{x}{y}": PD.all_of(PD.first_period(MK.correct_score(a, b)), PD.full_time(MK.correct_score(x, y)))
          for a, b, x, y in combos}
    got, ref = _check(m, d, G, mk, f, tag=f"tau G={G} f={f:g}")
    for key in ARRAYS:
        assert (got[key] >= 0.0).all(), key   # non-negative weights: nothing negative
    # a clipped cell's markets are exactly 0 in the draws that clip it (the restatement's factor is an exact 0)
    lh, la = SR.rates(m, d)
    rho = m.corr_coef[:, None]
    factor = {(0, 0): 1.0 - rho * lh * la, (0, 1): 1.0 + rho * lh, (1, 0): 1.0 + rho * la, (1, 1): 1.0 - rho + 0.0 * lh}
    clipped_any = 0
    for k, (a, b, x, y) in enumerate(combos):
        clipped = factor[(x, y)] <= 0.0   # [S, n]
        clipped_any += int(clipped.sum())
        assert (got["draws"][:, k][clipped] == 0.0).all(), (a, b, x, y)
        if 0.0 < f < 1.0:
            assert (got["draws"][:, k][factor[(x, y)] > 1e-9] > 0.0).all(), (a, b, x, y)
    assert clipped_any > 0
    assert (factor[(1, 1)][5::7] == 0.0).all() and (factor[(0, 0)][:, 0][12::14] == 0.0).all()   # AT the clip, exactly


# 4
@pytest.mark.parametrize("kind", ["extended", "dynamic"])
def test_against_predict_markets(kind):
    m = LR.hand_model(kind, S=129, T=8, seed=11)
    d = LR.hand_data(m, n=12, seed=12)
    G = 9
    full = dict(MR.all_builders(), first_goal=MK.first_goal("home"))
    want = m.predict_markets(d, full, max_goals=G, quantiles=(), return_draws=True)["draws"]
    gate = (_gate(G) + G_MARKETS) * np.maximum(1.0, np.abs(MR.weights_of(full, G)).reshape(len(full), -1).max(axis=1))
    ones = np.ones((G + 1,) * 4)
    for f in (0.0, 0.37, 1.0):
        mk = {name: PD.full_time(market) for name, market in full.items()}
        mk["ones"] = ones
        mk["ht_draw"], mk["second_draw"] = PD.first_period("draw"), PD.second_period("draw")
        got = m.predict_periods(d, mk, split=f, max_goals=G, quantiles=(), return_draws=True)["draws"]
        err = np.abs(got[:, :len(full)] - want).max(axis=(0, 2))
        print(f"{kind} f={f:g}: full_time markets against predict_markets, error / gate {(err / gate).max():.3e}")
        assert (err <= gate).all(), (err / gate).max()
        i = {name: k for k, name in enumerate(mk)}
        if f == 0.0:   # nothing is scored before the split: it is level then, whatever happens later
            assert got[:, i["ht_draw"]].tobytes() == got[:, i["ones"]].tobytes()
        if f == 1.0:   # nothing is scored after it
            assert got[:, i["second_draw"]].tobytes() == got[:, i["ones"]].tobytes()


# 5
@pytest.mark.parametrize("elapsed", [1.0 / 3.0, 0.5])
@pytest.mark.parametrize("kind", ["basic", "neutral"])
def test_against_predict_in_play(kind, elapsed):
    # exp(log evidence of the state) x the in-play value = the period market 1[a = a0, b = b0] F[x, y]: one law
    m = LR.hand_model(kind, S=129, T=8, seed=21)
    states = ((0, 0), (1, 0), (0, 2), (2, 1))
    d = LR.hand_data(m, n=len(states), seed=22)
    G = 9
    final = {"home_win": MK.home_win(), "over_2.5": MK.total_over(2.5), "goals_home": MK.goals("home")}
    live = dict(d, home_goals=[s[0] for s in states], away_goals=[s[1] for s in states],
                elapsed=[elapsed] * len(states))
    r = m.predict_in_play(live, final, max_goals=G, quantiles=(), reweight=False, return_draws=True)
    want = np.exp(r["draw_log_evidence"])[:, None, :] * r["draws"]   # [S, K, n]
    wmax = np.array([np.abs(mk.weights(G)).max() for mk in final.values()])
    # the evidence is a sum of three log pmfs and a log normaliser, each within a few roundings of its own size:
    # 16 (1 + |l|) 2^-53 in l, which exp turns into that relative error of exp(l) <= 1, plus its own rounding
    lmax = np.abs(r["draw_log_evidence"]).max()
    gate = (_gate(G) + G_MARKETS + (16.0 * (1.0 + lmax) + 2.0) * 2.0 ** -53) * np.maximum(1.0, wmax)
    worst = 0.0
    for i, (a0, b0) in enumerate(states):
        at = np.zeros((G + 1,) * 4)
        at[a0, b0] = 1.0
        mk = {name: at * PD.full_time(market).weights(G) for name, market in final.items()}
        fixture = {k: [v[i]] for k, v in d.items()}
        got = m.predict_periods(fixture, mk, split=elapsed, max_goals=G, quantiles=(), return_draws=True)["draws"]
        err = np.abs(got[:, :, 0] - want[:, :, i]).max(axis=0)
        worst = max(worst, (err / gate).max())
        assert not np.isnan(got).any() and (err <= gate).all(), (a0, b0, (err / gate).max())
    print(f"{kind} elapsed={elapsed:.3g}: against exp(evidence) x predict_in_play, error / gate {worst:.3e}")


# 6
def _bits_equal(a, b, keys=ARRAYS):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("kind", ["wc", "dynamic"])
def test_two_calls_and_permuted_fixtures_are_bit_identical(kind):
    m = LR.hand_model(kind, S=130, T=8, seed=15, G=4)
    d = LR.hand_data(m, n=30, seed=16)
    G = 9
    mk = _markets(G)
    split = np.random.RandomState(18).uniform(0, 1, 30)
    split[:3] = (0.0, 1.0, 0.5)
    a = m.predict_periods(d, mk, split=split, max_goals=G, return_draws=True)
    _bits_equal(a, m.predict_periods(d, mk, split=split, max_goals=G, return_draws=True))
    perm = np.random.RandomState(17).permutation(30)
    shuffled = {k: [v[i] for i in perm] for k, v in d.items()}
    b = m.predict_periods(shuffled, mk, split=split[perm], max_goals=G, return_draws=True)
    _bits_equal({k: np.ascontiguousarray(a[k][..., perm]) for k in ARRAYS}, b)


@pytest.mark.parametrize("kind", ["basic", "neutral"])
def test_chunked_workspace_is_bit_identical(kind):
    m = LR.hand_model(kind, S=130, T=8, seed=3)
    d = LR.hand_data(m, n=13, seed=4)
    G = 9
    mk = _markets(G)
    W = PR.weights_of(mk, G)
    split = np.random.RandomState(19).uniform(0, 1, 13)
    (_, device, kw), = m._fixture_groups(d, with_goals=False)[0]
    whole = device().period_summary(**kw, split=split, max_goals=G, weights=W, quantiles=QS, return_draws=True)
    per_fixture = W.shape[0] * 130 * 8
    for fixtures in (1, 4, 12):   # 13, 4 and 2 chunks
        part = device().period_summary(**kw, split=split, max_goals=G, weights=W, quantiles=QS, return_draws=True,
                                       workspace_bytes=fixtures * per_fixture + 5)
        _bits_equal(whole, part)
    _bits_equal(whole, m.predict_periods(d, mk, split=split, max_goals=G, quantiles=QS, return_draws=True))


# 7
def test_many_draws():
    # 4097 draws: 17 draw tiles of 256 in period_values, 65 values per lane in market_summary
    m = LR.hand_model("neutral", S=4097, T=6, seed=31)
    d = LR.hand_data(m, n=2, seed=32)
    _check(m, d, 15, {"draw_home": PD.ht_ft("draw", "home"), "second_goals": PD.second_period(MK.total_goals())},
           np.array([0.45, 0.5]), quantiles=(0.0, 0.001, 0.25, 0.5, 0.999, 1.0), tag="S=4097")


# 8
def test_library_errors():
    h = np.array([0, 1], dtype=np.uint16)
    f = np.array([0.5, 0.25])
    w = np.ones((2, 3, 3, 3, 3))
    ctx = HipContext(0)

    def fails(code, *args, **kwargs):
        with pytest.raises(BplHipError) as e:
            ctx.period_summary(*args, **kwargs)
        assert e.value.code == code, (e.value.code, args[2:], kwargs)

    fails(BPLHIP_ESTATE, h, h[::-1], f, 2, w)                      # no posterior
    rs = np.random.RandomState(0)
    ctx.predict_set_posterior(rs.normal(0, 0.2, (10, 2)), rs.normal(0, 0.2, (10, 2)), rs.normal(0, 0.1, 10),
                              rs.uniform(-0.05, 0.05, 10))
    fails(BPLHIP_ESTATE, h, h[::-1], f, 2, w, neutral=[0, 1])      # the other form's entry point
    fails(BPLHIP_EINVAL, h, h[::-1], f, 32, np.ones((1, 1)))       # max_goals = 32
    fails(BPLHIP_EINVAL, h, h[::-1], f, -1, np.ones((2, 0)))
    fails(BPLHIP_EINVAL, h[:0], h[:0], f[:0], 2, w)                # no fixture
    fails(BPLHIP_EINVAL, h, h[::-1], f, 2, np.ones((0, 3, 3, 3, 3)))    # K = 0
    fails(BPLHIP_EINVAL, h, h[::-1], f, 1, np.ones((33, 2, 2, 2, 2)))   # K = 33
    fails(BPLHIP_EINVAL, h, h[::-1], f, 2, w, quantiles=np.linspace(0, 1, 17))
    fails(BPLHIP_EINVAL, h, h[::-1], f, 2, w, quantiles=[0.5, 1.5])
    fails(BPLHIP_EINVAL, h, h[::-1], f, 2, w, quantiles=[np.nan])
    for bad in (-0.1, 1.5, np.nan, np.inf):
        fails(BPLHIP_EINVAL, h, h[::-1], np.array([0.5, bad]), 2, w)
    bad = w.copy()
    bad[1, 1, 0, 2, 1] = np.inf                                    # a readable cell
    fails(BPLHIP_EINVAL, h, h[::-1], f, 2, bad)
    bad[1, 1, 0, 2, 1] = np.nan
    fails(BPLHIP_EINVAL, h, h[::-1], f, 2, bad)
    fails(BPLHIP_EINVAL, h, h[::-1], f, 2, w, workspace_bytes=-1)
    fails(BPLHIP_EINVAL, h, h[::-1], f, 2, w, workspace_bytes=2 * 10 * 8 - 1)   # holds no fixture
    unread = w.copy()
    unread[0, 2, 0, 1, 2] = np.inf                                 # a > x: never read
    unread[1, 0, 1, 2, 0] = np.nan                                 # b > y
    good = ctx.period_summary(h, h[::-1], f, 2, w, quantiles=[0.1, 0.9], return_draws=True)
    out = ctx.period_summary(h, h[::-1], f, 2, unread, quantiles=[0.1, 0.9], return_draws=True)
    assert out["mean"].shape == (2, 2) and out["sd"].shape == (2, 2) and out["quantile"].shape == (2, 2, 2)
    assert out["draws"].shape == (10, 2, 2) and np.isfinite(out["draws"]).all()
    _bits_equal(good, out)
    out = ctx.period_summary(h, h[::-1], f, 31, np.ones((1, 32, 32, 32, 32)), workspace_bytes=10 * 8)   # one per chunk
    assert out["quantile"].shape == (1, 0, 2) and "draws" not in out and np.isfinite(out["mean"]).all()
    ctx.close()


# 9
@pytest.mark.parametrize("kind", ["basic", "wc"])
def test_first_goal(kind):
    m = LR.hand_model(kind, S=129, T=8, seed=41)
    d = LR.hand_data(m, n=20, seed=42)
    G = 15
    mk = {"first_home": MK.first_goal("home"), "first_away": MK.first_goal("away"), "s00": MK.correct_score(0, 0),
          "ones": np.ones((G + 1, G + 1))}
    got = m.predict_markets(d, mk, max_goals=G, quantiles=QS, return_draws=True)
    ref = MR.predict_markets(m, d, mk, G, QS)
    g = np.full(len(mk), G_MARKETS)
    for key, gate in (("mean", g), ("sd", 10 * g), ("quantile", g + 2.0 ** -52), ("draws", g)):
        e = np.abs(got[key] - ref[key])
        e = e.max(axis=(0, 2)) if key == "draws" else e.reshape(len(mk), -1).max(axis=1)
        print(f"{kind} first_goal: {key} error / gate {(e / gate).max():.3e}")
        assert (e <= gate).all(), (key, (e / gate).max())
    v = got["draws"]
    err = np.abs(v[:, 0] + v[:, 1] + v[:, 2] - v[:, 3]).max()
    print(f"{kind} first_goal: home + away + 0-0 against all ones {err:.3e}")
    assert err <= 3 * G_MARKETS


def test_zz_largest_errors():
    # (runs last in the module: the maxima of error / gate over the comparisons with the restatement above)
    for key, (ratio, tag) in LARGEST.items():
        print(f"largest {key} error / gate over the module: {ratio:.3e} ({tag})")
        assert ratio <= 1.0
