"""predict_in_play on the device (csrc/dc_inplay.hip.h, bpl/inplay.py) against the numpy restatement
(tests/inplay_ref.py: the full shifted grid of every draw and fixture from closed-form pmfs, Z from a wide grid,
np.argsort, np.cumsum and the crossing rule written out) for the five predictor classes, on shape edges, partial
blocks, reachable and unreachable tau cells, clipped tau, the kick-off identity with predict_markets, exact order
statistics, log weights from sequential_scores, determinism and the library's own errors.

Gates (computed by inplay_ref.gates from the RESTATEMENT's Z): the numerator carries section
16's g = 1e-12 max(1, max|W|) per market, scaled by max(1, Z) (the grid sums to Z, not 1); dividing by Z gives
g max(1, 1/Z) + |val| (e_Z / Z + 3 2^-53) with e_Z = 2^-53 (4 + 204 A) the rounding of the four-term closed form
(A the sum of |f - 1| u v it adds up).  l: 48 roundings relative to lh t + la t + a (|log lh| + |log t|) + ... +
lgamma + |log Z|, 12 (a + b) 2^-53 for the log rates, e_Z / Z, and 40 2^-53 for the restatement's own wide-grid Z.  mean: the value gate plus the weights' relative
error times twice the range of the values, plus S roundings of the sum.  sd: ten value gates (the Lipschitz
argument of section 16) plus the weights' share.  A weighted quantile is 1-Lipschitz in the sup norm of the values
for fixed weights: an unflagged cell is held to the value gate; in a flagged cell (some C_i within 1e-9 W of q W)
either neighbouring order statistic is accepted, and at most 1 % of a test's cells may be flagged."""
import numpy as np
import pytest

import inplay_ref as IR
import loglik_ref as LR
import markets_ref as MR
from bpl import markets as MK
from bpl._ffi import BPLHIP_EINVAL, BPLHIP_ESTATE, BplHipError, HipContext

pytestmark = pytest.mark.gpu

K_PASS = 8   # csrc/dc_inplay.hip.h INPLAY_KPASS
QS = IR.QS
ARRAYS = ("mean", "sd", "quantile", "ess", "log_evidence", "draws", "draw_log_evidence")


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


def _first(ref, K):
    """The restatement of the first K markets of `ref`'s."""
    out = dict(ref)
    for key in ("mean", "sd", "quantile", "flag", "neighbours", "wmax"):
        out[key] = ref[key][:K]
    out["draws"] = ref["draws"][:, :K]
    return out


def _check(m, d, G, markets, quantiles=QS, tag="", **kwargs):
    got = m.predict_in_play(d, markets, max_goals=G, quantiles=quantiles, return_draws=True, **kwargs)
    ref = IR.predict_in_play(m, d, markets, G, quantiles, **kwargs)
    assert got["kind"] == "in_play" and got["n"] == len(d["home_team"]) and got["markets"] == tuple(markets)
    np.testing.assert_array_equal(got["quantiles"], np.asarray(quantiles, dtype=np.float64))
    IR.compare(got, ref, tag)
    _extremes_are_exact(got)
    return got, ref


def _extremes_are_exact(got):
    """q = 0 and q = 1 are the minimum and maximum of the returned draws, bit for bit."""
    q = got["quantiles"]
    for i in np.nonzero(q == 0.0)[0]:
        assert got["quantile"][:, i].tobytes() == got["draws"].min(axis=0).tobytes()
    for i in np.nonzero(q == 1.0)[0]:
        assert got["quantile"][:, i].tobytes() == got["draws"].max(axis=0).tobytes()


# 1
@pytest.mark.parametrize("G", [1, 2, 15])
@pytest.mark.parametrize("kind", LR.KINDS)
def test_all_classes_against_restatement(kind, G):
    m = LR.hand_model(kind, S=257, T=8, seed=3)
    d = IR.with_states(LR.hand_data(m, n=130, seed=4), G, seed=5)
    got, ref = _check(m, d, G, _markets(G), tag=f"{kind} G={G}")
    assert (got["ess"] <= 257.0 * (1 + 1e-12)).all() and (got["ess"] >= 1.0).all()
    assert (ref["flag"].sum() == 0)


# 2
@pytest.mark.parametrize("G", [0, 1, 8, 9, 16, 63])
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 257])
def test_draw_edges(S, G):
    kind = ("basic", "wc")[(S + G) % 2]
    m = LR.hand_model(kind, S=S, T=6, seed=S)
    d = IR.with_states(LR.hand_data(m, n=5, seed=G), G, seed=S + G)
    full = _markets(G, K=K_PASS + 1, seed=G)
    ref = IR.predict_in_play(m, d, full, G, QS)
    for K in (1, K_PASS, K_PASS + 1):   # the passes of K_PASS: a part of one, a full one, one more
        got = m.predict_in_play(d, dict(list(full.items())[:K]), max_goals=G, quantiles=QS, return_draws=True)
        IR.compare(got, _first(ref, K), f"{kind} S={S} G={G} K={K}")
        _extremes_are_exact(got)
        if S == 1:
            assert (got["sd"] == 0.0).all() and (got["ess"] == 1.0).all()
            assert (got["quantile"] == got["draws"][0][:, None, :]).all()   # every quantile is the single value
            assert got["log_evidence"].tobytes() == got["draw_log_evidence"][0].tobytes()


@pytest.mark.parametrize("G", [0, 9, 63])
@pytest.mark.parametrize("n", [1, 64, 65])
def test_fixture_edges(n, G):
    kind = ("neutral", "extended", "dynamic")[(n + G) % 3]
    m = LR.hand_model(kind, S=65, T=6, seed=n)
    d = IR.with_states(LR.hand_data(m, n=n, seed=G + 1), G, seed=n + G)
    mk = _markets(G, K=K_PASS + 1, seed=n)
    _check(m, d, G, mk, tag=f"{kind} n={n} G={G}")


# 3
@pytest.mark.parametrize("G", [9, 16])
def test_partial_blocks_single_cells_and_tau_cells(G):
    """The y blocks start at b: G - b + 1 = 1, 7, 8, 9 cells (a partial last block, a full one, a block boundary),
    the single-cell grids a = G and b = G, every (a, b) in {0, 1, 2}^2 (tau cells reachable, partly, not), and
    elapsed 0 (with 0-0), 0.5 and 0.999."""
    states = [(0, G, 0.5), (1, G - 6, 0.5), (2, G - 7, 0.5), (0, G - 8, 0.5), (G, 0, 0.5), (G, G, 0.5), (G, G, 0.999),
              (G, 1, 0.999), (0, 0, 0.0), (0, 0, 0.999)]
    states += [(a, b, t) for a in range(3) for b in range(3) for t in (0.5, 0.999)]
    m = LR.hand_model("wc", S=257, T=8, seed=21)
    d = IR.with_state_list(LR.hand_data(m, n=len(states), seed=22), states)
    mk = _markets(G)
    for a, b in ((0, 0), (0, 1), (1, 1), (1, 2), (2, 2), (G, G), (0, G), (G, 0)):
        mk[f"score_{a}_{b}"] = MK.correct_score(a, b)
    got, _ = _check(m, d, G, mk, tag=f"states G={G}")
    i = {name: k for k, name in enumerate(mk)}
    at = states.index((G, G, 0.5))
    # a = b = G: the grid is the one cell (G, G); every market is its weight times that cell
    assert got["draws"][:, i[f"score_{G}_{G}"], at].tobytes() == got["draws"][:, i["draw"], at].tobytes()
    assert (got["draws"][:, i["home_win"], at] == 0.0).all() and (got["draws"][:, i["btts"], at] > 0.0).all()
    # a score that is behind the state has no mass
    for n, (a, b, _) in enumerate(states):
        for x, y in ((0, 0), (0, 1), (1, 1), (1, 2)):
            if x < a or y < b:
                assert (got["draws"][:, i[f"score_{x}_{y}"], n] == 0.0).all(), (a, b, x, y)


# 4
def test_clipped_tau_is_an_exact_zero_and_Z_stays_positive():
    m = LR.hand_model("basic", S=64, T=4, seed=2)
    m.corr_coef = np.where(np.arange(64) % 3 == 0, 5.0, 0.01)   # 1 - rho lh la < 0 and 1 - rho < 0 on some draws
    states = [(0, 0, 0.0), (0, 0, 0.5), (0, 1, 0.5), (1, 0, 0.5), (1, 1, 0.5), (1, 1, 0.999), (2, 0, 0.5), (0, 0, 0.999)]
    n = len(states)
    d = IR.with_state_list({"home_team": ["t00", "t01", "t02", "t03"] * 2, "away_team": ["t01", "t02", "t03", "t00"] * 2},
                           states)
    for G in (1, 15):
        mk = MR.all_builders()
        mk["score_0_0"], mk["score_1_1"], mk["score_0_1"] = (MK.correct_score(0, 0), MK.correct_score(1, 1),
                                                             MK.correct_score(0, 1))
        got, ref = _check(m, {k: (v if G == 15 else _cap(k, v, G)) for k, v in d.items()}, G, mk, tag=f"clipped G={G}")
        assert (ref["Z"] > 0.0).all() and np.isfinite(got["draw_log_evidence"]).all()
        for key in ARRAYS:
            if key != "draw_log_evidence" and key != "log_evidence":
                assert (got[key] >= 0.0).all(), key   # non-negative weights: nothing negative
        assert (got["draws"][::3, got["markets"].index("score_1_1")] == 0.0).all()   # a clipped cell is an exact 0
        assert got["draws"].shape[2] == n


def _cap(key, v, G):
    return np.minimum(v, G) if key in ("home_goals", "away_goals") else v


# 5
@pytest.mark.parametrize("kind", LR.KINDS)
def test_kick_off_is_predict_markets(kind):
    """elapsed = 0 at 0-0 without re-weighting, unclipped rho: the values are predict_markets' (the unclipped tau
    sums to one: Z = 1 up to its rounding), within 2 g; the log evidence of the state is log Z = 0 within its gate."""
    G = 15
    m = LR.hand_model(kind, S=257, T=8, seed=11)
    m.corr_coef = 0.2 * m.corr_coef   # |rho| <= 0.02: no cell is clipped (asserted below)
    d = IR.with_states(LR.hand_data(m, n=40, seed=12), 0, seed=1, elapsed=0.0)
    mk = _markets(G)
    got, ref = _check(m, d, G, mk, reweight=False, tag=f"{kind} kick-off")
    rho = np.asarray(m.corr_coef)[:, None]
    assert (1.0 - np.abs(rho) * np.maximum(ref["lh"] * ref["la"], np.maximum(ref["lh"], ref["la"])) > 0.0).all()
    pre = m.predict_markets(d, mk, max_goals=G, quantiles=QS, return_draws=True)
    g = 1e-12 * np.maximum(1.0, ref["wmax"])
    err = np.abs(got["draws"] - pre["draws"]).max(axis=(0, 2))
    print(f"{kind}: kick-off draws against predict_markets, error / 2 g {(err / (2 * g)).max():.3e}")
    assert (err <= 2 * g).all()
    lev = np.abs(got["draw_log_evidence"]) / IR.gates(ref)["draw_log_evidence"]
    print(f"{kind}: kick-off log evidence against 0, error / gate {lev.max():.3e}")
    assert lev.max() <= 1.0
    assert np.abs(got["ess"] - 257.0).max() <= 257 * 1e-13


# 6
@pytest.mark.parametrize("S", [1, 257, 1001])
def test_equal_weights_are_numpys_inverted_cdf_bit_for_bit(S):
    m = LR.hand_model("extended", S=S, T=8, seed=41)
    d = IR.with_states(LR.hand_data(m, n=20, seed=42), 15, seed=43)
    mk = _markets(15)
    qs = (0.0, 0.05, 0.3, 0.5, 0.95, 1.0) if S != 1001 else (0.0, 0.0513, 0.3, 0.4999, 0.95, 1.0)
    r = m.predict_in_play(d, mk, quantiles=qs, reweight=False, return_draws=True)
    want = np.quantile(r["draws"], qs, axis=0, method="inverted_cdf").transpose(1, 0, 2)
    assert r["quantile"].tobytes() == np.ascontiguousarray(want).tobytes()
    # q = 0 and q = 1 in every mode
    lw = np.random.RandomState(44).normal(0.0, 2.0, S)
    for kwargs in ({}, {"log_weights": lw}, {"reweight": False, "log_weights": lw}):
        _extremes_are_exact(m.predict_in_play(d, mk, quantiles=(0.0, 1.0, 0.5), return_draws=True, **kwargs))


# 7
@pytest.mark.parametrize("kind", ["basic", "dynamic"])
def test_log_weights_from_sequential_scores(kind):
    m = LR.hand_model(kind, S=257, T=8, seed=51)
    played = LR.hand_data(m, n=30, seed=52)
    block = np.repeat(np.arange(3), 10)
    lw = m.sequential_scores(played, block, return_weights=True)["log_weights"]
    assert lw.shape == (3, 257)
    d = IR.with_states(LR.hand_data(m, n=30, seed=53), 15, seed=54)
    mk = _markets(15, K=5)
    for b in (1, 2):
        for reweight in (False, True):
            got, ref = _check(m, d, 15, mk, reweight=reweight, log_weights=lw[b], tag=f"{kind} block {b} reweight={reweight}")
    # the updated-without-a-refit forecast: kick-off states under the block's weights differ from the unweighted one
    ko = IR.with_states(d, 0, seed=1, elapsed=0.0)
    a = m.predict_in_play(ko, mk, reweight=False, log_weights=lw[2])
    b = m.predict_in_play(ko, mk, reweight=False)
    assert np.abs(a["mean"] - b["mean"]).max() > 1e-6 and (a["ess"] < b["ess"]).all()
    assert a["log_evidence"].tobytes() == b["log_evidence"].tobytes()   # from l alone


# 8
def _bits_equal(a, b, keys=ARRAYS):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("kind", ["wc", "dynamic"])
def test_two_calls_and_permuted_fixtures_are_bit_identical(kind):
    m = LR.hand_model(kind, S=300, T=8, seed=15, G=4)
    d = IR.with_states(LR.hand_data(m, n=90, seed=16), 15, seed=17)
    mk = _markets(15)
    lw = np.random.RandomState(18).normal(0.0, 1.0, 300)
    a = m.predict_in_play(d, mk, quantiles=QS, log_weights=lw, return_draws=True)
    _bits_equal(a, m.predict_in_play(d, mk, quantiles=QS, log_weights=lw, return_draws=True))
    perm = np.random.RandomState(19).permutation(90)
    shuffled = {k: [v[i] for i in perm] for k, v in d.items()}
    b = m.predict_in_play(shuffled, mk, quantiles=QS, log_weights=lw, return_draws=True)
    _bits_equal({k: np.ascontiguousarray(a[k][..., perm]) for k in ARRAYS}, b)


@pytest.mark.parametrize("kind", ["basic", "neutral"])
def test_chunked_workspace_is_bit_identical(kind):
    m = LR.hand_model(kind, S=257, T=8, seed=3)
    d = IR.with_states(LR.hand_data(m, n=130, seed=4), 15, seed=5)
    G, mk = 15, _markets(15)
    W = MR.weights_of(mk, G)
    (_, device, kw), = m._fixture_groups(d, with_goals=True)[0]
    t = np.asarray(d["elapsed"])
    whole = device().inplay_summary(**kw, elapsed=t, max_goals=G, weights=W, quantiles=QS, return_draws=True)
    per_fixture = (W.shape[0] + 1) * 257 * 8
    for fixtures in (1, 7, 43, 129):   # 130, 19, 4 and 2 chunks
        part = device().inplay_summary(**kw, elapsed=t, max_goals=G, weights=W, quantiles=QS, return_draws=True,
                                       workspace_bytes=fixtures * per_fixture + 5)
        _bits_equal(whole, part)
    _bits_equal(whole, m.predict_in_play(d, mk, max_goals=G, quantiles=QS, return_draws=True))


# 9
def test_many_draws_sort_in_lds():
    # 12 288 draws, the most: 48 sorted positions per thread, 144 KiB of dynamic LDS
    m = LR.hand_model("neutral", S=12288, T=6, seed=31)
    d = IR.with_states(LR.hand_data(m, n=2, seed=32), 15, seed=33)
    _check(m, d, 15, {"over_2.5": MK.total_over(2.5), "goals_home": MK.goals("home")},
           quantiles=(0.0, 0.001, 0.25, 0.5, 0.95, 0.999, 1.0), tag="S=12288")


# 10
def test_library_errors():
    h = np.array([0, 1], dtype=np.uint16)
    x = np.array([1, 0], dtype=np.uint16)
    t = np.array([0.5, 0.25])
    w = np.ones((2, 16, 16))
    ctx = HipContext(0)

    def fails(code, *args, **kwargs):
        with pytest.raises(BplHipError) as e:
            ctx.inplay_summary(*args, **kwargs)
        assert e.value.code == code, (e.value.code, args[4:], kwargs)

    fails(BPLHIP_ESTATE, h, h[::-1], x, x, t, 15, w)                       # no posterior
    rs = np.random.RandomState(0)
    ctx.predict_set_posterior(rs.normal(0, 0.2, (10, 2)), rs.normal(0, 0.2, (10, 2)), rs.normal(0, 0.1, 10),
                              rs.uniform(-0.05, 0.05, 10))
    fails(BPLHIP_ESTATE, h, h[::-1], x, x, t, 15, w, neutral=[0, 1])       # the other form's entry point
    fails(BPLHIP_EINVAL, h, h[::-1], x, x, t, 64, np.ones((2, 65, 65)))
    fails(BPLHIP_EINVAL, h, h[::-1], x, x, t, -1, np.ones((2, 0, 0)))
    fails(BPLHIP_EINVAL, h[:0], h[:0], x[:0], x[:0], t[:0], 15, w)         # no fixture
    fails(BPLHIP_EINVAL, h, h[::-1], x, x, t, 15, np.ones((0, 16, 16)))    # K = 0
    fails(BPLHIP_EINVAL, h, h[::-1], x, x, t, 15, np.ones((65, 16, 16)))   # K = 65
    fails(BPLHIP_EINVAL, h, h[::-1], x, x, t, 15, w, quantiles=np.linspace(0, 1, 17))
    fails(BPLHIP_EINVAL, h, h[::-1], x, x, t, 15, w, quantiles=[0.5, 1.5])
    fails(BPLHIP_EINVAL, h, h[::-1], x, x, t, 15, w, quantiles=[np.nan])
    bad = w.copy()
    bad[1, 3, 4] = np.inf
    fails(BPLHIP_EINVAL, h, h[::-1], x, x, t, 15, bad)
    for e in (1.0, -0.25, 1.5, np.nan, np.inf):
        fails(BPLHIP_EINVAL, h, h[::-1], x, x, np.array([0.5, e]), 15, w)  # elapsed outside [0, 1)
    fails(BPLHIP_EINVAL, h, h[::-1], np.array([16, 0], dtype=np.uint16), x, t, 15, w)    # beyond max_goals
    fails(BPLHIP_EINVAL, h, h[::-1], x, np.array([0, 3], dtype=np.uint16), t, 2, np.ones((2, 3, 3)))
    fails(BPLHIP_EINVAL, h, h[::-1], x, x, np.array([0.0, 0.5]), 15, w)    # 1-0 at elapsed = 0
    for e in (np.nan, np.inf, -np.inf):
        fails(BPLHIP_EINVAL, h, h[::-1], x, x, t, 15, w, log_weights=np.where(np.arange(10) == 4, e, 0.0))
    fails(BPLHIP_EINVAL, h, h[::-1], x, x, t, 15, w, workspace_bytes=-1)
    fails(BPLHIP_EINVAL, h, h[::-1], x, x, t, 15, w, workspace_bytes=3 * 10 * 8 - 1)   # holds no fixture
    out = ctx.inplay_summary(h, h[::-1], x, x, t, 63, np.ones((3, 64, 64)), quantiles=[0.1, 0.9], return_draws=True)
    assert out["mean"].shape == (3, 2) and out["sd"].shape == (3, 2) and out["quantile"].shape == (3, 2, 2)
    assert out["ess"].shape == (2,) and out["log_evidence"].shape == (2,)
    assert out["draws"].shape == (10, 3, 2) and out["draw_log_evidence"].shape == (10, 2)
    assert all(np.isfinite(v).all() for v in out.values())
    out = ctx.inplay_summary(h, h[::-1], x * 0, x * 0, t * 0, 15, w, workspace_bytes=3 * 10 * 8)   # one fixture per chunk
    assert out["quantile"].shape == (2, 0, 2) and "draws" not in out
    # more draws than the sort holds in LDS
    ctx.predict_set_posterior(np.zeros((12289, 2)), np.zeros((12289, 2)), np.zeros(12289), np.zeros(12289))
    fails(BPLHIP_EINVAL, h, h[::-1], x, x, t, 15, w)
    ctx.close()
