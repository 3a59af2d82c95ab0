"""forecast_scores on the device (csrc/dc_score.hip.h, bpl/scoring.py) against the numpy restatement
(tests/scores_ref.py: the full scoreline grid of every draw and fixture, a different route from the
kernel's O(G) walk) for the five predictor classes, against the existing predict kernels, and on shape
edges, determinism and the library's own errors.

Tolerances: a per-draw probability is the result of fewer than ~600 float64
operations on quantities <= 1, each adding at most 2^-53 relative: outcome_proba within 1e-12 absolute,
the Brier and ranked probability scores within 1e-11, a log score within 1e-12 / p + 1e-12 for the
restatement's probability p of the observed class (the per-draw means: the mean of that bound)."""
import numpy as np
import pytest

import loglik_ref as LR
import scores_ref as SR
from bpl._ffi import BPLHIP_EINVAL, BPLHIP_ESTATE, BplHipError, HipContext

pytestmark = pytest.mark.gpu

NAMES = ("log_score", "brier", "rps")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _check(m, d, G, min_p=None):
    """forecast_scores(d, G) against the restatement; returns (result, restatement)."""
    got = m.forecast_scores(d, max_goals=G)
    ref = SR.scores(m, d, G)
    p = ref["p_draws"]
    if min_p is not None:
        print(f"max_goals={G}: least per-draw class probability {p.min():.3e}")
        assert p.min() >= min_p, p.min()
    for k, v in got.items():
        if k not in ("kind", "calibration"):
            assert not np.isnan(np.asarray(v, dtype=np.float64)).any(), k
    assert got["n"] == ref["n"]
    np.testing.assert_array_equal(got["outcome"], ref["outcome"])
    o = ref["outcome"].astype(np.int64)
    err = np.abs(got["outcome_proba"] - ref["outcome_proba"]).max()
    print(f"max_goals={G}: outcome_proba error {err:.3e}")
    assert err <= 1e-12, err
    for name in ("brier", "rps"):
        for suffix in ("_i", "_draws"):
            err = np.abs(got[name + suffix] - ref[name + suffix]).max()
            print(f"max_goals={G}: {name}{suffix} error {err:.3e}")
            assert err <= 1e-11, (name + suffix, err)
        assert abs(got[name] - ref[name]) <= 1e-11 and abs(got[name + "_se"] - ref[name + "_se"]) <= 1e-11
    # the log scores: exact where the restatement's probability is 0 (-inf), else within 1e-12 / p + 1e-12
    P_o = ref["outcome_proba"][np.arange(o.size), o]
    p_o = p[:, np.arange(o.size), o]
    zero = P_o == 0.0
    np.testing.assert_array_equal(got["log_score_i"][zero], ref["log_score_i"][zero])
    with np.errstate(divide="ignore"):
        bound_i = 1e-12 / P_o + 1e-12
        bound_draws = (1e-12 / p_o + 1e-12).mean(axis=1)
    err = np.abs(got["log_score_i"][~zero] - ref["log_score_i"][~zero])
    assert (err <= bound_i[~zero]).all(), err.max()
    dead = (p_o == 0.0).any(axis=1)   # draws with a -inf log score somewhere
    np.testing.assert_array_equal(got["log_score_draws"][dead], ref["log_score_draws"][dead])
    err = np.abs(got["log_score_draws"][~dead] - ref["log_score_draws"][~dead])
    print(f"max_goals={G}: log_score_draws error {err.max() if err.size else 0.0:.3e}")
    assert (err <= bound_draws[~dead]).all(), err.max()
    if zero.any():
        assert got["log_score"] == -np.inf and got["log_score_se"] == (np.inf if o.size > 1 else 0.0)
    else:
        assert abs(got["log_score"] - ref["log_score"]) <= bound_i.mean()
    return got, ref


@pytest.mark.parametrize("G", [1, 2, 15])
@pytest.mark.parametrize("kind", LR.KINDS)
def test_all_classes_against_restatement(kind, G):
    m = LR.hand_model(kind, S=257, T=8, seed=3)
    d = LR.hand_data(m, n=130, seed=4)
    _check(m, d, G, min_p=1e-5)


@pytest.mark.parametrize("G", [0, 16, 63])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65])
@pytest.mark.parametrize("kind", ["basic", "wc"])
def test_shape_edges(kind, S, n, G):
    m = LR.hand_model(kind, S=S, T=6, seed=S)
    d = LR.hand_data(m, n=n, seed=n)
    got, ref = _check(m, d, G)
    if G == 0:
        # only 0-0 is on the grid: the draw class alone has mass
        assert (got["outcome_proba"][:, [0, 2]] == 0.0).all() and (got["outcome_proba"][:, 1] > 0.0).all()
        lost = got["outcome"] != 1
        assert (got["log_score_i"][lost] == -np.inf).all() and np.isfinite(got["log_score_i"][~lost]).all()
        if lost.any():
            assert (got["log_score_draws"] == -np.inf).all()


def test_draw_and_fixture_tiles_beyond_one_block():
    # 513 draws: five draw tiles of 128, a second workgroup row; 300 fixtures: three fixture tiles
    m = LR.hand_model("neutral", S=513, T=8, seed=21)
    d = LR.hand_data(m, n=300, seed=22)
    _check(m, d, 15)


def test_outcomes_come_from_the_actual_goals():
    m = LR.hand_model("basic", S=64, T=4, seed=5)
    d = {"home_team": ["t00", "t01", "t02"], "away_team": ["t01", "t02", "t03"], "home_goals": [70, 255, 3],
         "away_goals": [90, 0, 3]}
    got, _ = _check(m, d, 2)
    np.testing.assert_array_equal(got["outcome"], [2, 0, 1])
    assert np.isfinite(got["log_score_i"]).all()


def test_clipped_tau_agrees_and_has_no_nan():
    m = LR.hand_model("basic", S=64, T=4, seed=2)
    m.corr_coef = np.where(np.arange(64) % 3 == 0, 5.0, 0.01)   # 1 - rho lh la < 0 and 1 - rho < 0 on some draws
    d = {"home_team": ["t00", "t01", "t02", "t03"], "away_team": ["t01", "t02", "t03", "t00"],
         "home_goals": [0, 1, 2, 1], "away_goals": [0, 1, 2, 0]}
    for G in (0, 1, 15):
        _check(m, d, G)


def _public_outcome_proba(kind, m, d, G):
    """predict_outcome_proba of the class on the fixtures of d, [n, 3]."""
    h, a = list(d["home_team"]), list(d["away_team"])
    if kind in ("basic", "extended"):
        out = m.predict_outcome_proba(h, a, max_goals=G)
    elif kind == "neutral":
        out = m.predict_outcome_proba(h, a, np.asarray(d["neutral_venue"]), max_goals=G)
    elif kind == "wc":
        out = m.predict_outcome_proba(h, a, list(d["home_conf"]), list(d["away_conf"]),
                                      np.asarray(d["neutral_venue"]), max_goals=G)
    else:
        gw, nv = np.asarray(d["gameweek"]), np.asarray(d["neutral_venue"])
        out = {k: np.empty(len(h)) for k in ("home_win", "draw", "away_win")}
        for g in np.unique(gw):
            pos = np.nonzero(gw == g)[0]
            part = m.predict_outcome_proba([h[i] for i in pos], [a[i] for i in pos], nv[pos], gameweek=int(g))
            for k in out:
                out[k][pos] = part[k]
    return np.stack([out["home_win"], out["draw"], out["away_win"]], axis=1)


@pytest.mark.parametrize("kind", LR.KINDS)
def test_outcome_proba_is_predict_outcome_proba(kind):
    # the float32 grid's gate of tests/test_gpu_fit.py: 3e-6 (the dynamic class predicts at depth 15 only)
    m = LR.hand_model(kind, S=500, T=8, seed=11)
    d = LR.hand_data(m, n=64, seed=12)
    for G in (15,) if kind == "dynamic" else (15, 4):
        got = m.forecast_scores(d, max_goals=G)["outcome_proba"]
        err = np.abs(got - _public_outcome_proba(kind, m, d, G)).max()
        print(f"{kind} max_goals={G}: against predict_outcome_proba {err:.3e}")
        assert err < 3e-6, err


@pytest.mark.parametrize("kind", LR.KINDS)
def test_single_draw_log_score_is_the_grid_class_sum(kind):
    # one draw: the forecast IS that draw's p, so exp(log_score_i) is the observed class's triangle of the
    # scoreline grid (float32 cells within 3e-6 relative, test_gpu_fit.py: a class sum <= 1 within 3e-6)
    m = LR.hand_model(kind, S=1, T=8, seed=17)
    d = LR.hand_data(m, n=40, seed=18)
    G = 15
    got = m.forecast_scores(d, max_goals=G)
    xs, ys = np.meshgrid(np.arange(G + 1), np.arange(G + 1), indexing="ij")
    masks = [xs > ys, xs == ys, xs < ys]
    groups, _ = m._loglik_groups(d)
    want = np.empty(40)
    for positions, device, kw in groups:
        at = np.arange(40) if positions is None else positions
        grid = device().predict_score_grid(kw["home_idx"], kw["away_idx"], G, neutral=kw.get("neutral"),
                                           conf=kw.get("conf"))
        for j, i in enumerate(at):
            want[i] = grid[j][masks[got["outcome"][i]]].sum()
    err = np.abs(np.exp(got["log_score_i"]) - want).max()
    print(f"{kind}: exp(log_score_i) against the grid's class sums {err:.3e}")
    assert err < 3e-6, err
    assert abs(got["log_score_draws"][0] - got["log_score"]) <= 1e-12   # one draw: the same numbers


def test_two_calls_are_bit_identical():
    m = LR.hand_model("wc", S=1000, T=12, seed=13)
    d = LR.hand_data(m, n=300, seed=14)
    a, b = m.forecast_scores(d), m.forecast_scores(d)
    for k in a:
        if k not in ("kind", "n", "calibration"):
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    for k in a["calibration"]:
        assert a["calibration"][k].tobytes() == b["calibration"][k].tobytes(), k


def test_dynamic_shuffled_fixtures_permute_the_results():
    m = LR.hand_model("dynamic", S=300, T=8, seed=15, G=4)
    d = LR.hand_data(m, n=90, seed=16)
    perm = np.random.RandomState(17).permutation(90)
    shuffled = {k: [v[i] for i in perm] for k, v in d.items()}
    a, b = m.forecast_scores(d), m.forecast_scores(shuffled)
    for k in ("outcome", "outcome_proba", "log_score_i", "brier_i", "rps_i"):
        assert a[k][perm].tobytes() == b[k].tobytes(), k
    # the per-draw sums run over the fixtures in another order: equal up to rounding
    for name in NAMES:
        np.testing.assert_allclose(b[name + "_draws"], a[name + "_draws"], rtol=1e-13, atol=0)


def test_library_errors():
    h = np.array([0, 1], dtype=np.uint16)
    ctx = HipContext(0)
    with pytest.raises(BplHipError) as e:
        ctx.outcome_scores(h, h[::-1], h, h, 15)          # no posterior
    assert e.value.code == BPLHIP_ESTATE
    rs = np.random.RandomState(0)
    ctx.predict_set_posterior(rs.normal(0, 0.2, (10, 2)), rs.normal(0, 0.2, (10, 2)), rs.normal(0, 0.1, 10),
                              rs.uniform(-0.05, 0.05, 10))
    for G in (64, -1):
        with pytest.raises(BplHipError) as e:
            ctx.outcome_scores(h, h[::-1], h, h, G)
        assert e.value.code == BPLHIP_EINVAL
    with pytest.raises(BplHipError) as e:
        ctx.outcome_scores(h[:0], h[:0], h[:0], h[:0], 15)   # no fixture
    assert e.value.code == BPLHIP_EINVAL
    with pytest.raises(BplHipError) as e:
        ctx.outcome_scores(h, h[::-1], h, h, 15, neutral=[0, 1])   # the other form's entry point
    assert e.value.code == BPLHIP_ESTATE
    out = ctx.outcome_scores(h, h[::-1], h, h, 63)
    assert out["proba"].shape == (2, 3) and out["draw_sums"].shape == (10, 3)
    ctx.close()
