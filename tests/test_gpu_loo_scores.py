"""loo_scores on the device (csrc/dc_loo.hip.h, bpl/loo_scores.py) against the numpy restatement
(tests/loo_scores_ref.py: the full log-likelihood matrix, a full sort, the full scoreline grids) for the five
predictor classes; agreement with loo and forecast_scores; two draws by hand; identical, tied and clipped draws;
bit identity; the query record's own errors.

Gates (DESIGN.md sections 12, 15, 17 and 32): tail_len exactly; pareto_k, ess and elpd_loo_i within
1e-9 (1 + |value|), exactly equal where the restatement is infinite; outcome_proba, pit_home and pit_away within
1e-9 absolute (the weights carry the 1e-9); Brier and RPS within 1e-8; a log score within 1e-9 / p + 1e-9;
outcome_proba_in_sample within 1e-12.  Draw counts 2, 10 (no smoothing), 64, 100 (not a multiple of the wave) and
700 (a tail longer than a wave); 1 and 50 fixtures (50 is not a multiple of the 4 waves of a workgroup); grids of
0, 1, 6, 15 and 63 goals under data with up to 6; hand_model's own spread (Pareto k up to about 1.6) and the
narrow one of loo_scores_ref.narrow (k mostly below 0.7); r_eff 1 and 0.3."""
import numpy as np
import pytest

import loglik_ref as LR
import loo_scores_ref as OR
import scores_ref as SR
from bpl import compare_scores
from bpl._ffi import BPLHIP_EINVAL, BPLHIP_ESTATE, BplHipError, HipContext

pytestmark = pytest.mark.gpu

DRAWS, GRIDS = (2, 10, 64, 100, 700), (0, 1, 6, 15, 63)
WORST = {}   # the largest error of each gated quantity, as a fraction of its gate (printed by every check)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _gate(name, got, want, bound):
    """|got - want| <= bound elementwise where want is finite; exact where it is infinite."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert not np.isnan(got).any(), name
    fin = np.isfinite(want)
    np.testing.assert_array_equal(got[~fin], want[~fin], err_msg=name)
    bound = np.broadcast_to(bound, want.shape)
    err = np.abs(got[fin] - want[fin])
    frac = float((err / bound[fin]).max()) if err.size else 0.0
    WORST[name] = max(WORST.get(name, 0.0), frac)
    print(f"{name}: largest error {err.max() if err.size else 0.0:.3e}, {frac:.3e} of its gate")
    assert (err <= bound[fin]).all(), (name, float(err.max()), frac)


def _rel(v):
    return 1e-9 * (1.0 + np.abs(np.where(np.isfinite(v), v, 0.0)))


def _close(a, b, tol):
    """Scalars: equal where b is infinite (a grid too shallow for the result scores -inf), within tol otherwise."""
    return abs(a - b) <= tol if np.isfinite(b) else a == b


def _no_nan(got):
    for k, v in got.items():
        if k not in ("kind", "calibration", "in_sample"):
            assert not np.isnan(np.asarray(v, dtype=np.float64)).any(), k
    assert not any(np.isnan(v) for v in got["in_sample"].values())


def _check(m, d, G=15, r_eff=1.0):
    """loo_scores against the restatement, every gate; returns (result, restatement)."""
    got = m.loo_scores(d, r_eff=r_eff, max_goals=G)
    ref = OR.scores(m, d, G, r_eff)
    _no_nan(got)
    o = SR.outcome_of(d["home_goals"], d["away_goals"])
    assert got["kind"] == "scores" and got["n"] == o.size
    np.testing.assert_array_equal(got["outcome"], o)
    np.testing.assert_array_equal(got["tail_len"], ref["tail_len"])
    for mine, theirs in (("pareto_k", "pareto_k"), ("ess", "ess"), ("elpd_loo_i", "elpd_loo")):
        _gate(mine, got[mine], ref[theirs], _rel(ref[theirs]))
    _gate("outcome_proba", got["outcome_proba"], ref["proba"], 1e-9)
    _gate("pit_home", got["pit_home"], ref["pit"][:, :2], 1e-9)
    _gate("pit_away", got["pit_away"], ref["pit"][:, 2:], 1e-9)
    _gate("outcome_proba_in_sample", got["outcome_proba_in_sample"], ref["proba_in_sample"], 1e-12)
    log, brier, rps = SR.rules(ref["proba"], o)
    _gate("brier_i", got["brier_i"], brier, 1e-8)
    _gate("rps_i", got["rps_i"], rps, 1e-8)
    assert abs(got["brier"] - brier.mean()) <= 1e-8 and abs(got["rps"] - rps.mean()) <= 1e-8
    P_o = ref["proba"][np.arange(o.size), o]
    with np.errstate(divide="ignore"):
        _gate("log_score_i", got["log_score_i"], log, 1e-9 / P_o + 1e-9)
    for name, want in zip(("log_score", "brier", "rps"), SR.rules(ref["proba_in_sample"], o)):
        assert _close(got["in_sample"][name], want.mean(), 1e-8), name
    if np.isfinite(ref["elpd_loo"]).all():
        assert abs(got["elpd_loo"] - ref["elpd_loo"].sum()) <= _rel(ref["elpd_loo"]).sum()
    else:
        assert got["elpd_loo"] == -np.inf
    np.testing.assert_array_equal(got["reliable"], ref["pareto_k"] <= 0.7)
    assert got["warning"] == bool((ref["pareto_k"] > 0.7).any())
    assert (got["pit_home"][:, 0] <= got["pit_home"][:, 1]).all() and (got["pit_away"][:, 0] <= got["pit_away"][:, 1]).all()
    return got, ref


def _first(d, n):
    return {k: list(v)[:n] for k, v in d.items()}


@pytest.mark.parametrize("S", DRAWS)
@pytest.mark.parametrize("kind", LR.KINDS)
def test_all_classes_against_restatement(kind, S):
    """Per class and draw count: both spreads, each with 50 fixtures and with 1, the grid depths and r_eff in
    rotation so that every class meets every depth and both r_eff at every spread."""
    i, c = DRAWS.index(S), LR.KINDS.index(kind)
    smoothed = []
    for j, spread in enumerate(("wide", "narrow")):
        m = LR.hand_model(kind, S=S, T=8, seed=3 + i)
        if spread == "narrow":
            OR.narrow(m)
        d = LR.hand_data(m, n=50, seed=4 + i, max_goals=6)
        G, G1, r_eff = GRIDS[(i + c + 2 * j) % 5], GRIDS[(i + c + 2 * j + 3) % 5], (1.0, 0.3)[(i + j) % 2]
        if S * G > 700 * 15:      # (the restatement's full grids: the deepest one under 700 draws goes to the single fixture)
            G, G1 = G1, G
        got, ref = _check(m, d, G, r_eff)
        smoothed.append(np.isfinite(ref["pareto_k"]))
        if G <= 1:      # scores beyond the grid: lower = upper = the weighted mass
            over = np.asarray(d["home_goals"]) > G
            assert over.any()
            np.testing.assert_array_equal(got["pit_home"][over, 0], got["pit_home"][over, 1])
        _check(m, _first(d, 1), G1, (1.0, 0.3)[(i + j + 1) % 2])
    # the comparison covers what the draw count is there for: no smoothing below 64 draws, smoothing from there on
    smoothed = np.concatenate(smoothed)
    assert not smoothed.any() if S < 64 else smoothed.mean() > 0.9, smoothed.mean()
    print("worst so far, as fractions of the gates:", {k: f"{v:.2e}" for k, v in WORST.items()})


@pytest.mark.parametrize("r_eff", [1.0, 0.3])
@pytest.mark.parametrize("kind", LR.KINDS)
def test_agrees_with_loo_and_forecast_scores(kind, r_eff):
    worst = 0.0
    for S in (10, 100, 700):
        m = OR.narrow(LR.hand_model(kind, S=S, T=8, seed=11), 0.1)
        d = LR.hand_data(m, n=50, seed=12)
        got, loo, fit = m.loo_scores(d, r_eff=r_eff, max_goals=9), m.loo(d, r_eff=r_eff), m.forecast_scores(d, max_goals=9)
        np.testing.assert_array_equal(got["tail_len"], m._loglik_summary(d, psis=True, r_eff=r_eff)["tail_len"])
        _gate("elpd_loo_i against loo", got["elpd_loo_i"], loo["elpd_loo_i"], _rel(loo["elpd_loo_i"]))
        _gate("pareto_k against loo", got["pareto_k"], loo["pareto_k"], _rel(loo["pareto_k"]))
        assert abs(got["elpd_loo"] - loo["elpd_loo"]) <= _rel(loo["elpd_loo_i"]).sum()
        fin = np.isfinite(loo["pareto_k"])
        worst = max(worst, float(np.abs(got["elpd_loo_i"] - loo["elpd_loo_i"]).max()),
                    float(np.abs(got["pareto_k"][fin] - loo["pareto_k"][fin]).max()) if fin.any() else 0.0)
        _gate("in sample against forecast_scores", got["outcome_proba_in_sample"], fit["outcome_proba"], 1e-12)
        for rule in ("log_score", "brier", "rps"):
            assert _close(got["in_sample"][rule], fit[rule], 1e-11), rule
        out = compare_scores({"in_sample": fit, "loo": got})
        assert set(out) == {"in_sample", "loo"}
    print(f"largest difference to loo ({kind}, r_eff {r_eff}): {worst:.3e}")


@pytest.mark.parametrize("kind", LR.KINDS)
def test_two_draws_by_hand(kind):
    m = LR.hand_model(kind, S=2, T=8, seed=13)
    d = LR.hand_data(m, n=12, seed=14)
    got = m.loo_scores(d, max_goals=10)
    lik = np.exp(m.log_likelihood(d))                        # [2, n] the scoreline likelihoods
    lh, la = SR.rates(m, d)
    p = SR.draw_probs(lh, la, np.asarray(m.corr_coef), 10)   # [2, n, 3]
    inv = 1.0 / lik
    want = (p[0] * inv[0][:, None] + p[1] * inv[1][:, None]) / (inv[0] + inv[1])[:, None]
    _gate("two draws", got["outcome_proba"], want, 1e-9)
    _gate("two draws elpd", got["elpd_loo_i"], np.log(2.0 / (inv[0] + inv[1])), 1e-9 * (1 + np.abs(np.log(lik[0]))))
    assert (got["tail_len"] == 1).all() and (got["pareto_k"] == np.inf).all()


@pytest.mark.parametrize("kind", LR.KINDS)
def test_identical_draws_give_the_in_sample_forecast(kind):
    m = LR.hand_model(kind, S=1, T=8, seed=15)
    for name in ("attack", "defence", "home_advantage", "home_attack", "away_attack", "home_defence", "away_defence",
                 "confederation_strength", "corr_coef"):
        if getattr(m, name, None) is not None:
            setattr(m, name, np.repeat(np.asarray(getattr(m, name)), 64, axis=0))
    d = LR.hand_data(m, n=9, seed=16)
    got = m.loo_scores(d)
    _gate("identical draws", got["outcome_proba"], got["outcome_proba_in_sample"], 1e-12)
    _gate("identical draws ess", got["ess"], np.full(9, 64.0), 1e-9)
    _gate("identical draws elpd", got["elpd_loo_i"], m.log_likelihood(d)[0], 1e-12 * (1 + np.abs(m.log_likelihood(d)[0])))
    _no_nan(got)


def test_clipped_tau_takes_the_limit():
    m = LR.hand_model("basic", S=100, T=8, seed=17)
    m.corr_coef = np.asarray(m.corr_coef).copy()
    m.corr_coef[::7] = 1.5                                   # tau(1, 1) = 1 - rho < 0 (and tau(0, 0) where lh la > 2/3)
    d = LR.hand_data(m, n=60, seed=18, max_goals=2)
    got, ref = _check(m, d, 6)
    x, y = np.asarray(d["home_goals"]), np.asarray(d["away_goals"])
    dead = ~np.isfinite(ref["elpd_loo"])
    assert ((x == 1) & (y == 1) <= dead).all() and dead.any() and not dead.all()
    assert (got["elpd_loo_i"][dead] == -np.inf).all() and (got["pareto_k"][dead] == np.inf).all()
    assert (got["tail_len"][dead] == 0).all() and got["elpd_loo"] == -np.inf and got["warning"] is True
    for k in ("outcome_proba", "outcome_proba_in_sample", "pit_home", "pit_away", "ess", "brier_i", "rps_i"):
        assert np.isfinite(got[k]).all(), k
    assert ((got["ess"][dead] >= 1) & (got["ess"][dead] <= 15) & (got["ess"][dead] == np.round(got["ess"][dead]))).all()
    # a negative coefficient as large clips the 0-1 and 1-0 cells instead
    m.corr_coef[::7] = -1.5
    got, ref = _check(m, d, 6)
    dead = ~np.isfinite(ref["elpd_loo"])
    low = ((x == 0) & (y == 1)) | ((x == 1) & (y == 0))
    assert (dead[low]).any() and not dead[(x == 2) | (y == 2)].any()
    _no_nan(got)


@pytest.mark.parametrize("kind", ["basic", "wc"])
def test_tied_draws_straddle_the_cutoff(kind):
    m = LR.hand_model(kind, S=64, T=8, seed=19)
    for name in ("attack", "defence", "home_advantage", "home_attack", "away_attack", "home_defence", "away_defence",
                 "confederation_strength", "corr_coef"):
        if getattr(m, name, None) is not None:
            setattr(m, name, np.repeat(np.asarray(getattr(m, name)), 2, axis=0))   # S = 128, every draw twice
    d = LR.hand_data(m, n=30, seed=20)
    got, ref = _check(m, d, 8)
    assert (ref["tail_len"] > 4).all() and np.isfinite(ref["pareto_k"]).all()


POINTWISE = ("outcome", "outcome_proba", "outcome_proba_in_sample", "log_score_i", "brier_i", "rps_i", "elpd_loo_i",
             "pareto_k", "ess", "tail_len", "reliable", "pit_home", "pit_away")


@pytest.mark.parametrize("kind", ["extended", "wc"])
def test_bit_identical_runs_and_permutations(kind):
    m = LR.hand_model(kind, S=700, T=8, seed=21)
    d = LR.hand_data(m, n=50, seed=22)
    a, b = m.loo_scores(d, r_eff=0.3), m.loo_scores(d, r_eff=0.3)
    for k in POINTWISE + ("elpd_loo", "log_score", "brier", "rps"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    perm = np.random.RandomState(23).permutation(50)
    other = m.loo_scores({k: [list(v)[i] for i in perm] for k, v in d.items()}, r_eff=0.3)
    for k in POINTWISE:
        np.testing.assert_array_equal(other[k], a[k][perm], err_msg=k)


# ---- the query record (the contexts of tests/test_gpu_query_record.py)
S0, T0 = 10, 2
PLAIN, VENUE, WC = {}, {"neutral": [0, 1]}, {"neutral": [0, 1], "conf": ([0, 1], [1, 0])}
FIX = ([0, 1], [1, 0], [1, 0], [0, 2])
EMPTY = ([], [], [], [])


@pytest.fixture(scope="module")
def ctxs():
    rs = np.random.RandomState(3)
    tabs = [rs.normal(0.0, 0.2, (S0, T0)) for _ in range(6)]
    corr = rs.uniform(-0.05, 0.05, S0)          # (no clipped tau: every log-likelihood is finite)
    c = {k: HipContext(0) for k in ("fresh", "plain", "venue", "wc")}
    c["plain"].predict_set_posterior(tabs[0], tabs[1], rs.normal(0.3, 0.05, S0), corr)
    c["venue"].predict_set_posterior_venue(*tabs, corr)
    c["wc"].predict_set_posterior_venue(*tabs, corr, confederation_strength=rs.normal(0.0, 0.2, (S0, 2)))
    yield c
    for x in c.values():
        x.close()


def _code(ctx, cols, G=3, **kw):
    with pytest.raises(BplHipError) as e:
        ctx.loo_scores(*cols, G, **kw)
    return e.value.code


def test_query_through_the_record(ctxs):
    for kw in (PLAIN, VENUE, WC):
        assert _code(ctxs["fresh"], FIX, **kw) == BPLHIP_ESTATE, kw
    for which, kw in (("plain", VENUE), ("plain", WC), ("venue", PLAIN), ("wc", PLAIN)):
        assert _code(ctxs[which], FIX, **kw) == BPLHIP_ESTATE, (which, kw)
        kw0 = {k: ([], []) if k == "conf" else [] for k in kw}
        assert _code(ctxs[which], EMPTY, **kw0) == BPLHIP_ESTATE, (which, kw0)
    assert _code(ctxs["venue"], FIX, **WC) == BPLHIP_EINVAL
    assert _code(ctxs["wc"], FIX, **VENUE) == BPLHIP_EINVAL
    shapes = {"elpd_loo": (2,), "pareto_k": (2,), "ess": (2,), "tail_len": (2,), "proba": (2, 3),
              "proba_in_sample": (2, 3), "pit": (2, 4)}
    for which, kw in (("plain", PLAIN), ("venue", VENUE), ("wc", WC)):
        assert _code(ctxs[which], FIX, G=64, **kw) == BPLHIP_EINVAL
        assert _code(ctxs[which], FIX, G=-1, **kw) == BPLHIP_EINVAL
        for r in (0.0, -1.0, np.inf, np.nan):
            assert _code(ctxs[which], FIX, r_eff=r, **kw) == BPLHIP_EINVAL, r
        kw0 = {k: ([], []) if k == "conf" else [] for k in kw}
        empty = ctxs[which].loo_scores(*EMPTY, 3, **kw0)            # m = 0: OK, nothing written
        assert {k: v.shape for k, v in empty.items()} == {k: (0,) + s[1:] for k, s in shapes.items()}
        got = ctxs[which].loo_scores(*FIX, 3, **kw)
        assert {k: v.shape for k, v in got.items()} == shapes
        assert got["tail_len"].dtype == np.int32 and all(v.dtype == np.float64 for k, v in got.items() if k != "tail_len")
        # S = 10 gives a PSIS tail of 2 draws: not smoothed, k = +inf by definition
        assert (got["pareto_k"] == np.inf).all() and (got["tail_len"] == 2).all()
        assert all(np.isfinite(v).all() for k, v in got.items() if k != "pareto_k")
        summ = ctxs[which].loglik_summary(*FIX, **kw)
        np.testing.assert_allclose(got["elpd_loo"], summ["elpd_loo"], rtol=1e-12)
        np.testing.assert_allclose(got["proba_in_sample"], ctxs[which].outcome_scores(*FIX, 3, **kw)["proba"], rtol=0, atol=1e-12)
