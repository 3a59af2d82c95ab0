"""Posterior predictive checks on the device (csrc/dc_ppc.hip.h) against the numpy restatement
(tests/ppc_ref.py) for the five predictor classes, and on one draw per replication, grouping invariance,
agreement with the score-grid kernel, consistency of the returned scorelines, determinism and error states."""
import numpy as np
import pytest

import loglik_ref as LR
import ppc_ref as PR
from bpl._ffi import BPLHIP_ESTATE, BplHipError, HipContext
from bpl.ppc import STATISTICS
from ppc_compare import against_restatement as _against_restatement

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.mark.parametrize("kind", LR.KINDS)
def test_all_classes_bit_exact(kind):
    m = LR.hand_model(kind, S=64, T=8, seed=3)
    d = LR.hand_data(m, n=70, seed=4)
    d["home_goals"][:3] = [0, 1, 12]
    _against_restatement(m, d, R=300, seed=11, G=4)


def test_clipped_tau_bit_exact():
    # rates e^1 (x e^0.25 at home) and rho = 0.5: 1 - lh la rho < 0, so 0-0 never happens
    m = LR.hand_model("extended", S=16, T=6, seed=5)
    m.attack[:] = 1.0
    m.defence[:] = 0.0
    m.corr_coef[:] = 0.5
    d = LR.hand_data(m, n=40, seed=6)
    res, _, _, _ = _against_restatement(m, d, R=400, seed=2, G=3)
    assert np.all(res["scoreline"]["replicated"][:, 0, 0] == 0)
    # rho = -0.9: 1 + lh rho and 1 + la rho are clipped, so 0-1 and 1-0 never happen
    m = LR.hand_model("wc", S=16, T=6, seed=5)
    m.attack[:] = 1.0
    m.defence[:] = 0.0
    m.corr_coef[:] = -0.9
    d = LR.hand_data(m, n=40, seed=6)
    res, _, _, _ = _against_restatement(m, d, R=400, seed=3, G=3)
    sc = res["scoreline"]["replicated"]
    assert np.all(sc[:, 0, 1] == 0) and np.all(sc[:, 1, 0] == 0)


@pytest.mark.parametrize("kind", ["basic", "dynamic"])
def test_one_draw_per_replication(kind):
    m = LR.hand_model(kind, S=2, T=6, seed=1)
    for nm in ("attack", "defence", "home_attack", "away_attack", "home_defence", "away_defence"):
        if hasattr(m, nm) and getattr(m, nm) is not None:
            getattr(m, nm)[:] = 0.0
    m.attack[0] = 1.5     # draw 0: ~4.5 goals a side; draw 1: ~0.14
    m.attack[1] = -2.0
    if kind == "basic":
        m.home_advantage[:] = 0.0
    d = LR.hand_data(m, n=60, seed=2)
    res = m.posterior_predictive_check(d, num_replications=50, random_state=4)
    tot = res["home_goals"]["replicated"] + res["away_goals"]["replicated"]
    assert tot[0::2].min() > 10 * tot[1::2].max(), (tot[0::2].min(), tot[1::2].max())


@pytest.mark.parametrize("kind", ["basic", "wc"])
def test_grouping_invariance(kind):
    m = LR.hand_model(kind, S=32, T=8, seed=7)
    d = LR.hand_data(m, n=90, seed=8)
    groups, n = m._loglik_groups(d)
    (_, device, kw), = groups
    idx, hs, as_ = PR.slots(m, d)
    k, key = idx.size, (0x1234, 0x5678)
    extra = {nm: kw[nm] for nm in ("neutral", "conf") if nm in kw}
    whole = device().ppc(kw["home_idx"], kw["away_idx"], hs, as_, k, 5, 200, key, return_scores=True, **extra)
    part = np.random.RandomState(0).rand(n) < 0.4
    total = None
    for sel in (np.nonzero(part)[0], np.nonzero(~part)[0]):
        sub = {nm: (v[sel] if nm != "conf" else (None if v is None else (v[0][sel], v[1][sel])))
               for nm, v in extra.items()}
        r = device().ppc(kw["home_idx"][sel], kw["away_idx"][sel], hs[sel], as_[sel], k, 5, 200, key,
                         fixture_id=sel, return_scores=True, **sub)
        np.testing.assert_array_equal(r["home_goals"], whole["home_goals"][:, sel])
        np.testing.assert_array_equal(r["away_goals"], whole["away_goals"][:, sel])
        r = {nm: r[nm].astype(np.int64) for nm in ("score", "outcome", "sums", "team")}
        total = r if total is None else {nm: total[nm] + r[nm] for nm in total}
    for nm in total:
        np.testing.assert_array_equal(total[nm], whole[nm].astype(np.int64))


@pytest.mark.parametrize("kind", ["basic", "extended", "neutral", "wc"])
def test_mean_scoreline_matches_the_grid_kernel(kind):
    # R = 500 S: every draw is used exactly 500 times, so the mean replicated count of a cell has expectation
    # sum over fixtures of the posterior-mean grid.  Tolerance: 5 standard errors of the mean, with the
    # replications' own standard deviation (it also holds the between-draw spread, so it overstates the error)
    m = LR.hand_model(kind, S=16, T=6, seed=9)
    d = LR.hand_data(m, n=25, seed=10)
    G, R = 4, 8000
    res = m.posterior_predictive_check(d, num_replications=R, random_state=5, max_goals=G)
    rep = res["scoreline"]["replicated"].astype(np.float64)
    groups, _ = m._loglik_groups(d)
    (_, device, kw), = groups
    extra = {nm: kw[nm] for nm in ("neutral", "conf") if nm in kw}
    grid = device().predict_score_grid(kw["home_idx"], kw["away_idx"], 40, **extra).sum(axis=0)
    assert abs(grid.sum() - 25) < 1e-5   # (the grid kernel's own rounding: ~1e-6 over 41 x 41 cells)
    fold = np.zeros((G + 1, G + 1))
    for i in range(41):
        for j in range(41):
            fold[min(i, G), min(j, G)] += grid[i, j]
    err = np.abs(rep.mean(axis=0) - fold)
    tol = 5 * rep.std(axis=0) / np.sqrt(R) + 1e-5
    assert np.all(err <= tol), (err / tol).max()
    assert abs(rep.sum(axis=(1, 2)) - 25).max() == 0


@pytest.mark.parametrize("kind", ["basic", "wc", "dynamic"])
def test_returned_scorelines_recount_to_the_tallies(kind):
    m = LR.hand_model(kind, S=40, T=10, seed=12)
    d = LR.hand_data(m, n=200, seed=13)
    G = 6
    res = m.posterior_predictive_check(d, num_replications=1000, random_state=8, max_goals=G,
                                       return_replications=True)
    idx, hs, as_ = PR.slots(m, d)
    raw = PR.raw_tallies(res["replications"]["home_goals"], res["replications"]["away_goals"], hs, as_, idx.size, G)
    np.testing.assert_array_equal(res["scoreline"]["replicated"], raw["score"])
    np.testing.assert_array_equal(res["outcome"]["replicated"], raw["outcome"])
    np.testing.assert_array_equal(res["home_goals"]["replicated"], raw["sums"][:, 0])
    np.testing.assert_array_equal(res["away_goals"]["replicated"], raw["sums"][:, 1])
    np.testing.assert_array_equal(res["team_goals_for"]["replicated"], raw["team"][..., 0])
    np.testing.assert_array_equal(res["team_goals_against"]["replicated"], raw["team"][..., 1])


def test_determinism():
    m = LR.hand_model("wc", S=50, T=12, seed=14)
    d = LR.hand_data(m, n=3000, seed=15)
    a = m.posterior_predictive_check(d, num_replications=700, random_state=99, return_replications=True)
    b = m.posterior_predictive_check(d, num_replications=700, random_state=99, return_replications=True)
    for nm in STATISTICS:
        np.testing.assert_array_equal(a[nm]["replicated"], b[nm]["replicated"])
    np.testing.assert_array_equal(a["replications"]["home_goals"], b["replications"]["home_goals"])
    np.testing.assert_array_equal(a["replications"]["away_goals"], b["replications"]["away_goals"])
    c = m.posterior_predictive_check(d, num_replications=700, random_state=100)
    assert not np.array_equal(a["scoreline"]["replicated"], c["scoreline"]["replicated"])


def test_error_states():
    h = np.array([0, 1], dtype=np.uint16)
    a = np.array([1, 0], dtype=np.uint16)
    ctx = HipContext(0)
    try:
        with pytest.raises(BplHipError) as e:
            ctx.ppc(h, a, h, a, 2, 4, 10, (1, 2))
        assert e.value.code == BPLHIP_ESTATE
        m = LR.hand_model("basic", S=8, T=3)
        ctx.predict_set_posterior(m.attack, m.defence, m.home_advantage, m.corr_coef)
        with pytest.raises(BplHipError) as e:
            ctx.ppc(h, a, h, a, 2, 4, 10, (1, 2), neutral=np.zeros(2))
        assert e.value.code == BPLHIP_ESTATE
        ctx.ppc(h, a, h, a, 2, 4, 10, (1, 2))
        w = LR.hand_model("neutral", S=8, T=3)
        ctx.predict_set_posterior_venue(w.attack, w.defence, w.home_attack, w.away_attack, w.home_defence,
                                        w.away_defence, w.corr_coef)
        with pytest.raises(BplHipError) as e:
            ctx.ppc(h, a, h, a, 2, 4, 10, (1, 2))
        assert e.value.code == BPLHIP_ESTATE
        r = ctx.ppc(h, a, h, a, 2, 4, 10, (1, 2), neutral=np.ones(2))
        assert r["outcome"].sum() == 20
        with pytest.raises(BplHipError):
            ctx.ppc(h, a, h, a, 1, 4, 10, (1, 2), neutral=np.ones(2))     # slot 1 >= n_slots
        with pytest.raises(BplHipError):
            ctx.ppc(h, a, h, a, 2, 16, 10, (1, 2), neutral=np.ones(2))    # max_goals > 15
    finally:
        ctx.close()
