"""simulate_season with matches in progress and weighted draws on the device (csrc/dc_live.hip.h) against the
kick-off simulator (the anchor: states 0-0 at t = 0 are ordinary fixtures, bit for bit), against the numpy
restatement (tests/live_ref.py) and against the separately written in-play restatement's log likelihood, and on the
properties the feature is for: the evidence of a state reaches the table, the final scores follow the conditional
law, the draws are used floor or ceil of their share."""
import numpy as np
import pytest

import inplay_ref as IR
import live_cases as LC
import live_ref as LR
from bpl import DixonColesMatchPredictor
from bpl._ffi import BPLHIP_EINVAL, BplHipError
from bpl.base import SEASON_MAX_FIXTURES, _prng_key
from test_gpu_season import _model, _round_robin
from test_live_host import check_frequencies

pytestmark = pytest.mark.gpu
TIEBREAKS = ("overall", "head_to_head")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---- the anchor
@pytest.mark.parametrize("kind", LC.KINDS)
@pytest.mark.parametrize("tiebreak", TIEBREAKS)
def test_kick_off_states_are_ordinary_fixtures_bit_for_bit(kind, tiebreak):
    m = LC.posterior(kind)
    home, away = LC.fixtures(m)
    ip = LC.in_play(m, ((0, 0, 0.0),) * 4)
    kw = dict(num_simulations=1000, random_state=77, current_table=LC.TABLE, return_tables=True, return_scores=True,
              tiebreak=tiebreak)
    live = m.simulate_season(home, away, in_play=ip, reweight=False, **kw)
    plain = m.simulate_season(home + ip["home_team"], away + ip["away_team"], **kw)     # the 13 fixtures
    for key in ("teams", "position_proba", "expected_points", "expected_goal_difference", "points", "position"):
        np.testing.assert_array_equal(live[key], plain[key], err_msg=key)
    for side in ("home_goals", "away_goals"):
        np.testing.assert_array_equal(live[side], plain[side][:, :9], err_msg=side)
        np.testing.assert_array_equal(live["in_play_" + side], plain[side][:, 9:], err_msg=side)
    np.testing.assert_array_equal(live["draw"], np.arange(1000) % LC.S)
    assert live["ess"] == float(LC.S) and np.isnan(live["log_evidence"])     # no weights in force, no likelihood
    assert set(live) == set(plain) | {"draw", "in_play_home_goals", "in_play_away_goals", "ess", "log_evidence"}
    # an empty in_play and no log_weights: the plain call
    empty = m.simulate_season(home, away, in_play={k: [] for k in ip}, **kw)
    plain9 = m.simulate_season(home, away, **kw)
    for key in plain9:
        np.testing.assert_array_equal(empty[key], plain9[key], err_msg=key)
    assert empty["ess"] == float(LC.S) and empty["log_evidence"] == 0.0 and empty["in_play_home_goals"].shape == (1000, 0)


# ---- the restatement
def _loglik_gate(m, ipr):
    """(sum over the matches of inplay_ref's l [S], its bound [S]) for the states `ipr`: inplay_ref.gates' bound per
    match, plus one rounding of the running sum per match."""
    ih, ia, ix, iy, it = ipr
    s = np.arange(m.attack.shape[0])[:, None]
    lh, la = LR.rates(m.attack, m.defence, m.home_advantage, s, ih.astype(np.int64)[None, :], ia.astype(np.int64)[None, :])
    G = int(max(ix.max(), iy.max()))
    ref = IR.from_rates(lh, la, m.corr_coef, ix, iy, it, np.ones((1, G + 1, G + 1)), G, ())
    ref.update(a=ix.astype(np.int64), b=iy.astype(np.int64), t=it, wmax=np.ones(1))
    lev, gate = ref["draw_log_evidence"], IR.gates(ref)["draw_log_evidence"]
    total, biggest = np.zeros(lev.shape[0]), np.zeros(lev.shape[0])
    for i in range(lev.shape[1]):
        total = total + lev[:, i]
        biggest = np.maximum(biggest, np.abs(total))
    return total, gate.sum(axis=1) + lev.shape[1] * IR.EPS * biggest


@pytest.mark.parametrize("kind", LC.KINDS)
@pytest.mark.parametrize("with_log_weights", [False, True])
@pytest.mark.parametrize("tiebreak", TIEBREAKS)
def test_against_the_restatement(kind, with_log_weights, tiebreak):
    m, ref = LC.restatement(kind, with_log_weights, tiebreak)
    home, away = LC.fixtures(m)
    lw = LC.random_log_weights() if with_log_weights else None
    res = m.simulate_season(home, away, num_simulations=LC.N, random_state=LC.SEED, current_table=LC.TABLE,
                            in_play=LC.in_play(m), log_weights=lw, return_tables=True, return_scores=True,
                            return_weights=True, tiebreak=tiebreak)
    keep = ~ref["flagged"]
    tag = f"{kind} log_weights={with_log_weights} {tiebreak}"
    print(f"{tag}: flagged {int(ref['flagged'].sum())} of {LC.N}")
    assert ref["flagged"].sum() <= 0.01 * LC.N
    for key in ("draw", "points", "position", "home_goals", "away_goals", "in_play_home_goals", "in_play_away_goals"):
        assert res[key].dtype == ref[key].dtype and res[key].shape == ref[key].shape, key
        np.testing.assert_array_equal(res[key][keep], ref[key][keep], err_msg=key)
    # the counts with the flagged simulations removed from both sides; the device's aggregates are its own rows'
    n = LC.T
    counts = np.zeros((n, n), dtype=np.int64)
    np.add.at(counts, (np.broadcast_to(np.arange(n), (LC.N, n))[keep], res["position"][keep].astype(np.int64)), 1)
    np.testing.assert_array_equal(counts, ref["unflagged_counts"])
    every = np.zeros((n, n), dtype=np.int64)
    np.add.at(every, (np.broadcast_to(np.arange(n), (LC.N, n)), res["position"].astype(np.int64)), 1)
    np.testing.assert_array_equal(res["position_proba"], every / LC.N)
    np.testing.assert_array_equal(res["expected_points"], res["points"].astype(np.int64).sum(axis=0) / LC.N)
    # L and L0 against the in-play restatement's closed-form route, within its own bound
    ipr = m._in_play_inputs(LC.in_play(m))
    raw = m._device().simulate_season_live(*m._team_indices(home, away), np.arange(n), np.zeros((n, 3)), (3, 1, 0), 64,
                                           _prng_key(1), in_play=ipr, log_weights=lw, return_weights=True)
    total, gate = _loglik_gate(m, ipr)
    e0 = np.abs(raw["L0"] - total) / gate
    L = total + (0.0 if lw is None else lw)
    e1 = np.abs(raw["L"] - L) / (gate + IR.EPS * np.abs(L))
    print(f"{tag}: L0 error / gate {e0.max():.3e}, L error / gate {e1.max():.3e}")
    assert e0.max() <= 1.0 and e1.max() <= 1.0
    np.testing.assert_array_equal(res["log_weights"], raw["L"] - raw["L"].max())
    e_ess = abs(res["ess"] - ref["ess"]) / ref["ess"]
    e_ev = abs(res["log_evidence"] - ref["log_evidence"]) / abs(ref["log_evidence"])
    print(f"{tag}: ess relative error {e_ess:.3e}, log_evidence relative error {e_ev:.3e}")
    assert e_ess <= 1e-9 and e_ev <= 1e-9


# ---- the evidence reaches the table
def test_a_state_moves_the_draws_and_the_title_odds():
    S, T, N = 2, 8, 20_000
    rs = np.random.RandomState(11)
    att, dfn = rs.normal(0, 0.1, (S, T)), rs.normal(0, 0.1, (S, T))
    att[0, 0], dfn[0, 0], att[1, 0], dfn[1, 0] = 1.5, 1.5, -1.5, -1.5      # team 0: best in draw 0, worst in draw 1
    m = _model(DixonColesMatchPredictor, att, dfn, np.full(S, 0.2), np.zeros(S))
    h, a = _round_robin(T)
    rest = ~((h == 0) & (a == 1))
    ip = {"home_team": ["t00"], "away_team": ["t01"], "home_goals": [4], "away_goals": [0], "elapsed": [0.3]}
    kw = dict(num_simulations=N, random_state=7, in_play=ip, return_tables=True)
    on = m.simulate_season(h[rest], a[rest], return_weights=True, **kw)
    off = m.simulate_season(h[rest], a[rest], reweight=False, **kw)
    om = np.exp(on["log_weights"])
    share = om[0] / om.sum()
    assert share > 0.99                                                    # 4-0 up after 27 minutes: draw 0
    assert abs(np.mean(on["draw"] == 0) - share) <= 1.0 / N
    assert abs(np.mean(off["draw"] == 0) - 0.5) <= 1.0 / N and off["ess"] == 2.0
    assert on["position_proba"][0, 0] > off["position_proba"][0, 0] + 0.3
    assert 1.0 <= on["ess"] < 1.02 and np.isfinite(on["log_evidence"])


# ---- the conditional law (one draw, one match in play and NO ordinary fixture)
@pytest.mark.parametrize("state", [(1, 0, 0.5), (0, 0, 0.25)])
@pytest.mark.parametrize("rho", [0.05, -1.1])                              # unclipped; tau(0, 1) and tau(1, 0) clipped
def test_final_scores_follow_the_conditional_law(state, rho):
    a, b, t = state
    N, G = 200_000, 12
    m = _model(DixonColesMatchPredictor, np.array([[0.3, 0.1]]), np.array([[0.05, -0.1]]), np.array([0.2]), np.array([rho]))
    ip = {"home_team": ["t00"], "away_team": ["t01"], "home_goals": [a], "away_goals": [b], "elapsed": [t]}
    res = m.simulate_season([], [], num_simulations=N, random_state=5, in_play=ip, return_scores=True)
    x, y = res["in_play_home_goals"][:, 0].astype(np.int64), res["in_play_away_goals"][:, 0].astype(np.int64)
    assert x.min() >= a and y.min() >= b and res["home_goals"].shape == (N, 0)
    lh, la = LR.rates(m.attack, m.defence, m.home_advantage, np.array([0]), np.array([0]), np.array([1]))
    check_frequencies(x, y, LR.conditional_pmf(float(lh[0]), float(la[0]), rho, a, b, t, G), N)
    assert res["ess"] == 1.0


# ---- log_weights alone
def test_log_weights_alone_select_the_draws():
    m = LC.posterior("basic")
    home, away = LC.fixtures(m)
    kw = dict(num_simulations=LC.N, random_state=3, return_tables=True)
    lw = np.full(LC.S, -1e4)
    lw[100] = 0.0
    res = m.simulate_season(home, away, log_weights=lw, **kw)
    assert (res["draw"] == 100).all() and res["ess"] == 1.0 and res["log_evidence"] == 0.0
    res = m.simulate_season(home, away, log_weights=np.full(LC.S, 3.5), **kw)
    used = np.bincount(res["draw"], minlength=LC.S)
    assert used.min() >= LC.N // LC.S and used.max() <= -(-LC.N // LC.S)
    assert abs(res["ess"] - LC.S) <= 1e-9 * LC.S
    # a row of generic weights: floor or ceil of the share (the restatement's weights; 1e-6 is far below their spacing)
    lw = LC.random_log_weights()
    res = m.simulate_season(home, away, log_weights=lw, **kw)
    w = LR.weights(lw, np.zeros(LC.S))
    expect = LC.N * w["omega"] / w["W"]
    used = np.bincount(res["draw"], minlength=LC.S)
    assert np.all(used >= np.floor(expect - 1e-6)) and np.all(used <= np.ceil(expect + 1e-6))


def test_determinism_and_context_reuse():
    m = LC.posterior("extended")
    home, away = LC.fixtures(m)
    kw = dict(num_simulations=3000, random_state=42, in_play=LC.in_play(m), log_weights=LC.random_log_weights(),
              return_tables=True, return_scores=True, return_weights=True, tiebreak="head_to_head")
    r1 = m.simulate_season(home, away, **kw)
    m.simulate_season(home, away, num_simulations=100, random_state=1)            # another call on the same context
    r2 = m.simulate_season(home, away, **kw)
    r3 = m.simulate_season(home, away, **dict(kw, random_state=43))
    for key in r1:
        np.testing.assert_array_equal(r1[key], r2[key], err_msg=key)
    assert not np.array_equal(r1["in_play_home_goals"], r3["in_play_home_goals"])
    np.testing.assert_array_equal(r1["log_weights"], r3["log_weights"])            # the weights do not depend on the key
    np.testing.assert_allclose(r1["position_proba"].sum(axis=0), 1.0, atol=1e-12)


def test_zero_ordinary_fixtures_and_the_last_minute():
    m = LC.posterior("basic")
    ref = LC.reference(m, [], [], LC.in_play(m), 512, 9, LC.TABLE)
    res = m.simulate_season([], [], num_simulations=512, random_state=9, current_table=LC.TABLE, in_play=LC.in_play(m),
                            return_tables=True, return_scores=True)
    keep = ~ref["flagged"]
    assert ref["flagged"].sum() <= 0.01 * 512
    for key in ("draw", "points", "position", "in_play_home_goals", "in_play_away_goals"):
        np.testing.assert_array_equal(res[key][keep], ref[key][keep], err_msg=key)
    assert res["home_goals"].shape == (512, 0)
    # t = 0.999 with rates <= 3: at least 99 % of the finals are the current score (exp(-0.006) = 0.994 at the least)
    rs = np.random.RandomState(6)
    m = _model(DixonColesMatchPredictor, rs.normal(0, 0.1, (64, 4)), rs.normal(0, 0.1, (64, 4)), np.full(64, 0.25),
               rs.uniform(-0.1, 0.1, 64))
    h, a = _round_robin(4)
    lh, la = LR.rates(m.attack, m.defence, m.home_advantage, np.arange(64)[:, None], h.astype(np.int64)[None, :],
                      a.astype(np.int64)[None, :])
    assert max(lh.max(), la.max()) <= 3.0
    ip = {"home_team": ["t00", "t02"], "away_team": ["t01", "t03"], "home_goals": [0, 2], "away_goals": [3, 2],
          "elapsed": [0.999, 0.999]}
    res = m.simulate_season([], [], num_simulations=20_000, random_state=2, in_play=ip, return_scores=True)
    for i, (x, y) in enumerate(((0, 3), (2, 2))):
        still = (res["in_play_home_goals"][:, i] == x) & (res["in_play_away_goals"][:, i] == y)
        assert still.mean() >= 0.99, (i, still.mean())


def test_the_library_refuses_malformed_input():
    m = LC.posterior("basic")
    ctx = m._device()
    S = LC.S

    def call(ip=((4,), (5,), (1,), (0,), (0.4,)), home=(0,), away=(1,), table_idx=(0, 1, 4, 5), lw=None):
        return ctx.simulate_season_live(list(home), list(away), list(table_idx), np.zeros((len(table_idx), 3)),
                                        (3, 1, 0), 10, (0, 1), in_play=ip, log_weights=lw)

    assert call()["counts"].sum() == 40
    bad = [dict(ip=((4,), (5,), (1,), (0,), (t,))) for t in (float("nan"), 1.0, -0.1, 0.0)]     # 0.0: 1-0 at kick-off
    bad += [dict(ip=((4,), (5,), (64,), (0,), (0.4,))), dict(ip=((4,), (5,), (0,), (64,), (0.4,))),
            dict(ip=((4,), (3,), (1,), (0,), (0.4,))),                   # team 3 is no row of the table
            dict(ip=((4,), (4,), (1,), (0,), (0.4,))),                   # a team playing itself
            dict(ip=((4,), (99,), (1,), (0,), (0.4,))),                  # no such team
            dict(lw=np.full(S, np.inf)), dict(lw=np.where(np.arange(S) == 7, np.nan, 0.0))]
    for kw in bad:
        with pytest.raises(BplHipError) as e:
            call(**kw)
        assert e.value.code == BPLHIP_EINVAL, kw
    F = SEASON_MAX_FIXTURES
    with pytest.raises(BplHipError) as e:
        call(home=np.zeros(F, np.uint16), away=np.ones(F, np.uint16))
    assert e.value.code == BPLHIP_EINVAL
    assert call()["counts"].sum() == 40                                  # the context is still good
    with pytest.raises(ValueError, match="not supported together"):
        m.simulate_season(["t00"], ["t01"], in_play=LC.in_play(m), playoffs={"bracket": [0, 1]})
