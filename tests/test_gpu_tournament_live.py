"""simulate_tournament with group matches in progress and weighted draws on the device
(csrc/dc_tournament_live.hip.h) against the numpy restatement (tests/tournament_live_ref.py): the kick-off identity
in all eight modes, the restatement on the shapes of tests/tournament_live_cases.py, a host listed second,
`log_weights` alone, determinism and reuse of a context, and the library's refusals through the raw binding.
tests/test_tournament_live_host.py shows without a GPU that the restatement flags at most 1 % of every case."""
import numpy as np
import pytest

import inplay_ref as IR
import tournament_live_cases as C
import tournament_live_ref as TLR
import tournament_ref as TR
from bpl._ffi import BPLHIP_EINVAL, BplHipError
from test_tournament_host import hand_posterior

pytestmark = pytest.mark.gpu

KICK_OFF = [("A", mode_id, False) for mode_id in C.MODE_IDS] + [("B", mode_id, table) for mode_id in C.MODE_IDS
                                                                for table in (False, True)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---- the anchor: fails on a library without the feature (TypeError: no such keyword)
@pytest.mark.parametrize("name,mode_id,table", KICK_OFF, ids=lambda v: str(v))
def test_kick_off_states_are_ordinary_group_fixtures_bit_for_bit(name, mode_id, table):
    states, pairs = C.kick_off(name)
    m, common, inp, _ = C.call(name, mode_id, table, in_play=states, reweight=False)
    live = m.simulate_tournament(return_stages=True, **common)
    plain_kw = {k: v for k, v in common.items() if k not in ("in_play", "reweight", "log_weights")}
    plain_kw["group_fixtures"] = list(common["group_fixtures"]) + pairs
    plain = m.simulate_tournament(return_stages=True, **plain_kw)
    keys = ["round_proba", "group_position_proba", "stage"]
    keys += ["decided", "decided_proba"] if inp["knockout_rule"] == "extra_time" else []
    keys += ["best_slot_count"] if table else []
    for k in keys:
        np.testing.assert_array_equal(live[k], plain[k], err_msg=k)
    S = np.asarray(m.corr_coef).size
    np.testing.assert_array_equal(live["draw"], np.arange(C.N) % S)
    assert live["draw"].dtype == np.int32 and live["in_play_home_goals"].shape == (C.N, len(pairs))
    assert live["ess"] == float(S) and np.isnan(live["log_evidence"])     # no weights in force, no likelihood
    assert set(live) == set(plain) | {"draw", "in_play_home_goals", "in_play_away_goals", "ess", "log_evidence"}


# ---- the restatement
def _loglik_gate(m, inp):
    """(sum over the states of inplay_ref's l [S], its bound [S]): inplay_ref.gates' bound per match plus one
    rounding of the running sum per match, summed as tests/test_gpu_live.py sums it, on the tournament's rates."""
    hs, as_, on, a, b, _ = TLR.oriented(inp, inp["in_play"])
    eh, ea = TLR.log_rates(TR.model_tables(m), inp, hs, as_, on)
    lh, la = np.exp(eh), np.exp(ea)
    t = inp["in_play"][4]
    G = int(max(a.max(), b.max()))
    ref = IR.from_rates(lh, la, np.asarray(m.corr_coef, np.float64), a, b, t, np.ones((1, G + 1, G + 1)), G, ())
    ref.update(a=a, b=b, t=t, wmax=np.ones(1))
    lev, gate = ref["draw_log_evidence"], IR.gates(ref)["draw_log_evidence"]
    total, biggest = np.zeros(lev.shape[0]), np.zeros(lev.shape[0])
    for i in range(lev.shape[1]):
        total = total + lev[:, i]
        biggest = np.maximum(biggest, np.abs(total))
    return total, gate.sum(axis=1) + lev.shape[1] * IR.EPS * biggest


@pytest.mark.parametrize("case", C.GPU_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_against_the_restatement(case):
    name, mode_id, table, with_lw = case
    m, common, inp, dev = C.call(name, mode_id, table, with_lw)
    ref = C.restatement(*case)
    res = m.simulate_tournament(return_stages=True, return_weights=True, **common)
    keep = ~ref["flagged"]
    print(f"{case}: flagged {int(ref['flagged'].sum())} of {C.N}")
    assert ref["flagged"].sum() <= 0.01 * C.N
    keys = ["draw", "stage", "in_play_home_goals", "in_play_away_goals"]
    keys += ["decided"] if inp["knockout_rule"] == "extra_time" else []
    for k in keys:
        assert res[k].dtype == ref[k].dtype and res[k].shape == ref[k].shape, k
        np.testing.assert_array_equal(res[k][keep], ref[k][keep], err_msg=k)
    # the aggregates are the device's own rows'
    n, R = len(inp["teams"]), inp["rounds"]
    reached = (res["stage"][:, :, None] >= np.arange(1, R + 2)[None, None, :]).sum(axis=0)
    np.testing.assert_array_equal(res["round_proba"], reached / C.N)
    if not ref["flagged"].any():
        if inp["group"] is not None:
            np.testing.assert_array_equal(res["group_position_proba"],
                                          ref["position_counts"][:, :inp["group_size"]] / C.N)
        if table:
            np.testing.assert_array_equal(res["best_slot_count"], ref["slot_counts"])
    # L and L0 within the in-play restatement's own bound
    lw = common["log_weights"]
    raw = m._device().simulate_tournament_live(*dev["args"], return_weights=True, reweight=True, **dev["kwargs"])
    np.testing.assert_array_equal(res["log_weights"], raw["L"] - raw["L"].max())
    if inp["in_play"][0].size:
        total, gate = _loglik_gate(m, inp)
        e0 = np.abs(raw["L0"] - total) / gate
        L = total + (0.0 if lw is None else lw)
        e1 = np.abs(raw["L"] - L) / (gate + IR.EPS * np.abs(L))
        print(f"{case}: L0 error / gate {e0.max():.3e}, L error / gate {e1.max():.3e}")
        assert e0.max() <= 1.0 and e1.max() <= 1.0
    else:
        np.testing.assert_array_equal(raw["L"], lw)
        np.testing.assert_array_equal(raw["L0"], 0.0)
    e_ess = abs(res["ess"] - ref["ess"]) / ref["ess"]
    e_ev = abs(res["log_evidence"] - ref["log_evidence"]) / max(abs(ref["log_evidence"]), 1e-300)
    print(f"{case}: ess relative error {e_ess:.3e}, log_evidence relative error {e_ev:.3e}")
    assert e_ess <= 1e-9 and (e_ev <= 1e-9 or res["log_evidence"] == ref["log_evidence"])


# ---- a host listed second
@pytest.mark.parametrize("mode_id", ["overall-redraw", "h2h-extra_time"])
def test_a_host_listed_second_keeps_the_listed_orientation(mode_id):
    ip = {"home_team": ["t00"], "away_team": ["t01"], "home_goals": [2], "away_goals": [1], "elapsed": [1.0 - 1e-9]}
    m, common, _, _ = C.call("A", mode_id, in_play=ip)      # t01 is the host
    common = dict(common, group_fixtures=[], current_table=None)
    res = m.simulate_tournament(return_stages=True, **common)
    np.testing.assert_array_equal(res["in_play_home_goals"], 2)
    np.testing.assert_array_equal(res["in_play_away_goals"], 1)
    # booked for the right sides: t00 won 2-1 and tops group A, t01 is last on goal difference, every time
    assert res["group_position_proba"][0, 0] == 1.0 and res["group_position_proba"][1, 3] == 1.0


# ---- log_weights alone
@pytest.mark.parametrize("mode_id", ["overall-redraw", "overall-extra_time"])
def test_log_weights_alone_select_the_weighted_draws(mode_id):
    m, common, _, _ = C.call("C", mode_id)
    S = np.asarray(m.corr_coef).size
    heavy = np.array([3, 11, 12, 29, 39])
    lw = np.full(S, -1000.0)
    lw[heavy] = 0.0
    res = m.simulate_tournament(return_stages=True, return_weights=True, **dict(common, log_weights=lw))
    assert set(np.unique(res["draw"])) == set(heavy)
    used = np.bincount(res["draw"], minlength=S)[heavy]
    assert used.sum() == C.N and ((used == C.N // 5) | (used == -(-C.N // 5))).all()     # floor or ceil of its share
    np.testing.assert_array_equal(res["log_weights"], lw)
    assert abs(res["ess"] - 5.0) <= 1e-9 and res["log_evidence"] == 0.0


# ---- determinism and reuse
def test_determinism_and_reuse_of_a_context():
    m, common, _, _ = C.call("B", "h2h-extra_time", table=True, with_lw=True)
    kw = dict(return_stages=True, return_weights=True)
    first = m.simulate_tournament(**kw, **common)
    again = m.simulate_tournament(**kw, **common)
    for k in first:
        np.testing.assert_array_equal(first[k], again[k], err_msg=k)
    other = m.simulate_tournament(**kw, **dict(common, random_state=C.SEED + 1))
    np.testing.assert_array_equal(other["log_weights"], first["log_weights"])
    assert (other["in_play_home_goals"] != first["in_play_home_goals"]).any()
    # an allocation set and cleared between live calls on one context
    ranked = m.simulate_tournament(**kw, **{k: v for k, v in common.items() if k != "best_allocation"})
    assert "best_slot_count" not in ranked
    np.testing.assert_array_equal(ranked["draw"], first["draw"])
    third = m.simulate_tournament(**kw, **common)
    for k in first:
        np.testing.assert_array_equal(first[k], third[k], err_msg=k)
    # a plain call after a live call is the plain call of a fresh context
    plain_kw = {k: v for k, v in common.items() if k not in ("in_play", "reweight", "log_weights")}
    plain_kw["group_fixtures"] = C.kick_off("B")[1]
    after = m.simulate_tournament(return_stages=True, **plain_kw)
    fresh_model = hand_posterior(type(m), T=9, S=40, seed=72)
    fresh = fresh_model.simulate_tournament(return_stages=True, **plain_kw)
    assert set(after) == set(fresh)
    for k in fresh:
        np.testing.assert_array_equal(after[k], fresh[k], err_msg=k)


# ---- the library's own refusals, through the raw binding
def test_the_library_refuses_malformed_requests():
    m, _, inp, dev = C.call("A", "overall-redraw", n_sims=64)
    ctx = m._device()
    p, q, gp, gq, t = inp["in_play"]

    def refused(in_play, **changes):
        kw = dict(dev["kwargs"], in_play=in_play, **changes)
        with pytest.raises(BplHipError) as e:
            ctx.simulate_tournament_live(*dev["args"], **kw)
        assert e.value.code == BPLHIP_EINVAL, (in_play, changes)

    for bad in (1.0, -0.25, float("nan")):
        refused((p, q, gp, gq, np.array([0.0, 0.5, bad])))
    refused((p, q, gp, gq, np.array([0.0, 0.0, 0.7])))                       # 1-0 at elapsed 0
    refused((p, q, np.array([0, 1, 64], dtype=np.uint8), gq, t))             # a goal count above 63
    refused((p, np.array([4, 1, 6], dtype=np.uint8), gp, gq, t))             # two sides of different groups
    refused((p, np.array([3, 0, 6], dtype=np.uint8), gp, gq, t))             # a team against itself (slot 0)
    limit = 1 << 20
    many = np.resize(dev["kwargs"]["fix_p"], limit - 2), np.resize(dev["kwargs"]["fix_q"], limit - 2)
    refused((p, q, gp, gq, t), fix_p=many[0], fix_q=many[1])                 # F + L over the limit
    refused((p, q, gp, gq, t), log_weights=np.full(300, np.inf))             # a non-finite log weight
    # matches in play without groups
    mc, _, _, devc = C.call("C", "overall-redraw", n_sims=64)
    with pytest.raises(BplHipError) as e:
        mc._device().simulate_tournament_live(*devc["args"], **dict(devc["kwargs"], in_play=(p, q, gp, gq, t)))
    assert e.value.code == BPLHIP_EINVAL
    # and the context still serves a well-formed call
    ok = ctx.simulate_tournament_live(*dev["args"], **dev["kwargs"])
    assert ok["stage_counts"].sum() == 64 * 8
