"""tournament_paths, tournament_scenarios and tournament_points with group matches in progress and weighted draws on
the device (csrc/dc_tournament_live_queries.hip.h): the kick-off identity, simulation j against the live
simulate_tournament's simulation j, the tables against the device's own records and against the numpy restatement
(tests/tournament_live_queries_ref.py), and the edges.  G1, G2 and G4 are exact; G3 excludes the restatement's flagged
simulations, of which tests/test_tournament_live_queries_host.py shows without a GPU that there are at most 1 %."""
import numpy as np
import pytest

import live_ref as LR
import paths_ref as PR
import tournament_live_queries_cases as Q
import tournament_live_queries_ref as QR
import tournament_live_ref as TLR
import tournament_points_ref as TP
import tournament_ref as TR
import tournament_scenarios_ref as TS
from bpl import paths as _paths
from bpl import scenarios as _scenarios
from bpl._ffi import BPLHIP_EINVAL, BplHipError
from bpl.base import _prng_key, leverage_from_counts, points_axis

pytestmark = pytest.mark.gpu

PATHS_TABLES = ("stage_count", "advance_count", "meet_count", "position_stage_count", "outcome_count", "target_count",
                "joint_count")
POINTS_FIVE = ("team_points_count", "team_target_count", "team_place_count", "place_points_count", "place_gap_count")
POINTS_REST = ("rest_count", "rest_through_count", "rest_rank_count")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _ids(c):
    return "-".join(str(v) for v in c)


def _same(a, b, keys=None, skip=()):
    for k in (keys if keys is not None else sorted(set(a) & set(b))):
        if k not in skip:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def _scen_kw(name):
    keys, caps = Q.KEYS[name]
    return {"fixtures": list(keys), "margin_cap": list(caps)}


# ---- G1: kick-off states are ordinary fixtures (fails on a library without the feature: no such keyword)
@pytest.mark.parametrize("name,mode_id,table", Q.KICK_OFF, ids=lambda v: str(v))
def test_kick_off_states_are_appended_fixtures_bit_for_bit(name, mode_id, table):
    states, pairs = Q.kick_off(name)
    m, common, inp, _ = Q.call(name, mode_id, table, in_play=states, reweight=False)
    plain = Q.plain(common, pairs)
    S, L = np.asarray(m.corr_coef).size, len(pairs)
    added = {"ess", "log_evidence"}
    for method, extra, more in (("tournament_paths", {"return_records": True}, {"in_play", "draw", "in_play_home_goals",
                                                                                 "in_play_away_goals"}),
                                ("tournament_scenarios", dict(_scen_kw(name), return_records=True),
                                 {"draw", "in_play_home_goals", "in_play_away_goals"}),
                                ("tournament_points", {}, set())):
        live = getattr(m, method)(**common, **extra)
        kick = getattr(m, method)(**plain, **extra)
        assert set(live) == set(kick) | added | more, method
        _same(live, kick)
        assert live["ess"] == float(S) and np.isnan(live["log_evidence"])
        if more:
            np.testing.assert_array_equal(live["draw"], np.arange(Q.N) % S)
            assert live["draw"].dtype == np.int32 and live["in_play_home_goals"].shape == (Q.N, L)
    F = len(common["group_fixtures"])
    np.testing.assert_array_equal(m.tournament_paths(**common)["in_play"], np.arange(F, F + L))


# ---- G2: simulation j is the live simulate_tournament's simulation j
@pytest.mark.parametrize("case", Q.GPU_CASES, ids=_ids)
def test_simulation_j_is_simulation_j(case):
    name, mode_id, table, with_lw = case
    m, common, inp, _ = Q.call(name, mode_id, table, with_lw)
    sim = m.simulate_tournament(return_stages=True, **common)
    shared = ["round_proba", "group_position_proba", "decided_proba", "ess", "log_evidence"]
    paths = m.tournament_paths(return_records=True, **common)
    _same(paths, sim, [k for k in shared if k in sim])
    _same(paths, sim, ["stage", "draw", "in_play_home_goals", "in_play_away_goals"] + (["decided"] if "decided" in sim else []))
    assert paths["draw"].dtype == np.int32 and paths["in_play_home_goals"].dtype == np.uint8
    if inp["group"] is None:
        for method, extra in (("tournament_scenarios", {"fixtures": [0]}), ("tournament_points", {})):
            with pytest.raises(ValueError):
                getattr(m, method)(**common, **extra)
        return
    F, L = inp["fix_p"].size, inp["in_play"][0].size
    margin = Q.listed_margin(paths)
    assert paths["group_outcome"].shape == (Q.N, F + L) and paths["fixtures"].shape == (F + L, 2)
    np.testing.assert_array_equal(paths["group_outcome"][:, F:], 1 - np.sign(margin))
    np.testing.assert_array_equal(paths["fixtures"][F:], np.stack(inp["in_play"][:2], axis=1))
    keys, caps = Q.KEYS[name]
    scen = m.tournament_scenarios(return_records=True, **common, **_scen_kw(name))
    _same(scen, sim, [k for k in shared if k in sim and k != "group_position_proba"])
    _same(scen, paths, ["draw", "in_play_home_goals", "in_play_away_goals"])
    # the scenario index: keys in play from the final scores, ordinary keys (cap 1 here) from tournament_paths' outcomes
    stride, _ = TS.strides(caps)
    want = np.zeros(Q.N, dtype=np.int64)
    for q, (f, c) in enumerate(zip(keys, caps)):
        if f >= F:
            cls = c - np.clip(margin[:, f - F], -c, c)
        else:
            assert c == 1
            cls = paths["group_outcome"][:, f].astype(np.int64)
        want += cls * stride[q]
    np.testing.assert_array_equal(scen["scenario"], want)
    assert scen["scenario"].dtype == np.uint32
    np.testing.assert_array_equal(scen["target_set"], QR.target_set(paths["stage"], paths["position"], inp["rounds"]))
    np.testing.assert_array_equal(scen["fixtures"], keys)
    np.testing.assert_array_equal(scen["home"], inp["teams"][paths["fixtures"][list(keys), 0]])
    pts = m.tournament_points(**common)
    _same(pts, sim, [k for k in shared if k in sim])


# ---- G3: the tables from the records, and against the restatement
@pytest.mark.parametrize("case", Q.REF_CASES, ids=_ids)
def test_tables_from_records_and_against_the_restatement(case):
    name, mode_id, table, with_lw = case
    m, common, inp, _ = Q.call(name, mode_id, table, with_lw)
    ref = Q.restatement(*case)
    keep = ~ref["flagged"]
    n_flagged, n = int(ref["flagged"].sum()), len(inp["teams"])
    print(f"{case}: flagged {n_flagged} of {Q.N}")
    assert n_flagged <= 0.01 * Q.N
    cat = QR.shown(inp, inp["in_play"])

    def close(got, want, what):
        # a flagged simulation may differ from the restatement: by at most one count per slot in any cell
        assert np.abs(np.asarray(got).astype(np.int64) - want).max(initial=0) <= n_flagged * n, what

    paths = m.tournament_paths(return_records=True, **common)
    for k in ("stage", "position", "group_outcome", "pair", "winner", "decided", "draw", "in_play_home_goals",
              "in_play_away_goals"):
        if k in ref:
            assert paths[k].dtype == ref[k].dtype and paths[k].shape == ref[k].shape, k
            np.testing.assert_array_equal(paths[k][keep], ref[k][keep], err_msg=k)
    mine = PR.counts(paths, cat)
    theirs = PR.counts(ref, cat)
    for k in PATHS_TABLES:
        if k in mine:
            np.testing.assert_array_equal(paths[k], mine[k], err_msg=k)
            close(paths[k], theirs[k], k)
    ps = paths["position_stage_count"] if inp["group"] is not None else None
    _same(paths, _paths.from_counts(paths["stage_count"], paths["advance_count"], Q.N, ps), skip=PATHS_TABLES)
    if "joint_count" in paths:
        _same(paths, leverage_from_counts(paths["outcome_count"], paths["target_count"], paths["joint_count"], Q.N))
    if inp["group"] is None:
        return
    keys, caps = Q.KEYS[name]
    scen = m.tournament_scenarios(return_records=True, **common, **_scen_kw(name))
    np.testing.assert_array_equal(scen["scenario"][keep], QR.scenario(ref["margin"], keys, caps)[keep])
    np.testing.assert_array_equal(scen["target_set"][keep], QR.target_set(ref["stage"], ref["position"], inp["rounds"])[keep])
    mine = TS.counts(scen, cat, keys, caps)
    theirs = TS.counts({"scenario": QR.scenario(ref["margin"], keys, caps),
                        "target_set": QR.target_set(ref["stage"], ref["position"], inp["rounds"])}, cat, keys, caps)
    for k in ("scenario_count", "joint_count"):
        np.testing.assert_array_equal(scen[k], mine[k], err_msg=k)
        close(scen[k], theirs[k], k)
    _same(scen, _scenarios.scenario_from_counts(scen["scenario_count"], scen["joint_count"], Q.N))
    pts = m.tournament_points(**common)
    points_min, n_bins = points_axis(inp["table"][:, 0], cat["fix_p"], cat["fix_q"], inp["points"])
    np.testing.assert_array_equal(pts["points"], points_min + np.arange(n_bins))
    mine = TP.counts(TP.records_from_paths(paths, cat), cat, points_min, n_bins)
    theirs = TP.counts(QR.points_records(ref), cat, points_min, n_bins, gd_cap=3)
    for k in POINTS_FIVE:
        np.testing.assert_array_equal(pts[k], mine[k], err_msg=k)
    for k in POINTS_FIVE + POINTS_REST:
        if k in theirs:
            assert pts[k].shape == theirs[k].shape, k
            close(pts[k], theirs[k], k)
    assert all(k in pts for k in POINTS_REST) == (inp["best_of_rest"] > 0)


# ---- G4: the edges
@pytest.mark.parametrize("mode_id", ["overall-redraw", "h2h-extra_time"])
def test_a_host_listed_second_keeps_the_listed_orientation(mode_id):
    ip = {"home_team": ["t00"], "away_team": ["t01"], "home_goals": [2], "away_goals": [1], "elapsed": [1.0 - 1e-9]}
    m, common, _, _ = Q.call("A", mode_id, in_play=ip)      # t01 is the host
    common = dict(common, group_fixtures=[], current_table=None)
    res = m.tournament_paths(return_records=True, **common)
    np.testing.assert_array_equal(res["in_play_home_goals"], 2)
    np.testing.assert_array_equal(res["in_play_away_goals"], 1)
    np.testing.assert_array_equal(res["fixtures"], [[0, 1]])
    np.testing.assert_array_equal(res["outcome_count"], [[Q.N, 0, 0]])      # one-hot on the current result
    np.testing.assert_array_equal(res["group_outcome"], 0)
    assert res["group_position_proba"][0, 0] == 1.0 and res["group_position_proba"][1, 3] == 1.0
    scen = m.tournament_scenarios(fixtures=[0], margin_cap=2, **common)
    np.testing.assert_array_equal(scen["scenario_count"], [0, Q.N, 0, 0, 0])   # "the first-listed side by one"
    assert scen["home"][0] == "t00" and scen["away"][0] == "t01"


def test_a_class_the_score_has_ruled_out_is_empty():
    # match 1 stands at 0-3 with the match all but over: of its 7 classes "the second-listed side by three or more" is
    # all that is left, the other six are ruled out
    ip = dict(Q.shape("B")[4], elapsed=[0.4, 1.0 - 1e-9])
    m, common, inp, _ = Q.call("B", "overall-redraw", in_play=ip)
    scen = m.tournament_scenarios(**common, **_scen_kw("B"))
    count = scen["scenario_count"].reshape(scen["shape"])
    assert count.sum() == Q.N and (count[:, :6] == 0).all() and count[:, 6].sum() == Q.N
    cond = scen["conditional_proba"].reshape(tuple(scen["shape"]) + scen["conditional_proba"].shape[1:])
    assert np.isnan(cond[:, :6]).all() and not np.isnan(cond[:, 6][count[:, 6] > 0]).any()
    first = _scenarios.marginal(scen, [0])
    np.testing.assert_array_equal(first["scenario_count"], count.sum(axis=1))
    np.testing.assert_array_equal(first["fixtures"], [0])
    assert _scenarios.format_table(scen, "t00", "round_0")
    assert _scenarios.coarsen(scen, 1)["scenario_count"].sum() == Q.N
    assert _scenarios.requirements(scen, "t07", "round_0").shape[1] == 2


@pytest.mark.parametrize("name", ["C", "A"])
def test_log_weights_alone_select_the_weighted_draws(name):
    m, common, inp, dev = Q.call(name, "overall-redraw", with_lw=True, in_play=None)
    assert inp["in_play"][0].size == 0
    res = m.tournament_paths(return_records=True, **common)
    L, L0 = LR.log_weights(TLR.state_loglik(TR.model_tables(m), inp, TLR.NO_PLAY), True, common["log_weights"])
    wt = LR.weights(L, L0)
    s, flagged = LR.resample(wt["C"], Q.N, _prng_key(Q.SEED))
    assert not flagged.any()
    np.testing.assert_array_equal(res["draw"], s)
    assert len(np.unique(res["draw"])) > 1 and (res["draw"] != np.arange(Q.N) % L.size).any()
    assert res["log_evidence"] == 0.0 and abs(res["ess"] - wt["ess"]) <= 1e-9 * wt["ess"]
    assert res["in_play"].size == 0 and res["in_play_home_goals"].shape == (Q.N, 0)
    sim = m.simulate_tournament(return_stages=True, **common)
    _same(res, sim, ["stage", "draw", "round_proba", "ess"])
    if name == "A":
        np.testing.assert_array_equal(m.tournament_points(**common)["round_proba"], sim["round_proba"])


def test_determinism_reuse_and_the_chunk_size():
    name = "A2"
    m, common, inp, dev = Q.call(name, "h2h-extra_time", with_lw=True)
    keys, caps = Q.KEYS[name]
    first = {"p": m.tournament_paths(return_records=True, **common),
             "s": m.tournament_scenarios(return_records=True, **common, **_scen_kw(name)),
             "g": m.tournament_points(**common)}
    again = {"p": m.tournament_paths(return_records=True, **common),
             "s": m.tournament_scenarios(return_records=True, **common, **_scen_kw(name)),
             "g": m.tournament_points(**common)}
    for q in first:
        assert set(first[q]) == set(again[q])
        _same(first[q], again[q])
    # two chunk sizes through the raw bindings: neither a multiple of the other, the last chunk short
    ctx = m._device()
    cat = QR.shown(inp, inp["in_play"])
    points_min, n_bins = points_axis(inp["table"][:, 0], cat["fix_p"], cat["fix_q"], inp["points"])
    calls = (("tournament_paths_live", dict(return_records=True)),
             ("tournament_scenarios_live", dict(return_records=True, key_fixture=keys, key_cap=caps)),
             ("tournament_points_live", dict(points_min=points_min, n_bins=n_bins, gd_cap=3)))
    for method, extra in calls:
        a = getattr(ctx, method)(*dev["args"], chunk_sims=192, **extra, **dev["kwargs"])
        b = getattr(ctx, method)(*dev["args"], chunk_sims=704, **extra, **dev["kwargs"])
        assert set(a) == set(b)
        _same(a, b)
    # a kick-off call after the live calls is the kick-off call of before
    kick = m.tournament_paths(**Q.plain(common))
    assert "ess" not in kick and kick["fixtures"].shape == (62, 2)


def test_the_library_refuses_malformed_requests():
    m, _, inp, dev = Q.call("A", "overall-redraw", n_sims=64)
    ctx = m._device()
    p, q, gp, gq, t = inp["in_play"]
    cat = QR.shown(inp, inp["in_play"])
    points_min, n_bins = points_axis(inp["table"][:, 0], cat["fix_p"], cat["fix_q"], inp["points"])
    keys, caps = Q.KEYS["A"]
    mc, _, _, devc = Q.call("C", "overall-redraw", n_sims=64)
    limit = 1 << 20
    many = np.resize(dev["kwargs"]["fix_p"], limit - 2), np.resize(dev["kwargs"]["fix_q"], limit - 2)
    for method, extra, most in (("tournament_paths_live", {}, 4096),
                                ("tournament_scenarios_live", dict(key_fixture=keys, key_cap=caps), limit),
                                ("tournament_points_live", dict(points_min=points_min, n_bins=n_bins, gd_cap=3), limit)):
        def refused(in_play, context=ctx, device=dev, **changes):
            kw = dict(device["kwargs"], in_play=in_play, **changes)
            with pytest.raises(BplHipError) as e:
                getattr(context, method)(*device["args"], **extra, **kw)
            assert e.value.code == BPLHIP_EINVAL, (method, in_play, changes)

        refused((p, q, gp, gq, np.array([0.0, 0.5, float("nan")])))              # a malformed state
        refused((p, q, gp, gq, np.array([0.0, 0.0, 0.7])))                       # 1-0 at elapsed 0
        refused((p, q, np.array([0, 1, 64], dtype=np.uint8), gq, t))             # a goal count above 63
        refused((p, np.array([4, 1, 6], dtype=np.uint8), gp, gq, t))             # two sides of different groups
        refused((p, q, gp, gq, t), log_weights=np.full(300, np.inf))             # a non-finite log weight
        big = dict(fix_p=many[0][:most - 2], fix_q=many[1][:most - 2])
        if method == "tournament_points_live":
            big.update(points_min=0, n_bins=256)                                 # (refused before the axis is read)
            extra = {k: v for k, v in extra.items() if k not in big}
        refused((p, q, gp, gq, t), **big)                                        # F + L over the limit
        # matches in play without groups
        without = dict(extra, key_fixture=[0], key_cap=[1]) if "key_cap" in extra else extra
        with pytest.raises(BplHipError) as e:
            getattr(mc._device(), method)(*devc["args"], **without, **dict(devc["kwargs"], in_play=(p, q, gp, gq, t)))
        assert e.value.code == BPLHIP_EINVAL
    # and the context still serves a well-formed call
    ok = ctx.tournament_paths_live(*dev["args"], **dev["kwargs"])
    assert ok["stage_counts"].sum() == 64 * 8 and ok["ess"] > 0.0
