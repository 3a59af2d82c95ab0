"""tournament_paths without a GPU: the argument checks (simulate_tournament's, all before any device call), the floats
from small hand-made integer tables, the helpers of bpl/paths.py, the restatement's invariants on a CPU run, the
public method's keys through a stand-in device in the manner of tests/fake_ctx.py, and the header's new symbol."""
import os
import re

import numpy as np
import pytest

import paths_ref as P
import tournament_ref as R
from bpl import NeutralDixonColesMatchPredictor, NeutralDixonColesMatchPredictorWC, _ffi, paths
from bpl.base import _prng_key
from fake_ctx import FakePredictCtx
from test_tournament_host import conf_of, hand_posterior

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class PathsCtx(FakePredictCtx):
    """TEST-ONLY stand-in for HipContext.tournament_paths: records the call and answers with the restatement's
    records (tests/paths_ref.py) cross-tabulated into the raw tables the device returns."""

    def __init__(self, model, inp, seed):
        self.model, self.inp, self.seed, self.calls = model, inp, seed, []

    def tournament_paths(self, team_idx, bracket, n_sims, key, return_records=False, **kwargs):
        self.calls.append(dict(kwargs, team_idx=team_idx, bracket=bracket, n_sims=n_sims, key=key,
                               return_records=return_records))
        inp = self.inp
        assert tuple(key) == tuple(_prng_key(self.seed)) and n_sims == inp["num_simulations"]
        rec = P.simulate(R.model_tables(self.model), inp, key, head_to_head=kwargs.get("head_to_head", False))
        c = P.counts(rec, inp)
        n, Rr = len(inp["teams"]), inp["rounds"]
        raw = {"stage_counts": c["stage_count"].astype(np.uint64), "advance": c["advance_count"].astype(np.uint64)}
        if inp["group"] is not None:
            ps = np.zeros((n, 8, 8), dtype=np.uint64)
            ps[:, :inp["group_size"], :Rr + 2] = c["position_stage_count"]
            raw["position_stage"], raw["position_counts"] = ps, ps.sum(axis=2)
        if "joint_count" in c:
            raw.update(outcome=c["outcome_count"], target=c["target_count"], joint=c["joint_count"])
        if "decided" in rec:
            k0, dc = 0, np.zeros((Rr, 4), dtype=np.uint64)
            for r in range(Rr):
                M = (1 << Rr) >> (r + 1)
                dc[r] = np.bincount(rec["decided"][:, k0:k0 + M].ravel(), minlength=4)
                k0 += M
            raw["decided_counts"] = dc
        if return_records:
            raw.update({k: v for k, v in rec.items() if k != "flagged"})
        return raw


def _raises(m, *args, **kwargs):
    with pytest.raises(ValueError):
        m.tournament_paths(*args, **kwargs)
    assert m._predict_ctx is None   # no device context was ever made


def test_argument_errors_are_simulate_tournaments_and_come_before_the_device():
    m = hand_posterior()
    t = list(m.teams)
    euro = R.euro_24(t)
    groups, ko = euro["groups"], euro["knockout"]
    kw = dict(advance=2, best_of_rest=4, num_simulations=10)
    _raises(m, ["t00", "nope"])
    _raises(m, ko, {**groups, "A": ["t00", "nope", "t02", "t03"]}, **kw)
    _raises(m, ko, groups, hosts=["t60"], **kw)
    _raises(m, ko, groups, current_table={"t60": (1, 1, 1)}, **kw)
    _raises(m, ko, groups, group_fixtures=[("t00", "t04")], **kw)
    _raises(m, ko, {**groups, "B": ["t00", "t05", "t06", "t07"]}, **kw)
    _raises(m, t[:3])
    _raises(m, ["t00", "t00"])
    bad = list(ko)
    bad[0] = ("A", 3)
    _raises(m, bad, groups, **kw)
    _raises(m, ko, groups, advance=2, best_of_rest=2, num_simulations=10)
    _raises(m, t[:4], group_fixtures=[("t00", "t01")])
    _raises(m, ko, groups, points=(3, -1, 0), **kw)
    for n in (0, 2 ** 31, 1.5, True):
        _raises(m, t[:4], num_simulations=n)
    _raises(m, t[:4], team_conf=conf_of(m))
    # the tie-break, the played matches and the knockout rule
    _raises(m, t[:4], tiebreak="coin")
    _raises(m, t[:4], played={"home_team": ["t00"], "away_team": ["t01"], "home_goals": [1], "away_goals": [0]})
    _raises(m, ko, groups, played={"home_team": ["t00"], "away_team": ["t04"], "home_goals": [1], "away_goals": [0]},
            **kw)
    _raises(m, t[:4], knockout_rule="golden_goal")
    _raises(m, t[:4], legs=2)                                    # needs "extra_time"
    _raises(m, t[:4], knockout_rule="extra_time", legs=(1, 2, 1))
    _raises(m, t[:4], knockout_rule="extra_time", extra_time_scale=0.0)
    _raises(m, t[:4], knockout_rule="extra_time", shootout={"t00": float("nan")})
    _raises(m, t[:4], knockout_rule="extra_time", away_goals=1)
    _raises(m, t[:4], return_records=1)
    w = hand_posterior(NeutralDixonColesMatchPredictorWC)
    _raises(w, t[:4])
    _raises(w, t[:4], team_conf={**conf_of(w), "t03": "CONMEBOL"})


def test_floats_from_hand_made_tables():
    # n = 3 slots, R = 2 rounds, N = 10: slot 2 never plays the final, slots 0 and 1 never meet in round 0
    stage = np.array([[0, 4, 2, 4], [2, 2, 4, 2], [5, 5, 0, 0]])          # furthest stage 0..3
    adv = np.zeros((2, 3, 3), dtype=np.int64)
    adv[0, 0, 2], adv[0, 2, 0], adv[0, 1, 2] = 5, 1, 2
    adv[1, 0, 1], adv[1, 1, 0] = 4, 2
    ps = np.zeros((3, 2, 4), dtype=np.int64)
    ps[0, 0], ps[1, 0], ps[1, 1], ps[2, 1] = stage[0], [0, 1, 4, 2], [2, 1, 0, 0], stage[2]
    out = paths.from_counts(stage, adv, 10, ps)
    np.testing.assert_array_equal(out["meet_count"][0], [[0, 0, 6], [0, 0, 2], [6, 2, 0]])
    np.testing.assert_array_equal(out["meet_count"][1], [[0, 6, 0], [6, 0, 0], [0, 0, 0]])
    np.testing.assert_array_equal(out["meet_proba"], out["meet_count"] / 10)
    # slot 0 plays round 0 in 10 simulations and the final in 6; slot 2 plays round 0 in 5 and never the final
    np.testing.assert_array_equal(out["opponent_proba"][0, 0], [0.0, 0.0, 6 / 10])
    np.testing.assert_array_equal(out["opponent_proba"][1, 0], [0.0, 6 / 6, 0.0])
    np.testing.assert_array_equal(out["opponent_proba"][0, 2], [6 / 5, 2 / 5, 0.0])   # (hand numbers, not a tournament)
    assert np.isnan(out["opponent_proba"][1, 2]).all()
    given = out["advance_given_meet"]
    assert given[0, 0, 2] == 5 / 6 and given[0, 2, 0] == 1 / 6 and given[1, 1, 0] == 2 / 6
    assert np.isnan(given[0, 0, 1]) and np.isnan(given[1, 2, 2]) and np.isnan(given[0, 0, 0])
    assert np.isnan(given).sum() == 18 - 6
    rp = out["round_proba_given_position"]
    assert rp.shape == (3, 2, 3)
    np.testing.assert_array_equal(rp[1, 0], [7 / 7, 6 / 7, 2 / 7])
    np.testing.assert_array_equal(rp[1, 1], [1 / 3, 0.0, 0.0])
    assert np.isnan(rp[0, 1]).all() and np.isnan(rp[2, 0]).all()
    np.testing.assert_array_equal(rp[2, 1], [0.5, 0.0, 0.0])
    assert "round_proba_given_position" not in paths.from_counts(stage, adv, 10)
    assert list(paths.target_names(2)) == ["round_0", "round_1", "winner"]


def _hand_result():
    stage = np.array([[0, 2, 2, 6], [0, 3, 5, 2], [1, 6, 3, 0], [9, 1, 0, 0]])
    adv = np.zeros((2, 4, 4), dtype=np.int64)
    adv[0, 0, 1], adv[0, 0, 2], adv[0, 1, 0], adv[0, 2, 3] = 5, 3, 2, 1
    adv[1, 0, 1], adv[1, 1, 0], adv[1, 0, 2] = 4, 1, 2
    res = {"teams": np.array(["ant", "bee", "cat", "dog"]), "targets": paths.target_names(2)}
    res.update(paths.from_counts(stage, adv, 10))
    reached = np.cumsum(stage[:, ::-1], axis=1)[:, ::-1]
    res["round_proba"] = reached[:, 1:] / 10
    return res


def test_opponents_and_format_table():
    res = _hand_result()
    opp = paths.opponents(res, "ant", top=2)
    assert [[name for name, _ in rnd] for rnd in opp] == [["bee", "cat"], ["bee", "cat"]]
    assert opp[0][0][1] == 7 / 10 and opp[0][1][1] == 3 / 10 and opp[1][0][1] == 5 / 8
    assert paths.opponents(res, "dog") == [[("cat", 1.0)], []]
    assert len(paths.opponents(res, "ant", top=1)[0]) == 1
    assert paths.most_likely_final(res) == ("ant", "bee", 0.5)
    for bad in (0, True, 1.5):
        with pytest.raises(ValueError):
            paths.opponents(res, "ant", top=bad)
    with pytest.raises(ValueError):
        paths.opponents(res, "eel")
    text = paths.format_table(res, "ant")
    assert text.splitlines()[0] == "ant" and "round_0" in text and "winner" in text and "v bee" in text
    assert "group place" not in text
    assert "71.4%" in text   # P(ant goes through | meets bee in round 0) = 5 / 7


def _cpu_case(rule=None, tiebreak="overall", hosts=None):
    m = hand_posterior(T=16, S=8, seed=21)
    kw = R.group_format(list(m.teams), 3, 4, 2, seed=4)
    # mid-tournament orientation: a host listed second
    kw["group_fixtures"] = [(g[i], g[k]) for g in kw["groups"].values() for i in range(4) for k in range(i + 1, 4)]
    rule = rule or {}
    inp = m._tournament_inputs(kw["knockout"], kw["groups"], 2, 2, kw["group_fixtures"], None, hosts, (3, 1, 0), 400,
                               None, **rule)
    return m, kw, inp


@pytest.mark.parametrize("rule,tiebreak", [
    ({}, "overall"), ({}, "head_to_head"),
    (dict(knockout_rule="extra_time", legs=(2, 1, 1), away_goals=True), "overall")])
def test_restatement_invariants_on_a_cpu_run(rule, tiebreak):
    m, kw, inp = _cpu_case(rule, hosts=["t01", "t06"])
    rec = P.simulate(R.model_tables(m), inp, _prng_key(8), head_to_head=tiebreak == "head_to_head")
    N, n, Rr = 400, 12, 3
    assert rec["pair"].shape == (N, 7, 2) and rec["winner"].shape == (N, 7) and rec["group_outcome"].shape == (N, 18)
    assert ("decided" in rec) == bool(rule)
    c = P.counts(rec, inp)
    reached = np.cumsum(c["stage_count"][:, ::-1], axis=1)[:, ::-1][:, 1:]
    np.testing.assert_array_equal(c["meet_count"].sum(axis=2), reached[:, :Rr].T)
    np.testing.assert_array_equal(c["meet_count"].sum(axis=(1, 2)), [8 * N, 4 * N, 2 * N])
    np.testing.assert_array_equal(c["position_stage_count"].sum(axis=1), c["stage_count"])
    np.testing.assert_array_equal(c["position_stage_count"].sum(axis=(1, 2)), N)
    np.testing.assert_array_equal(c["joint_count"].sum(axis=1), np.broadcast_to(c["target_count"], (18, n, Rr + 1)))
    np.testing.assert_array_equal(c["target_count"], reached)
    np.testing.assert_array_equal(c["outcome_count"].sum(axis=1), N)
    # the places that qualify do: first and second always, third as one of the two best
    pos, stage = rec["position"].astype(int), rec["stage"].astype(int)
    assert (stage[pos < 2] >= 1).all() and (stage[pos == 3] == 0).all()
    assert ((pos == 2) & (stage >= 1)).sum() == 2 * N
    # the final pairs the semi-finals' winners
    np.testing.assert_array_equal(rec["pair"][:, 6], rec["winner"][:, 4:6])
    # a group fixture's outcome is in the listed order: the points of its first-listed side follow it
    if not rule and tiebreak == "overall":
        plain, _, inp0 = _cpu_case()
        rec0 = P.simulate(R.model_tables(plain), inp0, _prng_key(8))
        assert not np.array_equal(rec0["group_outcome"], rec["group_outcome"])   # the hosts change scorelines


def test_public_method_through_a_stand_in_device():
    m, kw, inp = _cpu_case(hosts=["t01"])
    m._predict_ctx = ctx = PathsCtx(m, inp, 5)
    m._uploaded = None
    res = m.tournament_paths(num_simulations=400, random_state=5, hosts=["t01"], return_records=True, **kw)
    call = ctx.calls[0]
    assert call["return_records"] is True and call["advance"] == 2 and call["best_of_rest"] == 2
    np.testing.assert_array_equal(call["fix_p"], inp["fix_p"])
    n, Rr, nf, Pmax = 12, 3, 18, 4
    shapes = {"teams": (n,), "targets": (Rr + 1,), "fixtures": (nf, 2), "round_proba": (n, Rr + 1),
              "group_position_proba": (n, Pmax), "stage_count": (n, Rr + 2), "meet_count": (Rr, n, n),
              "advance_count": (Rr, n, n), "meet_proba": (Rr, n, n), "opponent_proba": (Rr, n, n),
              "advance_given_meet": (Rr, n, n), "position_stage_count": (n, Pmax, Rr + 2),
              "round_proba_given_position": (n, Pmax, Rr + 1), "outcome_count": (nf, 3), "outcome_proba": (nf, 3),
              "target_count": (n, Rr + 1), "target_proba": (n, Rr + 1), "joint_count": (nf, 3, n, Rr + 1),
              "conditional_proba": (nf, 3, n, Rr + 1), "conditional_se": (nf, 3, n, Rr + 1),
              "leverage": (nf, n, Rr + 1),
              "stage": (400, n), "position": (400, n), "group_outcome": (400, nf), "pair": (400, 7, 2),
              "winner": (400, 7)}
    assert {k: v.shape for k, v in res.items()} == shapes
    for k in ("stage_count", "meet_count", "advance_count", "position_stage_count", "outcome_count", "target_count",
              "joint_count"):
        assert res[k].dtype == np.int64, k
    np.testing.assert_array_equal(res["target_proba"], res["round_proba"])
    # a team's opponents in a round it plays sum to one; the value of first place is a probability
    opp = res["opponent_proba"]
    np.testing.assert_allclose(np.nansum(opp, axis=2)[~np.isnan(opp).all(axis=2)], 1.0, atol=1e-12)
    given = res["round_proba_given_position"]
    assert np.nanmax(given) <= 1.0 and (given[:, :2, 0][~np.isnan(given[:, :2, 0])] == 1.0).all()
    assert "group place" in paths.format_table(res, "t01")
    # without records, and knockout only: the keys that need groups or records are absent
    ko_inp = m._tournament_inputs(list(m.teams[:4]), None, 2, 0, None, None, None, (3, 1, 0), 50, None)
    m._predict_ctx = PathsCtx(m, ko_inp, 6)
    res = m.tournament_paths(list(m.teams[:4]), num_simulations=50, random_state=6)
    assert set(res) == {"teams", "targets", "round_proba", "stage_count", "meet_count", "advance_count", "meet_proba",
                        "opponent_proba", "advance_given_meet"}
    m._predict_ctx = None


def test_header_declares_the_new_symbol():
    header = open(os.path.join(ROOT, "include", "bplhip.h")).read()
    declared = set(re.findall(r"\b(bplhip_[a-z_0-9]+)\s*\(", header)) - {"bplhip_ctx"}
    assert "bplhip_tournament_paths" in declared and declared == set(_ffi.ABI_SYMBOLS)
    decl = re.search(r"int bplhip_tournament_paths\((.*?)\);", header, re.S).group(1)
    params = [p.strip() for p in decl.split(",")]
    restype, argtypes = _ffi._SIGNATURES["bplhip_tournament_paths"]
    assert len(params) == len(argtypes) == 46
    assert [a is _ffi._vp for a in argtypes] == ["*" in p for p in params]
    knockout = re.search(r"int bplhip_simulate_tournament_knockout\((.*?)\);", header, re.S).group(1)
    theirs = [p.strip().split()[-1].lstrip("*") for p in knockout.split(",")]
    ours = [p.split()[-1].lstrip("*") for p in params]
    assert ours[:29] == theirs[:29] and ours[29] == "extra_time" and ours[30:36] == theirs[29:]
    assert ours[36:] == ["chunk_sims", "advance_counts", "position_stage_counts", "outcome_counts", "target_counts",
                         "joint_counts", "sim_position", "sim_outcome", "sim_pair", "sim_winner"]
    assert _ffi.load_library().bplhip_tournament_paths is not None
    assert int(re.search(r"#define BPLHIP_ABI_VERSION (\d+)", header).group(1)) == 2 == _ffi.ABI_VERSION
