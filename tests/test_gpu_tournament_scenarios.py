"""tournament_scenarios on the device (csrc/dc_tscen.hip.h): its per-simulation records against the numpy restatement
(tests/tournament_scenarios_ref.py) on the simulations the restatement does not flag, in all four modes; its integer
tables against the pure cross-tabulation of its own records, exactly and over all simulations; its identity with
tournament_paths and simulate_tournament under one random_state, device against device; the shapes at which the kernel
can go wrong; the independence of the chunk; and the context and argument errors.  Integers only.

Every case's seed and shape were run through the restatement on the CPU first: its flagged share stays inside
1e-3 N, tests/test_gpu_paths.py's cap."""
import numpy as np
import pytest

import tournament_ref as R
import tournament_scenarios_ref as S
from bpl import NeutralDixonColesMatchPredictorWC, scenarios
from bpl._ffi import BPLHIP_EINVAL, BPLHIP_ESTATE, BplHipError, HipContext, _np_ptr
from bpl.base import _prng_key
from test_gpu_paths import _cycled
from test_gpu_tournament import _format
from test_tournament_host import conf_of, hand_posterior

pytestmark = pytest.mark.gpu
N, SEED, DRAWS = 2003, 4321, 7          # N mod DRAWS = 1: the draws do not divide the simulations
ET = dict(knockout_rule="extra_time")
MODES = [("overall", {}), ("head_to_head", {}),
         ("overall", dict(legs=(2, 1), away_goals=True, shootout={"t01": 0.8, "t06": -0.4}, **ET)),
         ("head_to_head", dict(legs=(1, 2), shootout={"t03": 1.5}, **ET))]
MODE_IDS = ["overall-redraw", "h2h-redraw", "overall-extra_time", "h2h-extra_time"]
DERIVED = ("scenario_count", "joint_count", "target_count", "scenario_proba", "target_proba", "conditional_proba",
           "conditional_se", "settled", "leverage", "margins", "fixtures", "home", "away", "margin_cap")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def shape(name):
    """(model, simulate_tournament kwargs, hosts, key fixtures, caps) of a case."""
    if name == "two_groups":
        # two groups of 4, R = 2; t01 is a host and listed second in key fixture 0 (t00 v t01)
        m = hand_posterior(T=8, S=DRAWS, seed=31)
        kw = {"groups": {"A": list(m.teams[:4]), "B": list(m.teams[4:])}, "advance": 2,
              "knockout": [("A", 1), ("B", 2), ("B", 1), ("A", 2)]}
        return m, kw, ["t01"], [0, 5, 11], [2, 1, 3]
    if name == "fixtures70":
        # 70 group fixtures (the round robins gone through again and again): keys in both blocks of 64, at the
        # block boundary and on the last lane in use
        m = hand_posterior(T=20, S=DRAWS, seed=32)
        kw = R.group_format(list(m.teams), 4, 4, 0, seed=1)
        kw["group_fixtures"] = _cycled(kw["groups"], 70)
        return m, kw, None, [0, 63, 64, 69], [1, 2, 1, 3]
    if name == "keys8":
        m, kw, hosts, _, _ = shape("two_groups")
        return m, kw, hosts, [3, 0, 11, 7, 6, 1, 9, 4], [1] * 8
    if name == "caps3":
        m, kw, hosts, _, _ = shape("two_groups")
        return m, kw, hosts, [10, 0, 4], [3, 3, 3]
    if name == "16x4":
        # n = 64, R = 5, K = 7: the widest rows of the counting kernel, several tiles
        m = hand_posterior(T=64, S=DRAWS, seed=33)
        return m, R.group_format(list(m.teams), 16, 4, 0, seed=2), ["t62"], [91, 0, 64], [3, 3, 1]
    if name == "last_matchday":
        # a Euro after two of its three group matchdays: the current table and the last matchday's fixtures only;
        # the keys are group A's two final matches
        m = hand_posterior(T=24, S=DRAWS, seed=34)
        return m, _format("mid", list(m.teams)), None, [0, 6], [3, 3]
    if name == "never":
        # t00 scores freely and concedes next to nothing: "the second-listed side wins" never occurs in fixture 0
        m, kw, hosts, _, _ = shape("two_groups")
        m.attack[:, 0] += 1.5
        m.defence[:, 0] += 8.0
        return m, kw, None, [0, 9], [3, 1]
    if name == "wc":
        # the World-Cup class: confederation strengths in every rate; 3 groups of 4 and the two best thirds, R = 3
        m = hand_posterior(NeutralDixonColesMatchPredictorWC, T=12, S=DRAWS, seed=35)
        return m, R.group_format(list(m.teams), 3, 4, 2, seed=5), ["t06"], [7, 17, 3], [1, 2, 2]     # 7: t04 v t06
    if name == "played_h2h":
        # the real last matchday: two matchdays played (they fill the table and, under the head-to-head order, the
        # pair records), the final pair of fixtures of each group left; t03 is a host, listed second in key 0
        m, kw, _, _, _ = shape("two_groups")
        home = ["t00", "t02", "t00", "t01", "t04", "t06", "t04", "t05"]
        away = ["t01", "t03", "t02", "t03", "t05", "t07", "t06", "t07"]
        kw["played"] = {"home_team": home, "away_team": away, "home_goals": [1, 0, 2, 1, 0, 1, 1, 0],
                        "away_goals": [1, 0, 1, 0, 2, 1, 1, 0]}
        kw["group_fixtures"] = [("t00", "t03"), ("t01", "t02"), ("t04", "t07"), ("t05", "t06")]
        return m, kw, ["t03"], [0, 1], [3, 3]
    raise KeyError(name)


def _call(m, kw, hosts, tiebreak, rule, n_sims=N, seed=SEED):
    """(the public call's keywords, the checked inputs, the head-to-head records or None), the last two as the
    public call itself forms them."""
    conf = conf_of(m) if isinstance(m, NeutralDixonColesMatchPredictorWC) else None
    common = dict(num_simulations=n_sims, random_state=seed, hosts=hosts, team_conf=conf, tiebreak=tiebreak, **kw,
                  **rule)
    inp, call = m._tournament_call(kw["knockout"], kw.get("groups"), kw.get("advance", 2), kw.get("best_of_rest", 0),
                                   kw.get("group_fixtures"), kw.get("current_table"), hosts, (3, 1, 0), n_sims, seed,
                                   conf, tiebreak, kw.get("played"), rule.get("knockout_rule", "redraw"),
                                   rule.get("legs"), rule.get("extra_time_scale", 1 / 3), rule.get("shootout"),
                                   rule.get("away_goals", False))
    return common, inp, call["kwargs"].get("pair_init")


def _check_own_tables(res, inp, keys, caps):
    """The device's tables are the pure cross-tabulation of the device's own records: exact, over all simulations."""
    want = S.counts({"scenario": res["scenario"], "target_set": res["target_set"]}, inp, keys, caps)
    for k, v in want.items():
        assert res[k].dtype == np.int64 and res[k].shape == v.shape, k
        np.testing.assert_array_equal(res[k], v, err_msg=k)
    assert res["scenario_count"].sum() == inp["num_simulations"]
    Rr = inp["rounds"]
    np.testing.assert_array_equal(res["target_count"][:, Rr + 1].sum(), inp["num_simulations"] * len(inp["group_names"]))
    np.testing.assert_array_equal(res["target_count"][:, :Rr + 1].sum(axis=0),
                                  inp["num_simulations"] * (1 << np.arange(Rr, -1, -1)))


def _check_against_restatement(name, tiebreak="overall", rule=None):
    m, kw, hosts, keys, caps = shape(name)
    rule = rule or {}
    common, inp, pair = _call(m, kw, hosts, tiebreak, rule)
    res = m.tournament_scenarios(fixtures=keys, margin_cap=caps, return_records=True, **common)
    ref = S.simulate(R.model_tables(m), inp, _prng_key(SEED), keys, caps, head_to_head=tiebreak == "head_to_head",
                     pair_init=pair)
    keep = ~ref["flagged"]
    print(f"{name}: {ref['flagged'].sum()} of {N} flagged")
    assert ref["flagged"].sum() <= 1e-3 * N, ref["flagged"].sum()
    for k in ("scenario", "target_set"):
        assert res[k].dtype == ref[k].dtype and res[k].shape == ref[k].shape, k
        np.testing.assert_array_equal(res[k][keep], ref[k][keep], err_msg=k)
    _check_own_tables(res, inp, keys, caps)
    return m, res, inp, ref


# ---- 1. records against the restatement, tables from the device's own records: all four of H2H x ET
@pytest.mark.parametrize("tiebreak,rule", MODES, ids=MODE_IDS)
def test_records_against_restatement(tiebreak, rule):
    m, res, inp, ref = _check_against_restatement("two_groups", tiebreak, rule)
    assert list(res["teams"]) == list(m.teams) and res["shape"] == (5, 3, 7)
    assert list(res["targets"]) == ["round_0", "round_1", "winner", "group_winner"]
    assert list(res["home"]) == ["t00", "t02", "t06"] and list(res["away"]) == ["t01", "t03", "t07"]
    assert ("decided_proba" in res) == bool(rule)
    # the host listed second plays at home and keeps the listed orientation: without it the scorelines differ
    common, _, _ = _call(m, shape("two_groups")[1], None, tiebreak, rule)
    plain = m.tournament_scenarios(fixtures=[0, 5, 11], margin_cap=[2, 1, 3], return_records=True, **common)
    assert not np.array_equal(plain["scenario"], res["scenario"])


# ---- 2. consistency with the existing calls, under one random_state
@pytest.mark.parametrize("tiebreak,rule", MODES, ids=MODE_IDS)
def test_consistency_with_paths_and_simulate_tournament(tiebreak, rule):
    m, kw, hosts, _, _ = shape("two_groups")
    common, inp, _ = _call(m, kw, hosts, tiebreak, rule)
    Rr = inp["rounds"]
    paths = m.tournament_paths(**common)
    sim = m.simulate_tournament(**common)
    for f in (0, 7):       # the host's fixture (listed second, at home) and a neutral one
        res = m.tournament_scenarios(fixtures=[f], margin_cap=1, **common)
        np.testing.assert_array_equal(res["scenario_count"], paths["outcome_count"][f])
        np.testing.assert_array_equal(res["joint_count"][:, :, :Rr + 1], paths["joint_count"][f])
        np.testing.assert_array_equal(res["target_count"][:, :Rr + 1], paths["target_count"])
        assert res["round_proba"].dtype == sim["round_proba"].dtype
        np.testing.assert_array_equal(res["round_proba"], sim["round_proba"])
        assert ("decided_proba" in res) == ("decided_proba" in sim) == bool(rule)
        if rule:
            np.testing.assert_array_equal(res["decided_proba"], sim["decided_proba"])
        first = res["target_count"][:, Rr + 1]
        np.testing.assert_array_equal(first / N, sim["group_position_proba"][:, 0])
        np.testing.assert_array_equal(first, np.rint(N * sim["group_position_proba"][:, 0]).astype(np.int64))
        np.testing.assert_array_equal(first, paths["position_stage_count"][:, 0].sum(axis=1))


# ---- 3. where the kernel can go wrong
@pytest.mark.parametrize("name", ["fixtures70", "keys8", "caps3", "16x4", "last_matchday", "wc", "played_h2h"])
def test_shapes(name):
    tiebreak = "head_to_head" if name in ("16x4", "played_h2h") else "overall"
    rule = ET if name in ("fixtures70", "wc") else {}
    m, res, inp, _ = _check_against_restatement(name, tiebreak, rule)
    _, _, _, keys, caps = shape(name)
    n, K = len(inp["teams"]), inp["rounds"] + 2
    M = int(np.prod([2 * c + 1 for c in caps]))
    assert res["joint_count"].shape == (M, n, K) and res["conditional_proba"].shape == (M, n, K)
    np.testing.assert_array_equal(res["fixtures"], keys)
    if name == "fixtures70":
        assert len(inp["fix_p"]) == 70
    if name == "keys8":
        assert M == 6561 and (res["scenario_count"] > 0).sum() > 500     # spread over the count tiles
    if name == "16x4":
        assert (n, K) == (64, 7) and res["home"][0] == "t60" and res["away"][0] == "t62"    # the host, listed second
    if name == "last_matchday":
        assert len(inp["fix_p"]) == 12 and inp["table"].any()
    if name == "wc":
        assert inp["conf"] is not None and "decided_proba" in res
    if name == "played_h2h":
        # the table comes from the played matches, and so do the pair records of the head-to-head order
        np.testing.assert_array_equal(inp["table"][:4], [[4, 3, 2], [4, 2, 1], [1, 1, 2], [1, 0, 1]])
        assert res["away"][0] == "t03" and res["shape"] == (7, 7)


def test_a_class_that_never_occurs():
    m, res, inp, _ = _check_against_restatement("never")
    sc = res["scenario_count"].reshape(res["shape"])
    # fixture 0: t01 never beats t00 (margin classes 4 .. 6 of cap 3: the second-listed side by 1, 2, 3 or more)
    assert not sc[4:].any() and sc[:4].sum() == N
    gone = (res["scenario_count"] == 0)[:, None, None] & np.ones_like(res["settled"], dtype=bool)
    assert gone.any() and not gone.all()
    np.testing.assert_array_equal(np.isnan(res["conditional_proba"]), gone)
    np.testing.assert_array_equal(np.isnan(res["conditional_se"]), gone)
    assert (res["settled"][gone] == 0).all()


# ---- 4. chunking and determinism
def test_chunking_and_determinism():
    m, kw, hosts, keys, caps = shape("two_groups")
    rule = dict(legs=(1, 2), **ET)
    inp, call = m._tournament_call(kw["knockout"], kw["groups"], kw["advance"], 0, None, None, hosts, (3, 1, 0), N, 123,
                                   None, "head_to_head", None, "extra_time", rule["legs"], 1 / 3, None, False)
    ctx = m._device()
    extra = dict(key_fixture=keys, key_cap=caps, return_records=True)
    first = ctx.tournament_scenarios(*call["args"], chunk_sims=0, **extra, **call["kwargs"])
    assert set(first) == {"scenario", "joint", "decided_counts", "sim_scenario", "sim_tset"}
    assert first["scenario"].sum() == N and first["decided_counts"].sum() == 3 * N
    for chunk in (0, 1, 64, 100):        # 0 again: two runs are bit-identical
        again = ctx.tournament_scenarios(*call["args"], chunk_sims=chunk, **extra, **call["kwargs"])
        assert set(again) == set(first)
        for k in first:
            np.testing.assert_array_equal(again[k], first[k], err_msg=f"{k} chunk {chunk}")
    bare = ctx.tournament_scenarios(*call["args"], key_fixture=keys, key_cap=caps, **call["kwargs"])
    assert set(bare) == {"scenario", "joint", "decided_counts"}
    for k in bare:
        np.testing.assert_array_equal(bare[k], first[k], err_msg=k)


# ---- 5. the helpers on a device result equal the narrower device calls
def test_marginal_and_coarsen_equal_the_narrower_device_calls():
    m, kw, hosts, keys, caps = shape("two_groups")
    common, _, _ = _call(m, kw, hosts, "overall", {})
    res = m.tournament_scenarios(fixtures=keys, margin_cap=caps, **common)
    for keep in ([1], [2, 0]):
        narrow = m.tournament_scenarios(fixtures=[keys[q] for q in keep], margin_cap=[caps[q] for q in keep], **common)
        got = scenarios.marginal(res, keep)
        assert got["shape"] == narrow["shape"]
        for k in DERIVED:
            np.testing.assert_array_equal(got[k], narrow[k], err_msg=f"{k} keep {keep}")
    for new in (1, [1, 1, 2]):
        coarse = m.tournament_scenarios(fixtures=keys, margin_cap=new, **common)
        got = scenarios.coarsen(res, new)
        assert got["shape"] == coarse["shape"]
        for k in DERIVED:
            np.testing.assert_array_equal(got[k], coarse[k], err_msg=f"{k} caps {new}")
    assert "t00 v t01" in scenarios.format_table(res, "t01", "group_winner")


# ---- 6. errors
def test_context_state_and_argument_errors():
    ctx = HipContext(0)
    try:
        grp = dict(team_idx=[0, 1, 2, 3], team_group=[0, 0, 1, 1], bracket=[0x0001, 0x0101], n_sims=10, key=(0, 1),
                   fix_p=[0, 2], fix_q=[1, 3], advance=1, key_fixture=[1], key_cap=[2])
        with pytest.raises(BplHipError) as e:        # no posterior
            ctx.tournament_scenarios(**grp)
        assert e.value.code == BPLHIP_ESTATE
        S_, T = 4, 8
        ctx.predict_set_posterior(np.zeros((S_, T)), np.zeros((S_, T)), np.zeros(S_), np.zeros(S_))
        with pytest.raises(BplHipError) as e:        # a plain posterior
            ctx.tournament_scenarios(**grp)
        assert e.value.code == BPLHIP_ESTATE
        ctx.predict_set_posterior_venue(*[np.zeros((S_, T)) for _ in range(6)], np.zeros(S_))
        out = ctx.tournament_scenarios(**grp, return_records=True)
        assert out["scenario"].shape == (5,) and out["scenario"].sum() == 10 and out["joint"].shape == (5, 4, 3)
        assert out["joint"][:, :, 0].sum() == 20 and out["joint"][:, :, 2].sum() == 20 and out["sim_tset"].shape == (10, 4)
        ko = dict(team_idx=[0, 1, 2, 3], bracket=[0, 1, 2, 3], n_sims=10, key=(0, 1), key_fixture=[0], key_cap=[1])
        rule = {"legs_mask": 0, "scale": 1 / 3, "away_goals": 0, "strength": None}
        bad = [
            ko,                                              # no groups: nothing to key on
            dict(grp, fix_p=[], fix_q=[]),                   # no group fixtures
            dict(grp, key_fixture=[], key_cap=[]),
            dict(grp, key_fixture=[0] * 9, key_cap=[1] * 9),
            dict(grp, key_fixture=[2]),
            dict(grp, key_fixture=[-1]),
            dict(grp, key_fixture=[1, 1], key_cap=[1, 1]),
            dict(grp, key_cap=[0]),
            dict(grp, key_cap=[4]),
            dict(grp, chunk_sims=-1),
            dict(grp, n_sims=0),
            dict(grp, team_idx=[0, 1, 2, 9]),
            dict(grp, points=(3, -1, 0)),
            dict(grp, knockout=dict(rule, scale=0.0)),
        ]
        for kwargs in bad:
            with pytest.raises(BplHipError) as e:
                ctx.tournament_scenarios(**kwargs)
            assert e.value.code == BPLHIP_EINVAL, kwargs
        # more than 6561 scenarios (5 keys with cap 3), and null required outputs: the entry point itself
        ti, br = np.arange(4, dtype=np.uint16), np.array([0x0001, 0x0101], dtype=np.uint16)
        tg, z = np.array([0, 0, 1, 1], dtype=np.uint8), np.zeros(4, dtype=np.int32)
        fp, fq = np.array([0, 2, 1, 3, 0, 2], dtype=np.uint8), np.array([1, 3, 0, 2, 1, 3], dtype=np.uint8)
        head = [ctx._h, 4, _np_ptr(ti), None, None, 2, _np_ptr(tg), _np_ptr(z), _np_ptr(z), _np_ptr(z), 6, _np_ptr(fp),
                _np_ptr(fq), 1, 0, 2, _np_ptr(br), 3, 1, 0, 10, 0, 1]
        mid = [None, None, 0, 0, 0, 1.0, 0, None, None, 0]   # stream .. chunk_sims
        fn = ctx._lib.bplhip_tournament_scenarios
        kf, kc = np.arange(5, dtype=np.int32), np.full(5, 3, dtype=np.int32)
        sc, jt = np.zeros(7, dtype=np.uint64), np.zeros((7, 4, 3), dtype=np.uint64)
        assert fn(*head, *mid, 5, _np_ptr(kf), _np_ptr(kc), _np_ptr(sc), _np_ptr(jt), None, None) == BPLHIP_EINVAL
        assert fn(*head, *mid, 1, _np_ptr(kf), _np_ptr(kc), None, _np_ptr(jt), None, None) == BPLHIP_EINVAL
        assert fn(*head, *mid, 1, _np_ptr(kf), _np_ptr(kc), _np_ptr(sc), None, None, None) == BPLHIP_EINVAL
        assert fn(*head, *mid, 1, None, _np_ptr(kc), _np_ptr(sc), _np_ptr(jt), None, None) == BPLHIP_EINVAL
        assert not sc.any() and not jt.any()
        assert fn(*head, *mid, 1, _np_ptr(kf), _np_ptr(kc), _np_ptr(sc), _np_ptr(jt), None, None) == 0
        assert sc.sum() == 10 and jt[:, :, 0].sum() == 20
    finally:
        ctx.close()
