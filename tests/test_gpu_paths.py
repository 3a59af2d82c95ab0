"""tournament_paths on the device (csrc/dc_paths.hip.h): its per-simulation records against the numpy restatement
(tests/paths_ref.py) bit for bit; its identity with simulate_tournament under one random_state, device against
device, in all four modes; its integer tables against the cross-tabulation of its own records; the shape edges; the
independence of the chunk; and the context and argument errors.  Integers only."""
import numpy as np
import pytest

import paths_ref as P
import tournament_ref as R
from bpl import NeutralDixonColesMatchPredictor, NeutralDixonColesMatchPredictorWC
from bpl._ffi import BPLHIP_EINVAL, BPLHIP_ESTATE, BplHipError, HipContext, _np_ptr
from bpl.base import _prng_key
from test_gpu_knockout import case as knockout_case
from test_gpu_tournament import _format, _posterior
from test_tournament_host import conf_of, hand_posterior

pytestmark = pytest.mark.gpu
ET = dict(knockout_rule="extra_time")
SEED = 4321
RECORDS = ("stage", "position", "group_outcome", "pair", "winner", "decided")
TABLES = ("stage_count", "advance_count", "meet_count", "position_stage_count", "outcome_count", "target_count",
          "joint_count")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _args(m, kw, N, hosts, rule):
    conf = conf_of(m) if isinstance(m, NeutralDixonColesMatchPredictorWC) else None
    inp = m._tournament_inputs(kw["knockout"], kw.get("groups"), kw.get("advance", 2), kw.get("best_of_rest", 0),
                               kw.get("group_fixtures"), kw.get("current_table"), hosts, (3, 1, 0), N, conf, **rule)
    return conf, inp


def _run(m, kw, N, seed, hosts=None, tiebreak="overall", records=True, **rule):
    conf, inp = _args(m, kw, N, hosts, rule)
    res = m.tournament_paths(num_simulations=N, random_state=seed, hosts=hosts, team_conf=conf, tiebreak=tiebreak,
                             return_records=records, **kw, **rule)
    return res, inp


def _check_against_restatement(m, kw, N, seed, hosts, tiebreak, rule):
    res, inp = _run(m, kw, N, seed, hosts=hosts, tiebreak=tiebreak, **rule)
    ref = P.simulate(R.model_tables(m), inp, _prng_key(seed), head_to_head=tiebreak == "head_to_head")
    keep = ~ref["flagged"]
    print(f"{ref['flagged'].sum()} of {N} flagged")
    assert ref["flagged"].sum() <= 1e-3 * N, ref["flagged"].sum()
    names = [k for k in RECORDS if k in ref]
    assert names == [k for k in RECORDS if k in res]
    for k in names:
        assert res[k].dtype == np.uint8 and res[k].shape == ref[k].shape, k
        np.testing.assert_array_equal(res[k][keep], ref[k][keep], err_msg=k)
    return res, inp, ref


def _check_tables(res, inp):
    """Every integer table is the cross-tabulation of the returned records, and the invariants hold."""
    N, Rr = inp["num_simulations"], inp["rounds"]
    want = P.counts(res, inp)
    assert [k for k in TABLES if k in want] == [k for k in TABLES if k in res]
    for k, v in want.items():
        assert res[k].dtype == np.int64 and res[k].shape == v.shape, k
        np.testing.assert_array_equal(res[k], v, err_msg=k)
    stage = res["stage"].astype(np.int64)
    reached = (stage[:, :, None] >= np.arange(1, Rr + 2)).sum(axis=0)       # [n, R + 1]
    meet, adv = res["meet_count"], res["advance_count"]
    np.testing.assert_array_equal(meet, adv + adv.transpose(0, 2, 1))
    np.testing.assert_array_equal(meet.sum(axis=2), reached[:, :Rr].T)
    np.testing.assert_array_equal(adv.sum(axis=2), reached[:, 1:].T)
    assert not meet[:, np.arange(meet.shape[1]), np.arange(meet.shape[1])].any()
    np.testing.assert_array_equal(res["round_proba"], reached / N)
    if "position_stage_count" in res:
        ps = res["position_stage_count"]
        np.testing.assert_array_equal(ps.sum(axis=1), res["stage_count"])
        np.testing.assert_array_equal(ps.sum(axis=2) / N, res["group_position_proba"])
    if "joint_count" in res:
        np.testing.assert_array_equal(res["joint_count"].sum(axis=1),
                                      np.broadcast_to(res["target_count"], res["joint_count"].sum(axis=1).shape))
        np.testing.assert_array_equal(res["target_count"], reached)
        np.testing.assert_array_equal(res["outcome_count"].sum(axis=1), N)
    # every knockout match pairs the winners of its two feeder matches
    nb = 1 << Rr
    pair, winner = res["pair"], res["winner"]
    k0 = 0
    for r in range(Rr - 1):
        M = nb >> (r + 1)
        nxt = pair[:, k0 + M:k0 + M + M // 2]
        np.testing.assert_array_equal(nxt[:, :, 0], winner[:, k0:k0 + M:2])
        np.testing.assert_array_equal(nxt[:, :, 1], winner[:, k0 + 1:k0 + M:2])
        k0 += M
    assert ((winner == pair[:, :, 0]) | (winner == pair[:, :, 1])).all()


# ---- 1. records against the restatement
REDRAW = [("neutral", "wc48"), ("hosts", "mid"), ("wc", "ko64"), ("clipped", "ko64"), ("rho_bounds", "wc48"),
          ("wc", "mid")]


@pytest.mark.parametrize("kind,fmt", REDRAW)
def test_records_against_restatement(kind, fmt):
    m = _posterior(kind)
    kw = _format(fmt, list(m.teams))
    teams = [t for g in kw["groups"].values() for t in g] if "groups" in kw else kw["knockout"]
    hosts = [teams[1], teams[6], teams[13]] if kind == "hosts" else None
    res, inp, _ = _check_against_restatement(m, kw, 2000, SEED, hosts, "overall", {})
    assert list(res["teams"]) == teams
    _check_tables(res, inp)


@pytest.mark.parametrize("name,redraw", [("mid_h2h", False), ("mid_h2h", True), ("hosts4", False), ("wc48", False)])
def test_records_against_restatement_other_modes(name, redraw):
    # test_gpu_knockout's cases and seed: head-to-head groups (under either knockout rule), two-legged rounds with
    # away goals, shoot-out strengths
    m, kw, N, hosts, tiebreak, rule = knockout_case(name)
    rule = {} if redraw else dict(rule, **ET)
    res, inp, ref = _check_against_restatement(m, kw, N, SEED, hosts, tiebreak, rule)
    assert ("decided" in res) == (not redraw)
    if name == "hosts4":
        assert (ref["decided"] == 1).any()   # away goals decided some tie
    _check_tables(res, inp)


# ---- 2. identity with simulate_tournament, on all simulations
MODES = [("overall", {}), ("head_to_head", {}), ("overall", dict(legs=(1, 2, 2, 2, 1), away_goals=True, **ET)),
         ("head_to_head", dict(shootout={"t03": 1.5, "t10": -0.5}, **ET))]


@pytest.mark.parametrize("tiebreak,rule", MODES)
def test_identity_with_simulate_tournament(tiebreak, rule):
    m = _posterior("wc", seed=3)
    kw = _format("wc48", list(m.teams))
    N, seed = 3000, 42
    res, _ = _run(m, kw, N, seed, tiebreak=tiebreak, **rule)
    sim = m.simulate_tournament(num_simulations=N, random_state=seed, team_conf=conf_of(m), tiebreak=tiebreak,
                                return_stages=True, **kw, **rule)
    assert ("decided" in sim) == ("knockout_rule" in rule)
    for k in sim:
        assert res[k].dtype == sim[k].dtype, k
        np.testing.assert_array_equal(res[k], sim[k], err_msg=k)
    # the records are optional and change nothing else
    bare, _ = _run(m, kw, N, seed, tiebreak=tiebreak, records=False, **rule)
    assert set(bare) == set(res) - set(RECORDS)
    for k in bare:
        np.testing.assert_array_equal(bare[k], res[k], err_msg=k)


def test_identity_knockout_only_and_hosts():
    m = _posterior("hosts")
    kw = _format("ko64", list(m.teams))
    hosts = [m.teams[1], m.teams[6]]
    for rule in ({}, dict(legs=(2, 2, 1, 1, 1, 1), **ET)):
        res, _ = _run(m, kw, 2000, 7, hosts=hosts, **rule)
        sim = m.simulate_tournament(num_simulations=2000, random_state=7, hosts=hosts, return_stages=True, **kw, **rule)
        for k in sim:
            np.testing.assert_array_equal(res[k], sim[k], err_msg=k)
        assert not set(res) & {"position", "position_stage_count", "round_proba_given_position", "joint_count",
                               "group_position_proba", "fixtures", "leverage"}


# ---- 4. shape edges, on hand posteriors
def _cycled(groups, count):
    """`count` group fixtures: the groups' round robins, gone through again and again."""
    pairs = [(g[i], g[k]) for g in groups.values() for i in range(len(g)) for k in range(i + 1, len(g))]
    return [pairs[i % len(pairs)][::1 if (i // len(pairs)) % 2 == 0 else -1] for i in range(count)]


def _edge(name):
    """(model, simulate_tournament kwargs) of a shape edge."""
    if name.startswith("fixtures"):
        m = hand_posterior(T=20, S=8, seed=11)
        kw = R.group_format(list(m.teams), 4, 4, 0, seed=1)
        kw["group_fixtures"] = _cycled(kw["groups"], int(name[8:]))
        return m, kw
    if name == "8x8":
        m = hand_posterior(T=64, S=12, seed=12)
        return m, R.group_format(list(m.teams), 8, 8, 0, seed=2)
    if name == "ko2":
        m = hand_posterior(T=8, S=9, seed=13)
        return m, {"knockout": ["t05", "t02"]}
    if name == "ko64":
        m = hand_posterior(T=64, S=16, seed=14)
        return m, R.knockout_64(list(m.teams)[::-1])
    if name == "unequal":
        m = hand_posterior(T=20, S=10, seed=15)
        t = list(m.teams)
        groups = {"A": t[0:3], "B": t[3:7], "C": t[7:12], "D": t[12:16]}
        ko = [("A", 1), ("best", 2), ("C", 1), ("best", 4), ("B", 1), ("best", 1), ("D", 1), ("best", 3)]
        return m, {"groups": groups, "advance": 1, "best_of_rest": 4, "knockout": ko}
    if name == "no_fixtures":
        m = hand_posterior(T=12, S=8, seed=16)
        kw = R.group_format(list(m.teams), 2, 4, 0, seed=3)
        rs = np.random.RandomState(5)
        kw["current_table"] = {t: (int(rs.randint(0, 7)), int(rs.randint(0, 5)), int(rs.randint(0, 5)))
                               for g in kw["groups"].values() for t in g}
        kw["group_fixtures"] = []
        return m, kw
    raise KeyError(name)


EDGES = ["fixtures63", "fixtures64", "fixtures65", "8x8", "ko2", "ko64", "unequal", "no_fixtures"]


@pytest.mark.parametrize("name", EDGES)
@pytest.mark.parametrize("rule", [{}, ET], ids=["redraw", "extra_time"])
def test_shape_edges(name, rule):
    m, kw = _edge(name)
    N = 300
    res, inp, _ = _check_against_restatement(m, kw, N, 99, None, "overall", rule)
    _check_tables(res, inp)
    n, Rr, nf = len(inp["teams"]), inp["rounds"], len(inp["fix_p"])
    assert res["stage_count"].shape == (n, Rr + 2) and res["meet_count"].shape == (Rr, n, n)
    assert list(res["targets"]) == [f"round_{r}" for r in range(Rr)] + ["winner"]
    assert ("joint_count" in res) == (nf > 0) and ("position_stage_count" in res) == ("groups" in kw)
    if nf:
        assert res["joint_count"].shape == (nf, 3, n, Rr + 1) and res["leverage"].shape == (nf, n, Rr + 1)
        np.testing.assert_array_equal(res["fixtures"], np.stack([inp["fix_p"], inp["fix_q"]], axis=1))
    sim = m.simulate_tournament(num_simulations=N, random_state=99, return_stages=True, **kw, **rule)
    for k in sim:
        np.testing.assert_array_equal(res[k], sim[k], err_msg=k)


def test_head_to_head_edge_above_the_small_table():
    # 8 groups of 8 under the head-to-head order: the two-wave workgroup of dc_h2h.hip.h
    m, kw = _edge("8x8")
    res, inp, _ = _check_against_restatement(m, kw, 300, 99, None, "head_to_head", {})
    _check_tables(res, inp)


def test_a_host_listed_second_keeps_the_listed_orientation():
    m = hand_posterior(T=8, S=8, seed=17)
    m.attack[:, 3] += 1.0          # t03, the host, listed second in its fixture: about 4.5 goals against 1
    m.home_attack[:, 3] += 0.5
    kw = {"groups": {"A": ["t00", "t03"], "B": ["t05", "t06"]}, "advance": 1, "knockout": [("A", 1), ("B", 1)],
          "group_fixtures": [("t00", "t03"), ("t05", "t06")]}
    N = 300
    res, inp, _ = _check_against_restatement(m, kw, N, 5, ["t03"], "overall", {})
    _check_tables(res, inp)
    np.testing.assert_array_equal(res["fixtures"], [[0, 1], [2, 3]])
    # outcome 2 = the second-listed side, the host at home, wins; t03 then tops the group.  Poisson rates of
    # 4.5 e^(+-0.4) against e^(+-0.4) give the host at least 0.7 and the visitor at most 0.15 of the matches
    assert res["outcome_count"][0, 2] > 2 * res["outcome_count"][0, 0]
    won = res["group_outcome"][:, 0] == 2
    assert (res["position"][won, 1] == 0).all() and (res["position"][res["group_outcome"][:, 0] == 0, 0] == 0).all()
    # without the host the same fixture keeps its orientation and loses the home terms
    res2, _ = _run(m, kw, N, 5)
    assert not np.array_equal(res2["group_outcome"], res["group_outcome"])


# ---- 5. chunking and determinism
@pytest.mark.parametrize("S", [64, 1])
@pytest.mark.parametrize("N", [1, 7, 257, 4097])
def test_chunking_and_determinism(N, S):
    m = _posterior("wc", S=S, seed=2)
    kw = _format("wc48", list(m.teams))
    rule = dict(legs=(1, 2, 1, 1, 1), **ET)
    inp, call = m._tournament_call(kw["knockout"], kw["groups"], kw["advance"], kw["best_of_rest"], None, None, None,
                                   (3, 1, 0), N, 123, conf_of(m), "overall", None, "extra_time", rule["legs"], 1 / 3,
                                   None, False)
    ctx = m._device()
    first = ctx.tournament_paths(*call["args"], return_records=True, chunk_sims=0, **call["kwargs"])
    assert first["stage_counts"].sum() == N * 48 and first["advance"].sum() == N * 31
    for chunk in (0, 64, 100, N):
        again = ctx.tournament_paths(*call["args"], return_records=True, chunk_sims=chunk, **call["kwargs"])
        assert set(again) == set(first)
        for k in first:
            np.testing.assert_array_equal(again[k], first[k], err_msg=f"{k} chunk {chunk}")


# ---- 6. errors
def test_context_state_and_argument_errors():
    ctx = HipContext(0)
    try:
        ko = dict(team_idx=[0, 1, 2, 3], bracket=[0, 1, 2, 3], n_sims=10, key=(0, 1))
        with pytest.raises(BplHipError) as e:        # no posterior
            ctx.tournament_paths(**ko)
        assert e.value.code == BPLHIP_ESTATE
        S, T = 4, 8
        ctx.predict_set_posterior(np.zeros((S, T)), np.zeros((S, T)), np.zeros(S), np.zeros(S))
        with pytest.raises(BplHipError) as e:        # a plain posterior
            ctx.tournament_paths(**ko)
        assert e.value.code == BPLHIP_ESTATE
        ctx.predict_set_posterior_venue(*[np.zeros((S, T)) for _ in range(6)], np.zeros(S))
        out = ctx.tournament_paths(**ko, return_records=True)
        assert out["stage_counts"].sum() == 40 and out["advance"].sum() == 30 and out["pair"].shape == (10, 3, 2)
        grp = dict(team_idx=[0, 1, 2, 3], team_group=[0, 0, 1, 1], bracket=[0x0001, 0x0101], n_sims=10, key=(0, 1),
                   fix_p=[0, 2], fix_q=[1, 3], advance=1)
        out = ctx.tournament_paths(**grp)
        assert out["position_stage"].sum() == 40 and out["outcome"].sum() == 20 and out["advance"].sum() == 10
        rule = {"legs_mask": 0b01, "scale": 1 / 3, "away_goals": 1, "strength": None}
        bad = [
            dict(ko, team_idx=[0, 1, 2, 9]),                 # team out of range
            dict(ko, bracket=[0, 1, 2, 2]),                  # repeated slot
            dict(ko, bracket=[0, 1, 2]),                     # not a power of two
            dict(ko, n_sims=0),
            dict(ko, team_host=[0, 2, 0, 0]),
            dict(ko, chunk_sims=-1),
            dict(ko, knockout=dict(rule, legs_mask=0b100)),
            dict(ko, knockout=dict(rule, scale=0.0)),
            dict(ko, knockout=dict(rule, strength=[0.0, float("nan"), 0.0, 0.0])),
            dict(grp, bracket=[0x0001, 0x0102]),             # place 2 does not qualify with advance 1
            dict(grp, fix_p=[0, 1], fix_q=[1, 2]),           # a fixture across two groups
            dict(grp, team_group=[0, 0, 0, 1]),              # a group of one
            dict(grp, points=(3, -1, 0)),
            dict(grp, chunk_sims=-5),
        ]
        for kwargs in bad:
            with pytest.raises(BplHipError) as e:
                ctx.tournament_paths(**kwargs)
            assert e.value.code == BPLHIP_EINVAL, kwargs
        # null required outputs, which the wrapper never passes: the entry point itself
        ti, br = np.arange(4, dtype=np.uint16), np.arange(4, dtype=np.uint16)
        sc, adv = np.zeros((4, 4), dtype=np.uint64), np.zeros((2, 4, 4), dtype=np.uint64)
        head = [ctx._h, 4, _np_ptr(ti), None, None, 0, None, None, None, None, 0, None, None, 2, 0, 4, _np_ptr(br),
                3, 1, 0, 10, 0, 1]
        mid = [None, None, None, 0, 0, 0, 1.0, 0, None, None, None, 0]   # stream .. chunk_sims
        fn = ctx._lib.bplhip_tournament_paths
        assert fn(*head, _np_ptr(sc), None, *mid, None, *[None] * 8) == BPLHIP_EINVAL
        assert fn(*head, None, None, *mid, _np_ptr(adv), *[None] * 8) == BPLHIP_EINVAL
        assert fn(*head, _np_ptr(sc), None, *mid, _np_ptr(adv), *[None] * 8) == 0
        assert sc.sum() == 40 and adv.sum() == 30
    finally:
        ctx.close()
