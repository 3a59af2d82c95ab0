"""simulate_tournament(knockout_rule="extra_time") on the device (csrc/dc_knockout.hip.h, dc_tournament_et<*>)
against the numpy restatement (tests/knockout_ref.py), bit for bit; against the redraw rule where the two must
agree; at limits that need no reference; and on its counts, repeatability and argument errors."""
import numpy as np
import pytest

import knockout_ref as K
import tournament_ref as R
from bpl import NeutralDixonColesMatchPredictorWC
from bpl._ffi import BPLHIP_EINVAL, BPLHIP_ESTATE, BplHipError, HipContext, _np_ptr
from bpl.base import _prng_key
from bpl.neutral_dixon_coles import tournament_result
from test_gpu_tournament import _format, _posterior
from test_tournament_host import conf_of

pytestmark = pytest.mark.gpu
ET = dict(knockout_rule="extra_time")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _run(m, kw, N, seed, hosts=None, tiebreak="overall", **rule):
    conf = conf_of(m) if isinstance(m, NeutralDixonColesMatchPredictorWC) else None
    res = m.simulate_tournament(num_simulations=N, random_state=seed, hosts=hosts, team_conf=conf, tiebreak=tiebreak,
                                **kw, **rule)
    inp = m._tournament_inputs(kw["knockout"], kw.get("groups"), kw.get("advance", 2), kw.get("best_of_rest", 0),
                               kw.get("group_fixtures"), kw.get("current_table"), hosts, (3, 1, 0), N, conf,
                               **{k: v for k, v in rule.items() if k != "return_stages"})
    return res, inp


def case(name):
    """(model, format kwargs, N, hosts, tiebreak, rule kwargs) of a bit-exact case."""
    if name == "final":
        m = _posterior("neutral")
        return m, {"knockout": ["t05", "t11"]}, 4096, None, "overall", dict(shootout={"t05": 0.7, "t11": -0.3})
    if name == "hosts4":
        m = _posterior("hosts")
        return (m, {"knockout": ["t02", "t09", "t17", "t30"]}, 2000, ["t09", "t17"], "overall",
                dict(legs=(2, 1), away_goals=True))
    if name == "wc48":
        m = _posterior("wc")
        strengths = {t: float(v) for t, v in zip(m.teams[:48], np.random.RandomState(7).normal(0, 0.5, 48))}
        return m, _format("wc48", list(m.teams)), 2000, None, "overall", dict(shootout=strengths)
    if name == "ko64":
        m = _posterior("rho_bounds")
        return m, _format("ko64", list(m.teams)), 2000, None, "overall", dict(legs=(2, 2, 2, 2, 2, 1))
    m = _posterior("clipped")
    return m, _format("mid", list(m.teams)), 2000, None, "head_to_head", dict(legs=(1, 2, 2, 1))


CASES = ["final", "hosts4", "wc48", "ko64", "mid_h2h"]
SEED = 4321


@pytest.mark.parametrize("name", CASES)
def test_bit_exact_against_restatement(name):
    m, kw, N, hosts, tiebreak, rule = case(name)
    res, inp = _run(m, kw, N, SEED, hosts=hosts, tiebreak=tiebreak, return_stages=True, **ET, **rule)
    ref = K.simulate_tournament(R.model_tables(m), inp, _prng_key(SEED), head_to_head=tiebreak == "head_to_head")
    keep = ~ref["flagged"]
    print(f"{name}: {ref['flagged'].sum()} of {N} flagged; decided {ref['decided_counts'].tolist()}")
    assert ref["flagged"].sum() <= 1e-3 * N, ref["flagged"].sum()
    nm = (1 << inp["rounds"]) - 1
    assert res["stage"].shape == (N, len(inp["teams"])) and res["decided"].shape == (N, nm)
    assert res["decided"].dtype == np.uint8 and res["decided_proba"].shape == (inp["rounds"], 4)
    np.testing.assert_array_equal(res["stage"][keep], ref["stage"][keep])
    np.testing.assert_array_equal(res["decided"][keep], ref["decided"][keep])
    if keep.all():
        want = tournament_result(inp, ref)
        for key in ("round_proba", "group_position_proba", "decided_proba"):
            if key in want:
                np.testing.assert_array_equal(res[key], want[key], err_msg=key)
    # every kind the case can produce is there: the comparison is not of empty columns
    kinds = ref["decided_counts"].sum(axis=0)
    assert kinds[K.NORMAL] and kinds[K.IN_EXTRA_TIME] and kinds[K.BY_SHOOTOUT]
    assert bool(kinds[K.AWAY_GOALS]) == bool(rule.get("away_goals"))


def test_redraw_given_explicitly_is_the_default():
    m = _posterior("wc")
    kw = _format("wc48", list(m.teams))
    r0, _ = _run(m, kw, 3000, 42, return_stages=True)
    r1, _ = _run(m, kw, 3000, 42, return_stages=True, knockout_rule="redraw")
    assert set(r1) == set(r0) == {"teams", "round_proba", "group_position_proba", "stage"}
    for key in r0:
        np.testing.assert_array_equal(r0[key], r1[key], err_msg=key)


def test_decided_in_normal_time_has_the_redraw_winner():
    m = _posterior("hosts")
    N = 4096
    for ko, hosts in ((["t05", "t11"], None), (["t02", "t09", "t17", "t30"], ["t09"])):
        old, _ = _run(m, {"knockout": ko}, N, 99, hosts=hosts, return_stages=True)
        new, _ = _run(m, {"knockout": ko}, N, 99, hosts=hosts, return_stages=True, **ET)
        first = len(ko) // 2                                   # the first round's matches come first
        normal = new["decided"][:, :first] == K.NORMAL
        assert 0.5 < normal.mean() < 0.95
        for k in range(first):
            rows = normal[:, k]
            sides = [2 * k, 2 * k + 1]
            np.testing.assert_array_equal(new["stage"][rows][:, sides] >= 2, old["stage"][rows][:, sides] >= 2)
        # and some level match went the other way than its redraw
        assert ((new["stage"][:, :2] >= 2) != (old["stage"][:, :2] >= 2)).any()


def test_limits_that_need_no_reference():
    m = _posterior("neutral")
    ko = ["t05", "t11", "t20", "t33"]
    N = 4096
    tiny = dict(extra_time_scale=1e-300, return_stages=True, **ET)
    res, _ = _run(m, {"knockout": ko}, N, 5, **tiny)
    assert not res["decided_proba"][:, K.IN_EXTRA_TIME].any() and res["decided_proba"][:, K.BY_SHOOTOUT].all()
    # strengths +20 / -20: exp(-40) ~ 4e-18 is below every uniform's distance from 1
    res, _ = _run(m, {"knockout": ko[:2]}, N, 5, shootout={"t05": -20.0, "t11": 20.0}, **tiny)
    shot = res["decided"][:, 0] == K.BY_SHOOTOUT
    assert shot.any() and (res["stage"][shot, 1] == 2).all() and (res["stage"][shot, 0] == 1).all()
    res, _ = _run(m, {"knockout": ko[:2]}, N, 5, shootout={"t05": 20.0, "t11": -20.0}, **tiny)
    assert (res["stage"][shot, 0] == 2).all()


def test_counts_are_the_records_and_runs_repeat():
    m = _posterior("wc", seed=3)
    kw = _format("wc48", list(m.teams))
    N = 5000
    rule = dict(legs=(1, 2, 2, 2, 1), away_goals=True, **ET)
    r1, inp = _run(m, kw, N, 42, return_stages=True, **rule)
    r2, _ = _run(m, kw, N, 42, return_stages=True, **rule)
    for key in r1:
        np.testing.assert_array_equal(r1[key], r2[key], err_msg=key)
    # the per-simulation records are optional and change nothing else
    r3, _ = _run(m, kw, N, 42, **rule)
    assert set(r3) == {"teams", "round_proba", "group_position_proba", "decided_proba"}
    for key in r3:
        np.testing.assert_array_equal(r1[key], r3[key], err_msg=key)
    k0 = 0
    for r in range(5):
        M = 32 >> (r + 1)
        counts = np.bincount(r1["decided"][:, k0:k0 + M].ravel(), minlength=4)
        np.testing.assert_array_equal(r1["decided_proba"][r], counts / (N * M))
        k0 += M
    np.testing.assert_allclose(r1["decided_proba"].sum(axis=1), 1.0, atol=1e-12)
    assert not r1["decided_proba"][[0, 4], K.AWAY_GOALS].any() and r1["decided_proba"][1:4, K.AWAY_GOALS].all()


def test_large_run():
    m = _posterior("wc", S=1000, seed=9)
    kw = R.world_cup_48(list(m.teams))
    N = 100_000
    res, _ = _run(m, kw, N, 31337, return_stages=True, **ET)
    counts = np.stack([np.bincount(res["stage"][:, i], minlength=7) for i in range(48)])
    assert counts.sum() == N * 48
    np.testing.assert_allclose(res["round_proba"].sum(axis=0), [32, 16, 8, 4, 2, 1], atol=1e-9)
    np.testing.assert_allclose(res["decided_proba"].sum(axis=1), 1.0, atol=1e-12)


def test_context_state_and_argument_errors():
    ctx = HipContext(0)
    try:
        rule = {"legs_mask": 0b01, "scale": 1 / 3, "away_goals": 1, "strength": [0.5, 0.0, -0.5, 0.0]}
        ko = dict(team_idx=[0, 1, 2, 3], bracket=[0, 1, 2, 3], n_sims=10, key=(0, 1), knockout=rule)
        with pytest.raises(BplHipError) as e:        # no posterior
            ctx.simulate_tournament(**ko)
        assert e.value.code == BPLHIP_ESTATE
        S, T = 4, 8
        ctx.predict_set_posterior(np.zeros((S, T)), np.zeros((S, T)), np.zeros(S), np.zeros(S))
        with pytest.raises(BplHipError) as e:        # a plain posterior
            ctx.simulate_tournament(**ko)
        assert e.value.code == BPLHIP_ESTATE
        tabs = [np.zeros((S, T)) for _ in range(6)]
        ctx.predict_set_posterior_venue(*tabs, np.zeros(S))
        out = ctx.simulate_tournament(**ko, return_stages=True)
        assert out["stage_counts"].sum() == 40 and out["decided"].shape == (10, 3)
        np.testing.assert_array_equal(out["decided_counts"].sum(axis=1), [20, 10])
        grp = dict(team_idx=[0, 1, 2, 3], team_group=[0, 0, 1, 1], bracket=[0x0001, 0x0101], n_sims=10, key=(0, 1),
                   fix_p=[0, 2], fix_q=[1, 3], advance=1, knockout=dict(rule, strength=None))
        for h2h in (False, True):
            out = ctx.simulate_tournament(**grp, head_to_head=h2h)
            assert out["position_counts"][:, :2].sum() == 40 and out["decided_counts"].sum() == 10
        bad = [
            dict(rule, legs_mask=0b100),                      # a bit at R
            dict(rule, legs_mask=1 << 31),
            dict(rule, scale=0.0),
            dict(rule, scale=-1.0),
            dict(rule, scale=1.5),
            dict(rule, scale=float("nan")),
            dict(rule, away_goals=2),
            dict(rule, strength=[0.0, float("nan"), 0.0, 0.0]),
            dict(rule, strength=[0.0, 0.0, float("inf"), 0.0]),
            dict(rule, strength=[0.0, 0.0, 0.0, -20.5]),
        ]
        for knockout in bad:
            with pytest.raises(BplHipError) as e:
                ctx.simulate_tournament(**dict(ko, knockout=knockout))
            assert e.value.code == BPLHIP_EINVAL, knockout
        with pytest.raises(BplHipError) as e:        # the counterpart's own checks still hold
            ctx.simulate_tournament(**dict(ko, bracket=[0, 1, 2, 2]))
        assert e.value.code == BPLHIP_EINVAL
        # a null decided_counts, which the wrapper never passes: the entry point itself
        ti, br = np.arange(4, dtype=np.uint16), np.arange(4, dtype=np.uint16)
        sc, dc = np.zeros((4, 4), dtype=np.uint64), np.zeros((2, 4), dtype=np.uint64)
        head = [ctx._h, 4, _np_ptr(ti), None, None, 0, None, None, None, None, 0, None, None, 2, 0, 4, _np_ptr(br), 3, 1,
                0, 10, 0, 1]
        rule_args = [None, 0, 0b01, 1 / 3, 1, None]
        fn = ctx._lib.bplhip_simulate_tournament_knockout
        assert fn(*head, _np_ptr(sc), None, None, None, *rule_args, None, None) == BPLHIP_EINVAL
        assert fn(*head, None, None, None, None, *rule_args, _np_ptr(dc), None) == BPLHIP_EINVAL
        assert fn(*head, _np_ptr(sc), None, None, None, *rule_args, _np_ptr(dc), None) == 0
        assert sc.sum() == 40 and dc.sum() == 30
    finally:
        ctx.close()
