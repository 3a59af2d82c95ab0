"""simulate_tournament on the device (csrc/dc_tournament.hip.h) against the numpy restatement
(tests/tournament_ref.py), bit for bit, on the property that per-match sampling cannot give (one
posterior draw per simulated tournament), and on its context and argument errors."""
import numpy as np
import pytest

import tournament_ref as R
from bpl import NeutralDixonColesMatchPredictor, NeutralDixonColesMatchPredictorWC
from bpl._ffi import BPLHIP_EINVAL, BPLHIP_ESTATE, BplHipError, HipContext
from bpl.base import _prng_key
from bpl.neutral_dixon_coles import tournament_result
from test_tournament_host import conf_of, hand_posterior

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _posterior(kind, S=64, seed=0):
    cls = NeutralDixonColesMatchPredictorWC if kind == "wc" else NeutralDixonColesMatchPredictor
    m = hand_posterior(cls, T=64, S=S, seed=seed)
    if kind in ("rho_bounds", "clipped"):
        # every draw's rates over every ordered pair, at a neutral venue and at home
        tabs = R.model_tables(m)
        h, a = np.nonzero(~np.eye(64, dtype=bool))
        s = np.arange(S)[:, None]
        lh = np.concatenate([R.rates(tabs, s, h, a, on)[0] for on in (False, True)], axis=1)
        la = np.concatenate([R.rates(tabs, s, h, a, on)[1] for on in (False, True)], axis=1)
        if kind == "rho_bounds":
            # rho 1e-6 inside its own draw's bound: the lower bound on even draws, the upper on odd
            lo = np.max(np.maximum(-1.0 / lh, -1.0 / la), axis=1)
            hi = np.min(np.minimum(1.0 / (lh * la), 1.0), axis=1)
            m.corr_coef = np.where(np.arange(S) % 2 == 0, lo + 1e-6, hi - 1e-6)
        else:
            m.corr_coef = np.where(np.arange(S) % 2 == 0, 0.9, -1.1)
            rho = m.corr_coef[:, None]
            clipped = (1 - lh * la * rho < 0) | (1 + lh * rho < 0) | (1 + la * rho < 0)
            assert clipped.any() and not clipped.all()
    return m


def _format(fmt, teams):
    if fmt == "wc48":
        return R.world_cup_48(teams, seed=1)
    if fmt == "euro24":
        return R.euro_24(teams, seed=2)
    if fmt == "ko64":
        return R.knockout_64(teams)
    # mid-tournament: a Euro after two of its three group matchdays, the last matchday left
    kw = R.euro_24(teams, seed=3)
    rs = np.random.RandomState(4)
    kw["current_table"] = {t: (int(rs.choice([0, 1, 2, 3, 4, 6])), int(rs.randint(0, 6)), int(rs.randint(0, 6)))
                           for g in kw["groups"].values() for t in g}
    kw["group_fixtures"] = [(g[0], g[3]) for g in kw["groups"].values()] + [(g[2], g[1]) for g in kw["groups"].values()]
    return kw


def _run(m, kw, N, seed, hosts=None, **extra):
    conf = conf_of(m) if isinstance(m, NeutralDixonColesMatchPredictorWC) else None
    res = m.simulate_tournament(num_simulations=N, random_state=seed, hosts=hosts, team_conf=conf, **kw, **extra)
    inp = m._tournament_inputs(kw["knockout"], kw.get("groups"), kw.get("advance", 2), kw.get("best_of_rest", 0),
                               kw.get("group_fixtures"), kw.get("current_table"), hosts, (3, 1, 0), N, conf)
    return res, inp


CASES = [("neutral", "wc48"), ("wc", "wc48"), ("hosts", "euro24"), ("rho_bounds", "mid"), ("clipped", "ko64"),
         ("wc", "ko64"), ("hosts", "mid"), ("neutral", "euro24"), ("wc", "mid"), ("rho_bounds", "wc48")]


@pytest.mark.parametrize("kind,fmt", CASES)
def test_bit_exact_against_restatement(kind, fmt):
    m = _posterior(kind)
    kw = _format(fmt, list(m.teams))
    teams = [t for g in kw["groups"].values() for t in g] if "groups" in kw else kw["knockout"]
    hosts = [teams[1], teams[6], teams[13]] if kind == "hosts" else None
    N, seed = 2000, 4321
    res, inp = _run(m, kw, N, seed, hosts=hosts, return_stages=True)
    ref = R.simulate_tournament(R.model_tables(m), inp, _prng_key(seed))
    assert list(res["teams"]) == teams
    keep = ~ref["flagged"]
    assert ref["flagged"].sum() <= 1e-3 * N, ref["flagged"].sum()
    np.testing.assert_array_equal(res["stage"][keep], ref["stage"][keep])
    if keep.all():
        want = tournament_result(inp, ref)
        for key in ("round_proba", "group_position_proba"):
            if key in want:
                np.testing.assert_array_equal(res[key], want[key], err_msg=key)
    # the aggregates are the returned stages' own
    Rr = inp["rounds"]
    stage = res["stage"].astype(np.int64)
    for r in range(Rr + 1):
        np.testing.assert_array_equal(res["round_proba"][:, r], (stage >= r + 1).sum(axis=0) / N)
        np.testing.assert_array_equal((stage >= r + 1).sum(axis=1), 2 ** (Rr - r))
    if "groups" in kw:
        P = res["group_position_proba"]
        assert P.shape == (len(teams), 4)
        np.testing.assert_allclose(P.sum(axis=1), 1.0, atol=1e-12)


def test_one_posterior_draw_per_tournament():
    # S = 2: t00 is dominant in draw 0 and hopeless in draw 1
    m = _posterior("neutral", S=2, seed=5)
    m.attack[0, 0], m.defence[0, 0], m.attack[1, 0], m.defence[1, 0] = 2.5, 2.5, -2.5, -2.5
    kw = R.world_cup_48(list(m.teams), seed=6)
    N = 20_000
    res, _ = _run(m, kw, N, 77, return_stages=True)
    st = res["stage"][:, 0]
    assert (st[0::2] == 6).mean() >= 0.99, (st[0::2] == 6).mean()
    assert (st[1::2] == 0).mean() >= 0.99, (st[1::2] == 0).mean()


def test_counts_are_the_stages_and_runs_repeat():
    m = _posterior("wc", seed=3)
    kw = R.world_cup_48(list(m.teams), seed=8)
    N = 5000
    r1, _ = _run(m, kw, N, 42, return_stages=True)
    r2, _ = _run(m, kw, N, 42, return_stages=True)
    r3, _ = _run(m, kw, N, 43)
    for key in r1:
        np.testing.assert_array_equal(r1[key], r2[key], err_msg=key)
    assert not np.array_equal(r1["round_proba"], r3["round_proba"])
    # the stages are optional and change nothing else
    r4, _ = _run(m, kw, N, 42)
    assert set(r4) == {"teams", "round_proba", "group_position_proba"}
    for key in r4:
        np.testing.assert_array_equal(r1[key], r4[key], err_msg=key)
    # the device counts are the bincount of the stages
    stage = r1["stage"].astype(np.int64)
    counts = np.stack([np.bincount(stage[:, i], minlength=7) for i in range(48)])
    reached = np.cumsum(counts[:, ::-1], axis=1)[:, ::-1][:, 1:]
    np.testing.assert_array_equal(r1["round_proba"], reached / N)


def test_context_state_and_argument_errors():
    ctx = HipContext(0)
    try:
        ko = dict(team_idx=[0, 1, 2, 3], bracket=[0, 1, 2, 3], n_sims=10, key=(0, 1))
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
        out = ctx.simulate_tournament(**ko)
        assert out["stage_counts"].shape == (4, 4) and out["stage_counts"].sum() == 40
        grp = dict(team_idx=[0, 1, 2, 3], team_group=[0, 0, 1, 1], bracket=[0x0001, 0x0101], n_sims=10,
                   key=(0, 1), fix_p=[0, 2], fix_q=[1, 3], advance=1)
        out = ctx.simulate_tournament(**grp)
        assert out["position_counts"][:, :2].sum() == 40 and out["stage_counts"].sum() == 40
        bad = [
            dict(ko, team_idx=[0, 1, 2, 9]),                 # team out of range
            dict(ko, team_idx=[0, 1, 2, 2]),                 # repeated team
            dict(ko, bracket=[0, 1, 2, 2]),                  # repeated slot
            dict(ko, bracket=[0, 1, 2]),                     # not a power of two
            dict(ko, n_sims=0),
            dict(ko, team_conf=[0, 0, 0, 0]),                # no confederations in this posterior
            dict(ko, team_host=[0, 2, 0, 0]),
            dict(grp, bracket=[0x0001, 0x0102]),             # place 2 does not qualify with advance 1
            dict(grp, bracket=[0x0001, 0x0001]),             # repeated reference
            dict(grp, bracket=[0x0001, 0x0201]),             # no group 2
            dict(grp, bracket=[0x0001, 0xFF01]),             # best_of_rest is 0
            dict(grp, fix_p=[0, 1], fix_q=[1, 2]),           # a fixture across two groups
            dict(grp, fix_p=[0], fix_q=[0]),                 # a team playing itself
            dict(grp, team_group=[0, 0, 0, 1]),              # a group of one
            dict(grp, table=-np.ones((4, 3))),
            dict(grp, points=(3, -1, 0)),
        ]
        for kwargs in bad:
            with pytest.raises(BplHipError) as e:
                ctx.simulate_tournament(**kwargs)
            assert e.value.code == BPLHIP_EINVAL, kwargs
    finally:
        ctx.close()


def test_large_run():
    m = _posterior("wc", S=1000, seed=9)
    kw = R.world_cup_48(list(m.teams))
    N, K = 100_000, 1000
    res, _ = _run(m, kw, N, 31337, return_stages=True)
    assert res["stage"].shape == (N, 48)
    np.testing.assert_allclose(res["round_proba"].sum(axis=0), [32, 16, 8, 4, 2, 1], atol=1e-9)
    _, inp = _run(m, kw, K, 31337)
    ref = R.simulate_tournament(R.model_tables(m), inp, _prng_key(31337))
    keep = ~ref["flagged"]
    np.testing.assert_array_equal(res["stage"][:K][keep], ref["stage"][keep])
