"""The head-to-head kernels on the device (csrc/dc_h2h.hip.h) against the numpy restatement of the rule
(tests/h2h_ref.py).  The season checks restate no sampling: the device's own scorelines, bit-identical to the
overall mode's, are ranked in numpy, so EVERY simulation is compared.  Every comparison is of integers."""
import numpy as np
import pytest

import h2h_ref as H
import leverage_ref as L
import tournament_ref as R
from bpl import (DixonColesMatchPredictor, ExtendedDixonColesMatchPredictor, NeutralDixonColesMatchPredictor,
                 NeutralDixonColesMatchPredictorWC)
from bpl._ffi import BPLHIP_EINVAL, BPLHIP_ESTATE, BplHipError, HipContext, prng_key
from bpl.base import LEVERAGE_TARGETS, leverage_targets
from bpl.neutral_dixon_coles import tournament_result
from test_h2h_host import HAND_CASES, _played, hand_case
from test_tournament_host import conf_of, hand_posterior

pytestmark = pytest.mark.gpu
POINTS = (3, 1, 0)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _posterior(per_team, T, S, seed):
    """S hand-built draws, with (the extended class) or without per-team home advantage."""
    rs = np.random.RandomState(seed)
    m = (ExtendedDixonColesMatchPredictor if per_team else DixonColesMatchPredictor)()
    m.teams = np.array([f"t{i:02d}" for i in range(T)])
    m._teams_dict = {t: i for i, t in enumerate(m.teams)}
    m.attack, m.defence = rs.normal(0, 0.3, (S, T)), rs.normal(0, 0.3, (S, T))
    m.home_advantage = rs.normal(0.25, 0.1, (S, T)) if per_team else rs.normal(0.25, 0.05, S)
    m.corr_coef = rs.uniform(-0.1, 0.1, S)
    return m


def _round_robin(T):
    h, a = np.nonzero(~np.eye(T, dtype=bool))
    return h, a


def _pairings(T, F, seed):
    rs = np.random.RandomState(seed)
    h = rs.randint(0, T, F)
    return h, (h + rs.randint(1, T, F)) % T


def _half_season(T, seed):
    """A single round robin already played (slots = model indices here): (home, away, x, y)."""
    rs = np.random.RandomState(seed)
    h, a = np.nonzero(np.triu(np.ones((T, T), dtype=bool), 1))
    swap = rs.rand(h.size) < 0.5
    h, a = np.where(swap, a, h), np.where(swap, h, a)
    return h, a, rs.poisson(1.4, h.size), rs.poisson(1.1, h.size)


def _season(m, h, a, N, seed, played=None):
    """Both modes under one key, the checks every shape shares, and the restated positions."""
    T = len(m.teams)
    kw = dict(num_simulations=N, random_state=seed, return_tables=True, return_scores=True, teams=list(m.teams))
    names = None
    if played is not None:
        names = {"home_team": list(m.teams[played[0]]), "away_team": list(m.teams[played[1]]),
                 "home_goals": [int(v) for v in played[2]], "away_goals": [int(v) for v in played[3]]}
    res = m.simulate_season(h, a, tiebreak="head_to_head", played=names, **kw)
    ovr = m.simulate_season(h, a, tiebreak="overall", played=names, **kw)
    assert list(res["teams"]) == list(m.teams)
    for key in ("home_goals", "away_goals", "points"):
        np.testing.assert_array_equal(res[key], ovr[key], err_msg=key)
    # the reference: the table and the pair records of `played`, restated here, then the device's own scorelines
    table = np.zeros((T, 3), dtype=np.int64)
    pair_init = None
    if played is not None:
        ph, pa, px, py = (np.asarray(v, np.int64) for v in played)
        _, pts0 = H.season_positions(ph, pa, px[None], py[None], table, POINTS, (0, 0))
        table[:, 0] = pts0[0]
        for col, v in ((1, (px, py)), (2, (py, px))):
            np.add.at(table[:, col], ph, v[0])
            np.add.at(table[:, col], pa, v[1])
        pair_init = H.pair_from_scores(ph, pa, px[None], py[None], POINTS, T)[0]
    pos, pts = H.season_positions(h, a, res["home_goals"], res["away_goals"], table, POINTS, prng_key(seed), pair_init)
    np.testing.assert_array_equal(res["points"], pts)
    np.testing.assert_array_equal(res["position"], pos)                 # every simulation
    counts = np.zeros((T, T), dtype=np.int64)
    np.add.at(counts, (np.broadcast_to(np.arange(T), (N, T)), res["position"].astype(np.int64)), 1)
    np.testing.assert_array_equal(res["position_proba"], counts / N)
    np.testing.assert_array_equal(res["expected_points"], ovr["expected_points"])
    np.testing.assert_array_equal(res["expected_goal_difference"], ovr["expected_goal_difference"])
    assert (np.sort(res["position"], axis=1) == np.arange(T)).all()
    return res, ovr, table, pair_init


# ---------------------------------------------------------------- 1. exact, without any restated sampling
# (n, fixtures, N, draws): a small double round robin; more simulations than the grid has waves (a wave plays
# several: the matrix reset); the row pitch, the last lane and the second fixture pass at 63 / 64 slots
SHAPES = {"4x12": (4, 12, 2000, 3), "6x30": (6, 30, 20_000, 16), "63x65": (63, 65, 500, 8), "64x128": (64, 128, 500, 64)}


@pytest.mark.parametrize("per_team", [False, True])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_positions_are_the_rule_on_the_devices_own_scorelines(shape, per_team):
    n, F, N, S = SHAPES[shape]
    m = _posterior(per_team, n, S, seed=n + F)
    h, a = _round_robin(n) if F == n * (n - 1) else _pairings(n, F, seed=F)
    assert h.size == F
    res, ovr, _, _ = _season(m, h, a, N, seed=100 + n)
    assert (res["position"] != ovr["position"]).any()


@pytest.fixture(scope="module")
def mid_season():
    """20 teams, 380 fixtures to come, a single round robin played: shared with the leverage test."""
    m = _posterior(False, 20, 64, seed=20)
    h, a = _round_robin(20)
    played = _half_season(20, seed=5)
    N, seed = 2000, 777
    res, ovr, table, pair_init = _season(m, h, a, N, seed, played)
    return dict(m=m, h=h, a=a, played=played, N=N, seed=seed, res=res, ovr=ovr, table=table, pair_init=pair_init)


def test_mid_season_pair_records(mid_season):
    res, ovr = mid_season["res"], mid_season["ovr"]
    assert (res["position"] != ovr["position"]).any()
    assert mid_season["pair_init"].max() > 0


def test_mid_season_with_per_team_home_advantage():
    m = _posterior(True, 20, 33, seed=21)
    h, a = _round_robin(20)
    res, ovr, _, _ = _season(m, h, a, 2000, 778, _half_season(20, seed=6))
    assert (res["position"] != ovr["position"]).any()


@pytest.mark.parametrize("per_team", [False, True])
def test_smallest_tables(per_team):
    """A single-slot table and the smallest table with a match.  Neither can differ from the overall order (two
    teams level on points have drawn their only match), so only the identities are checked."""
    m = _posterior(per_team, 1, 3, seed=1)
    res, _, _, _ = _season(m, np.zeros(0, int), np.zeros(0, int), 300, seed=1)
    assert (res["position"] == 0).all() and res["position_proba"].tolist() == [[1.0]]
    m = _posterior(per_team, 2, 5, seed=2)
    res, ovr, _, _ = _season(m, np.array([1]), np.array([0]), 300, seed=2)
    np.testing.assert_array_equal(res["position"], ovr["position"])
    assert 0 < res["position_proba"][0, 0] < 1


# ---------------------------------------------------------------- 2. nothing to simulate: the hand-built tables
@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_hand_built_tables_on_the_device(name):
    played, teams, order = hand_case(name)
    m = _posterior(False, 6, 4, seed=3)
    N = 2000
    res = m.simulate_season([], [], num_simulations=N, random_state=9, played=played, tiebreak="head_to_head",
                            return_tables=True)
    assert list(res["teams"]) == teams
    pos = res["position"].astype(np.int64)
    if order is not None:
        want = [order.index(t) for t in teams]
        np.testing.assert_array_equal(pos, np.broadcast_to(want, pos.shape))
    else:
        # t00 and t01 are level on all six keys: a fair coin from the tie-break word, 40-60 % is more than 4 sigma
        # on each side at N = 2000 (sigma = 1.1 %); t02 is last in every simulation
        assert (pos[:, 2] == 2).all() and (pos[:, 0] + pos[:, 1] == 1).all()
        first = (pos[:, 0] == 0).mean()
        assert 0.4 <= first <= 0.6, first


# ---------------------------------------------------------------- 3. leverage
def test_leverage_counts_are_the_cross_tabulation_of_the_season(mid_season):
    c = mid_season
    m, N = c["m"], c["N"]
    ph, pa, px, py = c["played"]
    names = {"home_team": list(m.teams[ph]), "away_team": list(m.teams[pa]),
             "home_goals": [int(v) for v in px], "away_goals": [int(v) for v in py]}
    res = m.match_leverage(c["h"], c["a"], num_simulations=N, random_state=c["seed"], teams=list(m.teams),
                           tiebreak="head_to_head", played=names)
    inside = L.target_masks(LEVERAGE_TARGETS, 20)
    outcome, target, joint = L.counts(c["res"]["position"], c["res"]["home_goals"], c["res"]["away_goals"], inside)
    np.testing.assert_array_equal(res["target_count"], target)
    np.testing.assert_array_equal(res["joint_count"], joint)
    np.testing.assert_array_equal(res["outcome_count"], outcome)
    # ... and not the overall order's
    _, t_ovr, _ = L.counts(c["ovr"]["position"], c["ovr"]["home_goals"], c["ovr"]["away_goals"], inside)
    assert not np.array_equal(target, t_ovr)
    # identical for every chunking
    _, masks = leverage_targets(None, 20)
    for chunk in (64, 1000, 0):
        raw = m._device().match_leverage(c["h"], c["a"], np.arange(20), c["table"], POINTS, N, prng_key(c["seed"]), masks,
                                         chunk_sims=chunk, pair_init=c["pair_init"], head_to_head=True)
        np.testing.assert_array_equal(raw["target"].astype(np.int64), target, err_msg=str(chunk))
        np.testing.assert_array_equal(raw["joint"].astype(np.int64), joint, err_msg=str(chunk))
        np.testing.assert_array_equal(raw["outcome"].astype(np.int64), outcome, err_msg=str(chunk))


def test_leverage_counts_in_two_wave_workgroups():
    """Above 48 slots a head-to-head workgroup has two waves: 50 slots, and a ragged last chunk (200, 200, 112)."""
    n, F, N, seed = 50, 64, 512, 150
    m = _posterior(False, n, 8, seed=n + F)
    h, a = _pairings(n, F, seed=F)
    res, _, table, _ = _season(m, h, a, N, seed)
    outcome, target, joint = L.counts(res["position"], res["home_goals"], res["away_goals"], L.target_masks(LEVERAGE_TARGETS, n))
    _, masks = leverage_targets(None, n)
    raw = m._device().match_leverage(h, a, np.arange(n), table, POINTS, N, prng_key(seed), masks, chunk_sims=200,
                                     head_to_head=True)
    np.testing.assert_array_equal(raw["target"].astype(np.int64), target)
    np.testing.assert_array_equal(raw["joint"].astype(np.int64), joint)
    np.testing.assert_array_equal(raw["outcome"].astype(np.int64), outcome)


# ---------------------------------------------------------------- 4. tournament
def _neutral(kind, S=16, seed=0):
    cls = NeutralDixonColesMatchPredictorWC if kind == "wc" else NeutralDixonColesMatchPredictor
    return hand_posterior(cls, T=64, S=S, seed=seed)


def _format(fmt, teams):
    """(simulate_tournament kwargs, `played` as (home, away, x, y) names / goals or None)."""
    if fmt == "wc48":
        return R.world_cup_48(teams, seed=1), None
    if fmt == "euro24":
        return R.euro_24(teams, seed=2), None
    # mid-tournament: a Euro after two of its three group matchdays, the last matchday left
    kw = R.euro_24(teams, seed=3)
    groups = list(kw["groups"].values())
    kw["group_fixtures"] = [(g[0], g[3]) for g in groups] + [(g[2], g[1]) for g in groups]
    done = [(g[0], g[1]) for g in groups] + [(g[2], g[3]) for g in groups] + \
           [(g[0], g[2]) for g in groups] + [(g[3], g[1]) for g in groups]
    rs = np.random.RandomState(4)
    return kw, [(p, q, int(rs.poisson(1.3)), int(rs.poisson(1.1))) for p, q in done]


def _tournament(m, kw, N, seed, hosts, played, tiebreak="head_to_head"):
    conf = conf_of(m) if isinstance(m, NeutralDixonColesMatchPredictorWC) else None
    res = m.simulate_tournament(num_simulations=N, random_state=seed, hosts=hosts, team_conf=conf, return_stages=True,
                                tiebreak=tiebreak, played=None if played is None else _played(played), **kw)
    inp = m._tournament_inputs(kw["knockout"], kw.get("groups"), kw.get("advance", 2), kw.get("best_of_rest", 0),
                               kw.get("group_fixtures"), None, hosts, POINTS, N, conf)
    pair_init = None
    if played is not None:
        # the table and the pair records of `played`, restated here
        slot = {t: i for i, t in enumerate(inp["teams"])}
        n = len(slot)
        ph, pa = np.array([slot[p[0]] for p in played]), np.array([slot[p[1]] for p in played])
        px, py = np.array([p[2] for p in played]), np.array([p[3] for p in played])
        table = np.zeros((n, 3), dtype=np.int64)
        _, pts0 = H.season_positions(ph, pa, px[None], py[None], table, POINTS, (0, 0))
        table[:, 0] = pts0[0]
        for col, v in ((1, (px, py)), (2, (py, px))):
            np.add.at(table[:, col], ph, v[0])
            np.add.at(table[:, col], pa, v[1])
        inp["table"] = table
        pair_init = H.pair_from_scores(ph, pa, px[None], py[None], POINTS, n)[0]
    return res, inp, pair_init


CASES = [("neutral", "wc48"), ("wc", "wc48"), ("hosts", "euro24"), ("wc", "euro24"), ("neutral", "mid"),
         ("hosts", "mid"), ("wc", "mid")]


@pytest.mark.parametrize("kind,fmt", CASES)
def test_tournament_against_the_restatement(kind, fmt):
    m = _neutral(kind)
    kw, played = _format(fmt, list(m.teams))
    teams = [t for g in kw["groups"].values() for t in g]
    hosts = [teams[1], teams[6], teams[13]] if kind == "hosts" else None
    N, seed = 2000, 4321
    res, inp, pair_init = _tournament(m, kw, N, seed, hosts, played)
    ref = H.simulate_tournament(R.model_tables(m), inp, prng_key(seed), pair_init)
    keep = ~ref["flagged"]
    assert ref["flagged"].sum() <= 1e-3 * N, ref["flagged"].sum()
    np.testing.assert_array_equal(res["stage"][keep], ref["stage"][keep])
    if keep.all():
        want = tournament_result(inp, ref)
        for key in ("round_proba", "group_position_proba"):
            np.testing.assert_array_equal(res[key], want[key], err_msg=key)
    np.testing.assert_allclose(res["group_position_proba"].sum(axis=1), 1.0, atol=1e-12)
    if fmt == "wc48":
        ovr, _, _ = _tournament(m, kw, N, seed, hosts, played, tiebreak="overall")
        assert not np.array_equal(res["group_position_proba"], ovr["group_position_proba"])


def test_tournament_in_two_wave_workgroups():
    """Above 48 slots a head-to-head workgroup has two waves: 64 slots in 16 groups of 4, a single round robin per
    group (96 fixtures, a second fixture pass), the top two into a bracket of 32."""
    m = _neutral("wc")
    kw = R.group_format(list(m.teams), 16, 4, 0, seed=5)
    N, seed = 300, 4322
    res, inp, pair_init = _tournament(m, kw, N, seed, None, None)
    assert len(inp["team_idx"]) == 64 and len(inp["fix_p"]) == 96 and len(inp["bracket"]) == 32
    ref = H.simulate_tournament(R.model_tables(m), inp, prng_key(seed), pair_init)
    assert not ref["flagged"].any(), ref["flagged"].sum()
    np.testing.assert_array_equal(res["stage"], ref["stage"])                # every simulation
    want = tournament_result(inp, ref)
    for key in ("round_proba", "group_position_proba"):
        np.testing.assert_array_equal(res[key], want[key], err_msg=key)


def test_best_of_the_rest_keeps_the_overall_keys():
    """Three groups of three, the top two and the two best thirds go through, nothing left to play.  The thirds of
    A and B are level on one point, and each is level on points with a team of its own group, so both carry
    head-to-head keys: t02 took a point and no goal from t01, t05 a point and two goals from t04.  Across groups
    those keys mean nothing: on overall goal difference t02 (-2) is ahead of t05 (-3) and takes the last place;
    ranked by the head-to-head keys t05 (two goals) would.  Group C is level throughout, its third has two points."""
    m = _neutral("neutral", S=4)
    t = list(m.teams[:9])
    groups = {"A": t[0:3], "B": t[3:6], "C": t[6:9]}
    played = [(t[0], t[1], 1, 0), (t[0], t[2], 2, 0), (t[1], t[2], 0, 0),
              (t[3], t[4], 1, 0), (t[3], t[5], 3, 0), (t[4], t[5], 2, 2),
              (t[6], t[7], 1, 1), (t[6], t[8], 1, 1), (t[7], t[8], 1, 1)]
    ko = [("A", 1), ("best", 2), ("B", 1), ("C", 2), ("C", 1), ("B", 2), ("A", 2), ("best", 1)]
    N = 500
    for tiebreak in ("head_to_head", "overall"):
        res = m.simulate_tournament(ko, groups, advance=2, best_of_rest=2, group_fixtures=[], played=_played(played),
                                    num_simulations=N, random_state=3, return_stages=True, tiebreak=tiebreak)
        stage = res["stage"]
        assert (stage[:, 2] >= 1).all() and (stage[:, 5] == 0).all(), tiebreak
        assert (stage[:, [0, 1, 3, 4]] >= 1).all() and ((stage[:, 6:9] >= 1).sum(axis=1) == 3).all()
        np.testing.assert_array_equal(res["group_position_proba"][:6], np.eye(3)[[0, 1, 2, 0, 1, 2]])


# ---------------------------------------------------------------- 5. repeats and errors
def test_runs_repeat_bit_for_bit():
    m = _posterior(True, 20, 16, seed=30)
    h, a = _round_robin(20)
    kw = dict(num_simulations=3000, random_state=42, tiebreak="head_to_head", return_tables=True, return_scores=True)
    r1, r2 = m.simulate_season(h, a, **kw), m.simulate_season(h, a, **kw)
    for key in r1:
        np.testing.assert_array_equal(r1[key], r2[key], err_msg=key)
    l1 = m.match_leverage(h, a, num_simulations=3000, random_state=42, tiebreak="head_to_head")
    l2 = m.match_leverage(h, a, num_simulations=3000, random_state=42, tiebreak="head_to_head")
    for key in ("outcome_count", "target_count", "joint_count"):
        np.testing.assert_array_equal(l1[key], l2[key], err_msg=key)
    nm = _neutral("wc")
    fmt = R.world_cup_48(list(nm.teams), seed=8)
    t1, _, _ = _tournament(nm, fmt, 3000, 42, None, None)
    t2, _, _ = _tournament(nm, fmt, 3000, 42, None, None)
    for key in t1:
        np.testing.assert_array_equal(t1[key], t2[key], err_msg=key)


def test_context_state_and_argument_errors():
    ctx = HipContext(0)
    try:
        season = ([0], [1], [0, 1], np.zeros((2, 3)), POINTS, 10, (0, 1))
        ko = dict(team_idx=[0, 1, 2, 3], team_group=[0, 0, 1, 1], bracket=[0x0001, 0x0101], n_sims=10, key=(0, 1),
                  fix_p=[0, 2], fix_q=[1, 3], advance=1, head_to_head=True)
        for call in (lambda: ctx.simulate_season(*season, head_to_head=True),
                     lambda: ctx.match_leverage(*season, [1], head_to_head=True),
                     lambda: ctx.simulate_tournament(**ko)):
            with pytest.raises(BplHipError) as e:        # no posterior
                call()
            assert e.value.code == BPLHIP_ESTATE
        S, T = 4, 8
        ctx.predict_set_posterior(np.zeros((S, T)), np.zeros((S, T)), np.zeros(S), np.zeros(S))
        with pytest.raises(BplHipError) as e:            # a plain posterior
            ctx.simulate_tournament(**ko)
        assert e.value.code == BPLHIP_ESTATE
        out = ctx.simulate_season(*season, head_to_head=True)
        assert out["counts"].sum() == 20
        out = ctx.match_leverage(*season, [1], head_to_head=True, pair_init=np.zeros((2, 2)))
        assert out["target"].sum() == 10
        full = np.array([[0, 0xFFFF << 16], [0, 0]], dtype=np.uint32)      # 65535 points, one meeting to come
        goals = np.array([[0, 0], [65281, 0]], dtype=np.uint32)           # 65281 + 255 goals
        for bad in (full, goals):
            for call in (lambda: ctx.simulate_season(*season, head_to_head=True, pair_init=bad),
                         lambda: ctx.match_leverage(*season, [1], head_to_head=True, pair_init=bad)):
                with pytest.raises(BplHipError) as e:
                    call()
                assert e.value.code == BPLHIP_EINVAL
        ok = np.array([[7, 65280], [65535 - 3 << 16, 9]], dtype=np.uint32)  # at the bound; the diagonal is ignored
        assert ctx.simulate_season(*season, head_to_head=True, pair_init=ok)["counts"].sum() == 20
        with pytest.raises(BplHipError) as e:            # the counterpart's own argument errors
            ctx.simulate_season([0], [0], [0, 1], np.zeros((2, 3)), POINTS, 10, (0, 1), head_to_head=True)
        assert e.value.code == BPLHIP_EINVAL
        with pytest.raises(ValueError):
            ctx.simulate_season(*season, head_to_head=True, pair_init=np.zeros((3, 3)))
        tabs = [np.zeros((S, T)) for _ in range(6)]
        ctx.predict_set_posterior_venue(*tabs, np.zeros(S))
        with pytest.raises(BplHipError) as e:            # a venue-form posterior
            ctx.simulate_season(*season, head_to_head=True)
        assert e.value.code == BPLHIP_ESTATE
        out = ctx.simulate_tournament(**ko)
        assert out["position_counts"][:, :2].sum() == 40 and out["stage_counts"].sum() == 40
        bad = np.zeros((4, 4), dtype=np.uint32)
        bad[2, 3] = 0xFFFF
        with pytest.raises(BplHipError) as e:
            ctx.simulate_tournament(**ko, pair_init=bad)
        assert e.value.code == BPLHIP_EINVAL
        with pytest.raises(BplHipError) as e:            # a fixture across two groups
            ctx.simulate_tournament(**dict(ko, fix_p=[0, 1], fix_q=[1, 2]))
        assert e.value.code == BPLHIP_EINVAL
    finally:
        ctx.close()
    m = _posterior(False, 4, 3, seed=1)
    with pytest.raises(ValueError):
        m.simulate_season([0], [1], num_simulations=10, tiebreak="nope")
