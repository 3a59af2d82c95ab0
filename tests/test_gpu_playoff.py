"""simulate_season(..., playoffs=...) on the device (csrc/dc_playoff.hip.h, dc_playoff<*>) against the numpy
restatement (tests/playoff_ref.py), bit for bit; against the call without play-offs, whose every output it must
keep; on the property that one posterior draw drives league and bracket; at limits that need no reference; and on
its counts, repeatability and argument errors."""
import functools

import numpy as np
import pytest

import playoff_ref as PR
from bpl import DixonColesMatchPredictor, ExtendedDixonColesMatchPredictor
from bpl._ffi import BPLHIP_EINVAL, BPLHIP_ESTATE, BplHipError, HipContext, _np_ptr
from bpl.base import PLAYOFF_BYE, PLAYOFF_GUEST, _prng_key, playoff_inputs, playoff_result
from test_gpu_season import _model, _posterior, _rates, _round_robin

pytestmark = pytest.mark.gpu
SEED = 2468
LEAGUE_KEYS = ("teams", "position_proba", "expected_points", "expected_goal_difference", "points", "position",
               "home_goals", "away_goals")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _rounds_left(names, rounds, seed):
    """`rounds` match days among `names` (an even number of them): everybody plays once per day."""
    rs = np.random.RandomState(seed)
    home, away = [], []
    for _ in range(rounds):
        order = rs.permutation(len(names))
        home += [names[i] for i in order[0::2]]
        away += [names[i] for i in order[1::2]]
    return home, away


def _table(names, seed):
    rs = np.random.RandomState(seed)
    return {t: (int(rs.randint(20, 60)), int(rs.randint(20, 70)), int(rs.randint(20, 70))) for t in names}


def _played(names, count, seed):
    rs = np.random.RandomState(seed)
    h = rs.randint(0, len(names), count)
    a = (h + 1 + rs.randint(0, len(names) - 1, count)) % len(names)
    return {"home_team": [names[i] for i in h], "away_team": [names[i] for i in a],
            "home_goals": [int(v) for v in rs.poisson(1.4, count)], "away_goals": [int(v) for v in rs.poisson(1.1, count)]}


def _extended(kind, T=6, S=64, seed=5):
    """Per-team home advantage with rho beyond the bounds (tau clips) or 1e-6 inside either bound."""
    rs = np.random.RandomState(seed)
    m = _model(ExtendedDixonColesMatchPredictor, rs.normal(0, 0.3, (S, T)), rs.normal(0, 0.3, (S, T)),
               rs.normal(0.25, 0.1, (S, T)), np.zeros(S))
    h, a = _round_robin(T)
    lh, la = _rates(m, h, a)
    if kind == "clipped":
        m.corr_coef = np.where(np.arange(S) % 2 == 0, 0.9, -1.1)
        rho = m.corr_coef[:, None]
        clipped = (1 - lh * la * rho < 0) | (1 + lh * rho < 0) | (1 + la * rho < 0)
        assert clipped.any() and not clipped.all()
    else:
        lo = np.max(np.maximum(-1.0 / lh, -1.0 / la), axis=1)
        hi = np.min(np.minimum(1.0 / (lh * la), 1.0), axis=1)
        m.corr_coef = np.where(np.arange(S) % 2 == 0, lo + 1e-6, hi - 1e-6)
    return m


@functools.lru_cache(maxsize=None)
def case(name):
    """(model, simulate_season keywords, N) of a bit-exact case."""
    if name == "championship":
        m = _posterior("basic", T=24)
        names = list(m.teams)
        home, away = _rounds_left(names, 2, 1)
        strengths = {t: float(v) for t, v in zip(names, np.random.RandomState(7).normal(0, 0.5, 24))}
        return m, dict(home_team=home, away_team=away, current_table=_table(names, 2),
                       playoffs={"bracket": [5, 2, 4, 3], "legs": (2, 1), "venue": ("seed", "neutral"),
                                 "shootout": strengths}), 2000
    if name == "relegation":
        m = _posterior("basic", T=19, seed=2)
        names = list(m.teams[:18])
        home, away = _rounds_left(names, 1, 3)
        return m, dict(home_team=home, away_team=away, current_table=_table(names, 4),
                       playoffs={"bracket": [15, "t18"], "legs": 2, "away_goals": True}), 4096
    if name == "league_phase":
        m = _posterior("basic", T=36, seed=3)
        names = list(m.teams)
        home, away = _rounds_left(names, 2, 5)
        bracket = sum(([i, None, 8 + i, 23 - i] for i in range(8)), [])
        return m, dict(home_team=home, away_team=away, played=_played(names, 108, 6), tiebreak="head_to_head",
                       playoffs={"bracket": bracket, "legs": (2, 2, 2, 2, 1), "away_goals": True,
                                 "venue": ("seed", "seed", "seed", "seed", "neutral")}), 2000
    if name in ("extended_clipped", "extended_rho_bounds"):
        m = _extended(name[len("extended_"):])
        names = list(m.teams)
        home, away = _rounds_left(names, 3, 7)
        return m, dict(home_team=home, away_team=away, current_table=_table(names, 8),
                       playoffs={"bracket": [0, 3, 1, 2], "legs": (1, 2), "venue": ("neutral", "seed"),
                                 "away_goals": True}), 4096
    if name == "bracket_64":
        m = _posterior("basic", T=64, seed=4)
        names = list(m.teams)
        home, away = _rounds_left(names, 1, 9)
        bracket = [int(v) for v in np.random.RandomState(10).permutation(64)]
        return m, dict(home_team=home, away_team=away,
                       playoffs={"bracket": bracket, "venue": ("seed", "neutral", "seed", "neutral", "seed", "neutral")}), 2000
    assert name == "identical"
    # no fixtures, an empty table, identical teams: the tie-break word alone seeds the bracket
    T, S = 8, 4
    m = _model(DixonColesMatchPredictor, np.zeros((S, T)), np.zeros((S, T)), np.full(S, 0.3), np.zeros(S))
    return m, dict(home_team=[], away_team=[], teams=list(m.teams),
                   playoffs={"bracket": [0, 7, 3, 4, 1, 6, 2, 5], "legs": (1, 2, 1), "venue": ("seed", "seed", "neutral"),
                             "away_goals": True}), 4096


CASES = ["championship", "relegation", "league_phase", "extended_clipped", "extended_rho_bounds", "bracket_64",
         "identical"]


def _inputs(m, kw, N):
    """What the restatement takes: `_season_h2h_inputs`' results and `playoff_inputs`' dict."""
    h, a, table_idx, table, points, n, h2h, pair = m._season_h2h_inputs(
        kw["home_team"], kw["away_team"], N, kw.get("current_table"), kw.get("teams"), (3, 1, 0),
        kw.get("tiebreak", "overall"), kw.get("played"))
    return (h, a, table_idx, table, points, n), playoff_inputs(kw["playoffs"], table_idx, m._teams_dict), h2h, pair


@functools.lru_cache(maxsize=None)
def reference(name):
    m, kw, N = case(name)
    inputs, po, h2h, pair = _inputs(m, kw, N)
    ref = PR.simulate_season(m, inputs, po, _prng_key(SEED), head_to_head=h2h, pair_init=pair)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref, po


@pytest.mark.parametrize("name", CASES)
def test_bit_exact_against_restatement(name):
    m, kw, N = case(name)
    ref, po = reference(name)
    res = m.simulate_season(num_simulations=N, random_state=SEED, return_tables=True, return_scores=True, **kw)
    keep = ~ref["flagged"]
    print(f"{name}: {ref['flagged'].sum()} of {N} flagged; decided {ref['decided_counts'].tolist()}")
    assert ref["flagged"].sum() <= 1e-3 * N, ref["flagged"].sum()
    R = po["rounds"]
    nt = len(res["teams"]) + len(po["guests"])
    assert list(res["playoff_teams"]) == list(res["teams"]) + po["guest_names"]
    assert res["playoff_stage"].shape == (N, nt) and res["playoff_stage"].dtype == np.uint8
    assert res["playoff_decided"].shape == (N, (1 << R) - 1) and res["playoff_decided"].dtype == np.uint8
    assert res["playoff_round_proba"].shape == (nt, R + 1) and res["playoff_decided_proba"].shape == (R, 4)
    for key in ("home_goals", "away_goals", "points", "position", "playoff_stage", "playoff_decided"):
        np.testing.assert_array_equal(res[key][keep], ref[key][keep], err_msg=key)
    if keep.all():
        want = playoff_result(po, ref, N)
        for key in ("position_proba", "expected_points", "expected_goal_difference"):
            np.testing.assert_array_equal(res[key], ref[key], err_msg=key)
        for key in ("playoff_round_proba", "playoff_decided_proba"):
            np.testing.assert_array_equal(res[key], want[key], err_msg=key)
    # every kind the case can produce is there: the comparison is not of empty columns
    kinds = ref["decided_counts"].sum(axis=0)
    assert kinds[PR.NORMAL] and kinds[PR.IN_EXTRA_TIME] and kinds[PR.BY_SHOOTOUT]
    two_legged_with_away_goals = bool(po["away_goals"]) and bool(po["legs_mask"])
    assert bool(kinds[PR.AWAY_GOALS]) == two_legged_with_away_goals
    byes = bool((po["bracket"] == PLAYOFF_BYE).any())
    assert bool((ref["playoff_decided"] == PR.DECIDED_BYE).any()) == byes


def test_identical_teams_are_seeded_by_the_tie_break_word():
    # the case the word alone decides: the positions are those of the words, and every team gets every seed
    m, kw, N = case("identical")
    ref, _ = reference("identical")
    words = PR.H.words(_prng_key(SEED), N, 8)
    order = np.argsort(-words, axis=1, kind="stable")
    np.testing.assert_array_equal(np.argsort(ref["position"], axis=1), order)
    assert (np.stack([np.bincount(ref["position"][:, i], minlength=8) for i in range(8)]) > 0).all()


@pytest.mark.parametrize("tiebreak", ["overall", "head_to_head"])
def test_league_outputs_are_those_of_the_call_without_playoffs(tiebreak):
    m, kw, N = case("championship")
    kw = dict(kw, tiebreak=tiebreak)
    if tiebreak == "head_to_head":
        kw["played"] = _played(list(m.teams), 60, 11)
    run = dict(num_simulations=N, random_state=77, return_tables=True, return_scores=True)
    with_po = m.simulate_season(**run, **kw)
    without = m.simulate_season(**run, **{k: v for k, v in kw.items() if k != "playoffs"})
    assert set(without) == set(LEAGUE_KEYS)
    assert set(with_po) == set(LEAGUE_KEYS) | {"playoff_teams", "playoff_round_proba", "playoff_decided_proba",
                                               "playoff_stage", "playoff_decided"}
    for key in LEAGUE_KEYS:
        assert with_po[key].dtype == without[key].dtype, key
        np.testing.assert_array_equal(with_po[key], without[key], err_msg=key)
    # and the aggregates alone
    a = m.simulate_season(num_simulations=N, random_state=77, **kw)
    b = m.simulate_season(num_simulations=N, random_state=77, **{k: v for k, v in kw.items() if k != "playoffs"})
    assert set(a) - set(b) == {"playoff_teams", "playoff_round_proba", "playoff_decided_proba"}
    for key in b:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


def test_one_draw_drives_league_and_bracket():
    # two draws.  In draw 0 t06 is far stronger than everybody: it wins its two remaining matches, climbs from 7th
    # into the play-off places and wins the bracket.  In draw 1 it is far weaker: it loses both and stays 7th.
    T, S = 10, 2
    att, dfn = np.zeros((S, T)), np.zeros((S, T))
    att[0, 6], dfn[0, 6] = 3.0, 3.0
    att[1, 6], dfn[1, 6] = -3.0, -3.0
    m = _model(DixonColesMatchPredictor, att, dfn, np.full(S, 0.2), np.zeros(S))
    pts = [80, 75, 60, 58, 56, 54, 51, 40, 10, 5]
    table = {t: (p, 30, 30) for t, p in zip(m.teams, pts)}
    N = 4000
    res = m.simulate_season(["t06", "t09"], ["t08", "t06"], num_simulations=N, random_state=5, current_table=table,
                            return_tables=True, playoffs={"bracket": [5, 2, 4, 3], "legs": (2, 1)})
    pos, stage = res["position"][:, 6].astype(int), res["playoff_stage"][:, 6]
    even, odd = np.arange(N) % 2 == 0, np.arange(N) % 2 == 1
    in_places = (pos >= 2) & (pos <= 5)
    assert (in_places & (stage == 3))[even].mean() >= 0.99
    assert (~in_places & (stage == 0))[odd].mean() >= 0.99
    # the marginal a per-stage resampling of the draws would give is far from both
    assert 0.49 <= res["playoff_round_proba"][6, 2] <= 0.51


def test_limits_that_need_no_reference():
    m = _posterior("basic", T=6)
    names = list(m.teams)
    table = {t: (50 - 5 * i, 0, 0) for i, t in enumerate(names)}     # no fixtures: t00 is 1st, t01 2nd, ...
    N = 4096
    run = dict(home_team=[], away_team=[], num_simulations=N, random_state=5, current_table=table, return_tables=True)
    tiny = {"bracket": [1, 0, 3, 2], "extra_time_scale": 1e-300}
    res = m.simulate_season(**run, playoffs=tiny)
    assert not res["playoff_decided_proba"][:, PR.IN_EXTRA_TIME].any() and res["playoff_decided_proba"][:, PR.BY_SHOOTOUT].all()
    # strengths +20 / -20: exp(-40) ~ 4e-18 is below every uniform's distance from 0 and 1
    for strong, weak in ((0, 1), (1, 0)):
        res = m.simulate_season(**run, playoffs={"bracket": [1, 0], "extra_time_scale": 1e-300,
                                                 "shootout": {names[strong]: 20.0, names[weak]: -20.0}})
        shot = res["playoff_decided"][:, 0] == PR.BY_SHOOTOUT
        assert shot.any() and (res["playoff_stage"][shot, strong] == 2).all() and (res["playoff_stage"][shot, weak] == 1).all()
    # a bye's team is in round 1 in every simulation it is seeded, with or without a league still to play
    h, a = _round_robin(6)
    res = m.simulate_season(h, a, num_simulations=N, random_state=5, return_tables=True,
                            playoffs={"bracket": [0, None, 1, 2], "legs": (2, 1)})
    first = res["position"] == 0
    assert (first.sum(axis=1) == 1).all() and (first.sum(axis=0) > 0).all()
    assert (res["playoff_stage"][first] >= 2).all() and (res["playoff_decided"][:, 0] == PR.DECIDED_BYE).all()
    assert (res["playoff_decided"][:, 1:] <= 3).all()
    np.testing.assert_array_equal(res["playoff_round_proba"][:, 1], (res["playoff_stage"] >= 2).mean(axis=0))
    assert abs(res["playoff_round_proba"][:, 0].sum() - 3) < 1e-9 and abs(res["playoff_round_proba"][:, 1].sum() - 2) < 1e-9


def test_counts_are_the_records_and_runs_repeat():
    m, kw, N = case("league_phase")
    run = dict(num_simulations=N, random_state=42)
    r1 = m.simulate_season(**run, return_tables=True, **kw)
    r2 = m.simulate_season(**run, return_tables=True, **kw)
    for key in r1:
        np.testing.assert_array_equal(r1[key], r2[key], err_msg=key)
    # the per-simulation records are optional and change nothing else
    r3 = m.simulate_season(**run, **kw)
    assert set(r1) - set(r3) == {"points", "position", "playoff_stage", "playoff_decided"}
    for key in r3:
        np.testing.assert_array_equal(r1[key], r3[key], err_msg=key)
    R, nb = 5, 32
    stage = r1["playoff_stage"].astype(np.int64)
    for r in range(R):
        np.testing.assert_array_equal(r1["playoff_round_proba"][:, r], (stage >= r + 1).sum(axis=0) / N)
    np.testing.assert_array_equal(r1["playoff_round_proba"][:, R], (stage == R + 1).sum(axis=0) / N)
    k0 = 0
    for r in range(R):
        M = nb >> (r + 1)
        counts = np.bincount(r1["playoff_decided"][:, k0:k0 + M].ravel(), minlength=256)
        played = N * M - counts[PR.DECIDED_BYE]
        np.testing.assert_array_equal(r1["playoff_decided_proba"][r], counts[:4] / played)
        k0 += M
    np.testing.assert_allclose(r1["playoff_decided_proba"].sum(axis=1), 1.0, atol=1e-12)
    assert abs(r1["playoff_round_proba"][:, 0].sum() - 24) < 1e-9 and abs(r1["playoff_round_proba"][:, R].sum() - 1) < 1e-9


def test_large_run():
    m = _posterior("basic", T=24, S=1000, seed=9)
    h, a = _round_robin(24)
    N = 100_000
    res = m.simulate_season(h, a, num_simulations=N, random_state=31337, return_tables=True,
                            playoffs={"bracket": [5, 2, 4, 3], "legs": (2, 1), "venue": ("seed", "neutral")})
    counts = np.stack([np.bincount(res["playoff_stage"][:, i], minlength=4) for i in range(24)])
    assert counts.sum() == N * 24 and counts[:, 1:].sum() == 4 * N and counts[:, 3].sum() == N
    np.testing.assert_allclose(res["playoff_round_proba"].sum(axis=0), [4, 2, 1], atol=1e-9)
    np.testing.assert_allclose(res["playoff_decided_proba"].sum(axis=1), 1.0, atol=1e-12)
    places = (res["position"] >= 2) & (res["position"] <= 5)
    np.testing.assert_array_equal(res["playoff_stage"] >= 1, places)


def test_context_state_and_argument_errors():
    ctx = HipContext(0)
    try:
        G, B = PLAYOFF_GUEST, PLAYOFF_BYE
        rule = {"guests": [6, 7], "bracket": [0, G | 1, G | 0, 3], "legs_mask": 0b01, "neutral_mask": 0b10,
                "scale": 1 / 3, "away_goals": 1, "strength": [0.5, 0.0, -0.5, 0.0, 0.0, 1.0]}
        season = dict(home_idx=[0, 1], away_idx=[1, 2], table_idx=[0, 1, 2, 3], table=np.zeros((4, 3)), points=(3, 1, 0),
                      n_sims=10, key=(0, 1))
        with pytest.raises(BplHipError) as e:        # no posterior
            ctx.simulate_season(**season, playoff=rule)
        assert e.value.code == BPLHIP_ESTATE
        S, T = 4, 70
        ctx.predict_set_posterior_venue(*[np.zeros((S, T)) for _ in range(6)], np.zeros(S))
        with pytest.raises(BplHipError) as e:        # a venue-form posterior
            ctx.simulate_season(**season, playoff=rule)
        assert e.value.code == BPLHIP_ESTATE
        ctx.predict_set_posterior(np.zeros((S, T)), np.zeros((S, T)), np.zeros(S), np.zeros(S))
        for h2h in (False, True):
            out = ctx.simulate_season(**season, playoff=rule, return_tables=True, head_to_head=h2h)
            assert out["counts"].sum() == 40 and out["stage_counts"].shape == (6, 4) and out["stage_counts"].sum() == 60
            assert out["playoff_stage"].shape == (10, 6) and out["playoff_decided"].shape == (10, 3)
            np.testing.assert_array_equal(out["decided_counts"].sum(axis=1), [20, 10])
        out = ctx.simulate_season(**season, playoff=dict(rule, strength=None, bracket=[0, B, G | 0, 3]))
        np.testing.assert_array_equal(out["decided_counts"].sum(axis=1), [10, 10])
        bad = [
            dict(rule, bracket=[0]),                                  # R = 0
            dict(rule, bracket=list(range(4)) + [B] * 124),           # R = 7
            dict(rule, bracket=[0, G | 1, G | 0, 4]),                 # a position outside the table
            dict(rule, bracket=[0, G | 2, G | 0, 3]),                 # a guest that is not there
            dict(rule, bracket=[0, 0x7FFF, G | 0, 3]),
            dict(rule, bracket=[0, G | 1, G | 0, 0]),                 # a position twice
            dict(rule, bracket=[0, G | 1, G | 1, 3]),                 # a guest twice
            dict(rule, bracket=[0, 1, B, B]),                         # two byes paired
            dict(rule, legs_mask=0b100),                              # a bit at R
            dict(rule, legs_mask=1 << 31),
            dict(rule, neutral_mask=0b100),
            dict(rule, scale=0.0),
            dict(rule, scale=-1.0),
            dict(rule, scale=1.5),
            dict(rule, scale=float("nan")),
            dict(rule, away_goals=2),
            dict(rule, strength=[0.0, float("nan"), 0.0, 0.0, 0.0, 0.0]),
            dict(rule, strength=[0.0, 0.0, float("inf"), 0.0, 0.0, 0.0]),
            dict(rule, strength=[0.0, 0.0, 0.0, 0.0, 0.0, -20.5]),
            dict(rule, guests=[6, 3]),                                # a guest that is a row of the table
            dict(rule, guests=[6, 6]),
            dict(rule, guests=[6, 70]),                               # outside the model
        ]
        for playoff in bad:
            with pytest.raises(BplHipError) as e:
                ctx.simulate_season(**season, playoff=playoff)
            assert e.value.code == BPLHIP_EINVAL, playoff
        # table rows plus guests number at most 64
        wide = dict(season, table_idx=list(range(63)), table=np.zeros((63, 3)))
        ok = ctx.simulate_season(**wide, playoff=dict(rule, guests=[63], bracket=[0, G | 0], legs_mask=0, neutral_mask=0,
                                                      strength=None))
        assert ok["stage_counts"].shape == (64, 3) and ok["stage_counts"].sum() == 640
        with pytest.raises(BplHipError) as e:
            ctx.simulate_season(**wide, playoff=dict(rule, guests=[63, 64], strength=None))
        assert e.value.code == BPLHIP_EINVAL
        with pytest.raises(BplHipError) as e:        # the counterpart's own checks still hold
            ctx.simulate_season(**dict(season, away_idx=[1, 5]), playoff=rule)
        assert e.value.code == BPLHIP_EINVAL
        # null required outputs and a head_to_head flag that is not 0 / 1, which the wrapper never passes
        arr = lambda v, dt: np.ascontiguousarray(v, dtype=dt)   # noqa: E731
        hi, ai, ti = arr([0, 1], np.uint16), arr([1, 2], np.uint16), arr([0, 1, 2, 3], np.uint16)
        zero = [np.zeros(4, dtype=np.int32) for _ in range(3)]
        counts, ps, gs = np.zeros((4, 4), dtype=np.uint64), np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64)
        guests, br = arr([6, 7], np.uint16), arr(rule["bracket"], np.uint16)
        sc, dc = np.zeros((6, 4), dtype=np.uint64), np.zeros((2, 4), dtype=np.uint64)
        head = [ctx._h, 2, _np_ptr(hi), _np_ptr(ai), 4, _np_ptr(ti), *(_np_ptr(z) for z in zero), 3, 1, 0, 10, 0, 1]
        outs = [_np_ptr(counts), _np_ptr(ps), _np_ptr(gs), None, None, None, None, None, None]
        po = [2, _np_ptr(guests), _np_ptr(br), 2, 0b01, 0b10, 1 / 3, 1, None]
        fn = ctx._lib.bplhip_simulate_season_playoff
        assert fn(*head, *outs, 0, *po, None, _np_ptr(dc), None, None) == BPLHIP_EINVAL
        assert fn(*head, *outs, 0, *po, _np_ptr(sc), None, None, None) == BPLHIP_EINVAL
        assert fn(*head, None, *outs[1:], 0, *po, _np_ptr(sc), _np_ptr(dc), None, None) == BPLHIP_EINVAL
        assert fn(*head, *outs, 2, *po, _np_ptr(sc), _np_ptr(dc), None, None) == BPLHIP_EINVAL
        assert fn(*head, *outs, 0, *po[:2], None, *po[3:], _np_ptr(sc), _np_ptr(dc), None, None) == BPLHIP_EINVAL
        assert fn(*head, *outs, 0, 2, None, *po[2:], _np_ptr(sc), _np_ptr(dc), None, None) == BPLHIP_EINVAL
        assert fn(*head, *outs, 0, *po, _np_ptr(sc), _np_ptr(dc), None, None) == 0
        assert counts.sum() == 40 and sc.sum() == 60 and dc.sum() == 30
    finally:
        ctx.close()
