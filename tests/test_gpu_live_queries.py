"""match_leverage, points_needed and match_scenarios with `in_play`, `reweight` and `log_weights` on the device
(csrc/dc_live_queries.hip.h) against the live season simulator: under one random_state simulation j of a query IS
simulation j of `simulate_season(in_play=..., return_tables=True, return_scores=True)` -- code from before these
keywords, held to tests/live_ref.py by tests/test_gpu_live.py -- so its per-simulation tables, cross-tabulated by
tests/leverage_ref.py, points_ref.py and scenarios_ref.py, ARE the query's integer tables.  Everything compared is an
integer table or a float the host derives from those integers by one function: every comparison is exact, with no
tolerance and no excluded simulation."""
import functools

import numpy as np
import pytest

import leverage_ref as VR
import live_cases as LC
import points_ref as PR
import scenarios_ref as SR
from bpl import scenarios as _scenarios
from bpl._ffi import BPLHIP_EINVAL, BplHipError
from bpl.base import LEVERAGE_MAX_FIXTURES, _prng_key, leverage_from_counts, points_from_counts
from test_gpu_season import _round_robin

pytestmark = pytest.mark.gpu
TIEBREAKS = ("overall", "head_to_head")
QUERIES = ("leverage", "points", "scenarios")
TARGETS = {"title": (0,), "top_three": (0, 1, 2), "bottom_two": (-1, -2)}
F = len(LC.FIXTURES)
KEYS, CAPS = (2, F + 1, F + 4), (1, 2, 3)        # an ordinary fixture and two matches in play: 3 x 5 x 7 scenarios
LEVELS = (0.5, 0.9)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _season(m, home, away, **kw):
    """The oracle: the live season simulator's per-simulation tables, the scores over the CONCATENATED list."""
    sim = m.simulate_season(home, away, return_tables=True, return_scores=True, **kw)
    hg = np.concatenate([sim["home_goals"], sim.get("in_play_home_goals", sim["home_goals"][:, :0])], axis=1)
    ag = np.concatenate([sim["away_goals"], sim.get("in_play_away_goals", sim["away_goals"][:, :0])], axis=1)
    return sim, hg, ag


def _query(m, which, home, away, keys=KEYS, caps=CAPS, **kw):
    if which == "leverage":
        return m.match_leverage(home, away, targets=TARGETS, **kw)
    if which == "points":
        return m.points_needed(home, away, targets=TARGETS, levels=LEVELS, **kw)
    return m.match_scenarios(home, away, list(keys), targets=TARGETS, margin_cap=list(caps), **kw)


def _check(which, res, sim, hg, ag, n_sims, keys=KEYS, caps=CAPS):
    """Every integer table of `res` is the cross-tabulation of the oracle's simulations, every derived float what the
    host's own function makes of those integers, and ess / log_evidence are the simulator's bit for bit."""
    inside = VR.target_masks(TARGETS, sim["position"].shape[1])
    if which == "leverage":
        ref = dict(zip(("outcome_count", "target_count", "joint_count"), VR.counts(sim["position"], hg, ag, inside)))
        derived = leverage_from_counts(*(ref[k].astype(np.uint64) for k in ref), n_sims)
    elif which == "points":
        pmin, P = int(res["points"][0]), res["points"].size
        names = ("team_points_count", "team_target_count", "position_points_count", "gap_count")
        ref = dict(zip(names, PR.counts(sim["points"], sim["position"], inside, pmin, P)))
        derived = points_from_counts(*(ref[k].astype(np.uint64) for k in names), pmin, n_sims, np.asarray(LEVELS))
    else:
        ref = dict(zip(("scenario_count", "joint_count"), SR.counts(sim["position"], hg, ag, inside, keys, caps)))
        derived = _scenarios.scenario_from_counts(*(ref[k].astype(np.uint64) for k in ref), n_sims)
    for key, want in ref.items():
        assert res[key].dtype == np.int64 and res[key].shape == want.shape, key
        print(f"{which} {key}: {int((res[key] != want).sum())} of {want.size} cells differ, total {int(want.sum())}")
        np.testing.assert_array_equal(res[key], want, err_msg=key)
    for key, want in derived.items():
        np.testing.assert_array_equal(res[key], want, err_msg=key)
    if "ess" in sim:
        assert res["ess"] == sim["ess"], (res["ess"], sim["ess"])
        np.testing.assert_array_equal(res["log_evidence"], sim["log_evidence"])     # (NaN equals NaN here)


@functools.lru_cache(maxsize=None)
def _base(kind, tiebreak, with_log_weights):
    """(model, the live arguments, the oracle) of tests/live_cases.py's shape: T = 6, S = 257, N = 4096, F = 9, its
    six STATES and its TABLE; computed once and shared by the three queries."""
    m = LC.posterior(kind)
    home, away = LC.fixtures(m)
    kw = dict(num_simulations=LC.N, random_state=LC.SEED, current_table=LC.TABLE, tiebreak=tiebreak, in_play=LC.in_play(m),
              log_weights=LC.random_log_weights() if with_log_weights else None)
    return m, home, away, kw, _season(m, home, away, **kw)


# ---- 1. against simulate_season live
@pytest.mark.parametrize("kind", LC.KINDS)
@pytest.mark.parametrize("tiebreak", TIEBREAKS)
@pytest.mark.parametrize("with_log_weights", [False, True])
@pytest.mark.parametrize("which", QUERIES)
def test_against_the_live_season_simulator(which, kind, tiebreak, with_log_weights):
    m, home, away, kw, (sim, hg, ag) = _base(kind, tiebreak, with_log_weights)
    res = _query(m, which, home, away, **kw)
    _check(which, res, sim, hg, ag, LC.N)
    assert np.isfinite(res["ess"]) and res["ess"] < LC.S and np.isfinite(res["log_evidence"])    # weights in force
    if which == "leverage":
        np.testing.assert_array_equal(res["in_play"], np.arange(F, F + len(LC.STATES)))
        assert res["in_play"].dtype == np.int64 and res["outcome_count"].shape == (F + len(LC.STATES), 3)
        # 0-3 after 99.9 % of the match: the away side has won it in (nearly) every simulation
        assert res["outcome_count"][F + 5, 2] >= 0.99 * LC.N
    if which == "scenarios":
        np.testing.assert_array_equal(res["fixtures"], KEYS)
        ip = kw["in_play"]
        assert list(res["home"]) == [home[2], ip["home_team"][1], ip["home_team"][4]]
        assert list(res["away"]) == [away[2], ip["away_team"][1], ip["away_team"][4]]
        # a class that never occurred (the current score has all but ruled it out): count 0, NaN conditionals
        gone = res["scenario_count"] == 0
        assert np.isnan(res["conditional_proba"][gone]).all() and not np.isnan(res["conditional_proba"][~gone]).any()
        # bpl.scenarios' helpers take the result unchanged: match 1 in play alone, at its cap of 2
        alone = _scenarios.marginal(res, [1])
        np.testing.assert_array_equal(alone["fixtures"], [F + 1])
        assert alone["scenario_count"].sum() == LC.N and alone["shape"] == (5,)


# ---- 2. the anchor: 0-0 at elapsed = 0 without re-weighting is the plain call over the 13 fixtures
@pytest.mark.parametrize("tiebreak", TIEBREAKS)
@pytest.mark.parametrize("which", QUERIES)
def test_kick_off_states_are_ordinary_fixtures_table_for_table(which, tiebreak):
    m = LC.posterior("extended")
    home, away = LC.fixtures(m)
    ip = LC.in_play(m, ((0, 0, 0.0),) * 4)
    kw = dict(num_simulations=1000, random_state=77, current_table=LC.TABLE, tiebreak=tiebreak)
    keys = (2, F + 1, F + 3)
    live = _query(m, which, home, away, keys=keys, in_play=ip, reweight=False, **kw)
    plain = _query(m, which, home + ip["home_team"], away + ip["away_team"], keys=keys, **kw)
    for key in plain:
        np.testing.assert_array_equal(live[key], plain[key], err_msg=key)
    extra = {"ess", "log_evidence"} | ({"in_play"} if which == "leverage" else set())
    assert set(live) == set(plain) | extra
    assert live["ess"] == float(LC.S) and np.isnan(live["log_evidence"])     # no weights in force, no likelihood


# ---- 3. the matches in play straddle a block of 64 fixtures
@pytest.mark.parametrize("tiebreak", TIEBREAKS)
@pytest.mark.parametrize("which", ("leverage", "scenarios"))
def test_in_play_fixtures_across_the_block_boundary(which, tiebreak):
    m = LC.posterior("extended")
    h, a = _round_robin(LC.T)
    pairs = tuple(zip(h.tolist(), a.tolist())) * 2                           # the double round robin listed twice
    assert len(pairs) == 60
    home, away = LC.fixtures(m, pairs)
    kw = dict(num_simulations=1024, random_state=5, current_table=LC.TABLE, tiebreak=tiebreak, in_play=LC.in_play(m),
              log_weights=LC.random_log_weights())
    keys, caps = (3, 61, 63, 64, 65), (1, 1, 2, 1, 1)
    sim, hg, ag = _season(m, home, away, **kw)
    res = _query(m, which, home, away, keys=keys, caps=caps, **kw)
    _check(which, res, sim, hg, ag, 1024, keys=keys, caps=caps)
    if which == "leverage":
        np.testing.assert_array_equal(res["in_play"], np.arange(60, 66))
        want = VR.counts(sim["position"], hg, ag, VR.target_masks(TARGETS, LC.T))[0]
        np.testing.assert_array_equal(res["outcome_count"][60:66], want[60:66])
        assert (res["outcome_count"][60:66].sum(axis=1) == 1024).all()


# ---- 4. the resampling step is the call's, whatever the chunk
@pytest.mark.parametrize("which", QUERIES)
def test_chunking_leaves_the_tables_alone(which):
    m = LC.posterior("basic")
    ctx = m._device()
    h, a = m._team_indices(*LC.fixtures(m))
    ipr = m._in_play_inputs(LC.in_play(m))
    masks = [0b000001, 0b000111, 0b110000]
    args = (h, a, np.arange(LC.T), np.zeros((LC.T, 3)), (3, 1, 0), 1000, _prng_key(12), masks)
    live = dict(in_play=ipr, log_weights=LC.random_log_weights())
    runs = []
    for chunk in (64, 333, 0):
        if which == "leverage":
            runs.append(ctx.match_leverage_live(*args, chunk_sims=chunk, **live))
        elif which == "points":
            runs.append(ctx.season_points_live(*args, 0, 3 * 5 + 1, chunk_sims=chunk, **live))
        else:
            runs.append(ctx.season_scenarios_live(*args, KEYS, CAPS, chunk_sims=chunk, **live))
    for other in runs[1:]:
        assert set(other) == set(runs[0])
        for key in runs[0]:
            np.testing.assert_array_equal(other[key], runs[0][key], err_msg=key)
    assert runs[0]["ess"] < LC.S


# ---- 5. log_weights alone: the season updated without a refit
@pytest.mark.parametrize("which", QUERIES)
def test_log_weights_alone(which):
    m = LC.posterior("basic")
    home, away = LC.fixtures(m)
    keys, caps = (0, 4, 8), (1, 2, 1)
    one = np.full(LC.S, -1e4)
    one[100] = 0.0
    for lw in (LC.random_log_weights(), one):
        kw = dict(num_simulations=LC.N, random_state=3, current_table=LC.TABLE, log_weights=lw)
        sim, hg, ag = _season(m, home, away, **kw)
        res = _query(m, which, home, away, keys=keys, caps=caps, **kw)
        _check(which, res, sim, hg, ag, LC.N, keys=keys, caps=caps)
        assert res["log_evidence"] == 0.0                                    # no state, no likelihood
        if which == "leverage":
            assert res["in_play"].shape == (0,) and res["outcome_count"].shape == (F, 3)
    assert (sim["draw"] == 100).all() and res["ess"] == 1.0                   # all the mass on one draw


# ---- 6. extremes: no ordinary fixture at all (and a state at elapsed = 0.999 among LC.STATES)
@pytest.mark.parametrize("tiebreak", TIEBREAKS)
@pytest.mark.parametrize("which", QUERIES)
def test_every_match_in_play(which, tiebreak):
    m = LC.posterior("clipped")
    kw = dict(num_simulations=512, random_state=9, current_table=LC.TABLE, in_play=LC.in_play(m), tiebreak=tiebreak)
    assert LC.STATES[5][2] == 0.999
    keys, caps = (5, 0, 3), (3, 1, 2)
    sim, hg, ag = _season(m, [], [], **kw)
    assert sim["home_goals"].shape == (512, 0) and hg.shape == (512, 6)
    res = _query(m, which, [], [], keys=keys, caps=caps, **kw)
    _check(which, res, sim, hg, ag, 512, keys=keys, caps=caps)
    if which == "leverage":
        np.testing.assert_array_equal(res["in_play"], np.arange(6))


# ---- 7. determinism, and a context that has served a live call
@pytest.mark.parametrize("which", QUERIES)
def test_determinism_and_context_reuse(which):
    m = LC.posterior("extended")
    home, away = LC.fixtures(m)
    kw = dict(num_simulations=3000, random_state=42, current_table=LC.TABLE, tiebreak="head_to_head")
    live = dict(kw, in_play=LC.in_play(m), log_weights=LC.random_log_weights())
    keys, caps = (0, 4, 8), (1, 2, 1)
    r1 = _query(m, which, home, away, **live)
    r2 = _query(m, which, home, away, **live)
    for key in r1:
        np.testing.assert_array_equal(r1[key], r2[key], err_msg=key)
    after = _query(m, which, home, away, keys=keys, caps=caps, **kw)          # the kick-off call on the used context
    fresh = _query(LC.posterior("extended"), which, home, away, keys=keys, caps=caps, **kw)
    assert set(after) == set(fresh) and "ess" not in after
    for key in fresh:
        np.testing.assert_array_equal(after[key], fresh[key], err_msg=key)


# ---- 8. refusals, before the device is touched
@pytest.mark.parametrize("which", QUERIES)
def test_the_library_refuses_malformed_input(which):
    m = LC.posterior("basic")
    ctx = m._device()
    S = LC.S

    def call(ip=((4,), (5,), (1,), (0,), (0.4,)), home=(0,), away=(1,), table_idx=(0, 1, 4, 5), lw=None, keys=(0, 1)):
        n = len(table_idx)
        args = (list(home), list(away), list(table_idx), np.zeros((n, 3)), (3, 1, 0), 10, (0, 1), [1, 3])
        if which == "leverage":
            return ctx.match_leverage_live(*args, in_play=ip, log_weights=lw)["target"][:, 1].sum()
        if which == "points":
            return ctx.season_points_live(*args, 0, 4, in_play=ip, log_weights=lw)["position_points"][:2].sum()
        return ctx.season_scenarios_live(*args, keys, (1, 1), in_play=ip, log_weights=lw)["joint"][:, :, 1].sum()

    assert call() == 20                                                      # two of the four rows are in the top two
    bad = [dict(ip=((4,), (5,), (1,), (0,), (t,))) for t in (float("nan"), 1.0, -0.1, 0.0)]     # 0.0: 1-0 at kick-off
    bad += [dict(ip=((4,), (5,), (64,), (0,), (0.4,))), dict(ip=((4,), (5,), (0,), (64,), (0.4,))),
            dict(ip=((4,), (3,), (1,), (0,), (0.4,))),                   # team 3 is no row of the table
            dict(ip=((4,), (4,), (1,), (0,), (0.4,))),                   # a team playing itself
            dict(ip=((4,), (99,), (1,), (0,), (0.4,))),                  # no such team
            dict(lw=np.full(S, np.inf)), dict(lw=np.where(np.arange(S) == 7, np.nan, 0.0))]
    if which == "scenarios":
        bad.append(dict(keys=(0, 2)))                                    # F + L = 2 is past the concatenated list
    for kw in bad:
        with pytest.raises(BplHipError) as e:
            call(**kw)
        assert e.value.code == BPLHIP_EINVAL, kw
    big = LEVERAGE_MAX_FIXTURES
    with pytest.raises(BplHipError) as e:
        call(home=np.zeros(big, np.uint16), away=np.ones(big, np.uint16))   # F + L one past the bound
    assert e.value.code == BPLHIP_EINVAL
    assert call() == 20                                                      # the context is still good
