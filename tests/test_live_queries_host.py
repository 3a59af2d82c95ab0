"""match_leverage, points_needed and match_scenarios with `in_play`, `reweight` and `log_weights` without a GPU: the
result's keys, shapes and dtypes through a stand-in context, key fixtures on the concatenated list, the points axis
over the matches in play, every argument check (all made on the host before a context is touched), and the defaults:
the kick-off entry point and the key set of before."""
import numpy as np
import pytest

from bpl.base import LEVERAGE_MAX_FIXTURES
from test_playoff_host import hand_posterior

QUERIES = ("leverage", "points", "scenarios")
TARGETS = {"title": (0,), "bottom_two": (-1, -2)}
IN_PLAY = {"home_team": ["t04", "t05"], "away_team": ["t00", "t06"], "home_goals": [1, 0], "away_goals": [0, 0],
           "elapsed": [0.4, 0.0]}
HOME, AWAY = ["t00", "t01", "t02"], ["t01", "t02", "t00"]     # F = 3; with IN_PLAY the table has six rows


class StandInCtx:
    """TEST-ONLY stand-in for HipContext's three queries and their live forms: records every call under its method's
    name and answers with arrays of the documented shapes and dtypes (tests/fake_ctx.py is left as it is)."""

    def __init__(self):
        self.calls = []

    def _record(self, name, home_idx, table_idx, masks, kw, live):
        nf = len(home_idx) + (len(kw["in_play"][0]) if live else 0)
        self.calls.append(dict(kw, method=name, home_idx=np.array(home_idx), table_idx=np.array(table_idx)))
        extra = {"ess": 3.5, "log_evidence": -7.25} if live else {}
        return len(table_idx), nf, len(masks), extra

    def _leverage(self, name, live, home_idx, away_idx, table_idx, table, points, n_sims, key, masks, **kw):
        n, nf, k, extra = self._record(name, home_idx, table_idx, masks, kw, live)
        outcome = np.zeros((nf, 3), dtype=np.uint64)
        outcome[:, 0] = n_sims
        return dict(extra, outcome=outcome, target=np.zeros((n, k), dtype=np.uint64),
                    joint=np.zeros((nf, 3, n, k), dtype=np.uint64))

    def _points(self, name, live, home_idx, away_idx, table_idx, table, points, n_sims, key, masks, points_min, n_bins,
                **kw):
        n, nf, k, extra = self._record(name, home_idx, table_idx, masks, dict(kw, points_min=points_min, n_bins=n_bins),
                                       live)
        first = np.zeros((n, n_bins), dtype=np.uint64)
        first[:, 0] = n_sims
        return dict(extra, team_points=first, team_target=np.zeros((n, n_bins, k), dtype=np.uint64),
                    position_points=first.copy(), gap=first[1:].copy())

    def _scenarios(self, name, live, home_idx, away_idx, table_idx, table, points, n_sims, key, masks, key_fixture,
                   key_cap, **kw):
        n, nf, k, extra = self._record(name, home_idx, table_idx, masks, dict(kw, key_fixture=np.array(key_fixture)), live)
        cells = int(np.prod(2 * np.asarray(key_cap) + 1))
        scenario = np.zeros(cells, dtype=np.uint64)
        scenario[0] = n_sims
        return dict(extra, scenario=scenario, joint=np.zeros((cells, n, k), dtype=np.uint64))

    def match_leverage(self, *a, **kw):
        return self._leverage("match_leverage", False, *a, **kw)

    def match_leverage_live(self, *a, **kw):
        return self._leverage("match_leverage_live", True, *a, **kw)

    def season_points(self, *a, **kw):
        return self._points("season_points", False, *a, **kw)

    def season_points_live(self, *a, **kw):
        return self._points("season_points_live", True, *a, **kw)

    def season_scenarios(self, *a, **kw):
        return self._scenarios("season_scenarios", False, *a, **kw)

    def season_scenarios_live(self, *a, **kw):
        return self._scenarios("season_scenarios_live", True, *a, **kw)


def _with_stand_in(m):
    ctx = StandInCtx()
    m._device = lambda: ctx
    return ctx


def _query(m, which, home=HOME, away=AWAY, keys=(1, 3, 4), **kw):
    kw.setdefault("num_simulations", 12)
    kw.setdefault("random_state", 1)
    if which == "leverage":
        return m.match_leverage(home, away, targets=TARGETS, **kw)
    if which == "points":
        return m.points_needed(home, away, targets=TARGETS, levels=(0.5,), **kw)
    return m.match_scenarios(home, away, list(keys), targets=TARGETS, **kw)


KICK_OFF = {"leverage": "match_leverage", "points": "season_points", "scenarios": "season_scenarios"}


@pytest.mark.parametrize("which", QUERIES)
def test_result_keys_shapes_and_dtypes(which):
    m = hand_posterior()
    ctx = _with_stand_in(m)
    S, N, n, K, F, L = m.attack.shape[0], 12, 6, 2, 3, 2
    plain = _query(m, which, keys=(1,))
    res = _query(m, which, in_play=IN_PLAY, log_weights=np.zeros(S), tiebreak="head_to_head")
    assert list(res["teams"]) == ["t00", "t01", "t02", "t04", "t05", "t06"]   # the in-play teams are table rows
    assert set(res) == set(plain) | {"ess", "log_evidence"} | ({"in_play"} if which == "leverage" else set())
    assert isinstance(res["ess"], float) and res["ess"] == 3.5 and res["log_evidence"] == -7.25
    if which == "leverage":
        assert res["in_play"].dtype == np.int64
        np.testing.assert_array_equal(res["in_play"], [F, F + 1])
        assert res["outcome_count"].shape == (F + L, 3) and res["joint_count"].shape == (F + L, 3, n, K)
        assert res["leverage"].shape == (F + L, n, K) and res["outcome_count"].dtype == np.int64
    elif which == "points":
        assert res["team_points_count"].shape == (n, res["points"].size) and res["team_points_count"].dtype == np.int64
        assert res["gap_count"].shape == (n - 1, res["points"].size)
    else:
        np.testing.assert_array_equal(res["fixtures"], [1, 3, 4])
        assert list(res["home"]) == ["t01", "t04", "t05"] and list(res["away"]) == ["t02", "t00", "t06"]
        assert res["scenario_count"].shape == (27,) and res["joint_count"].shape == (27, n, K)
        assert res["scenario_count"].dtype == np.int64 and res["shape"] == (3, 3, 3)
    call = ctx.calls[-1]
    assert call["method"] == KICK_OFF[which] + "_live"
    np.testing.assert_array_equal(call["home_idx"], [0, 1, 2])            # the fixtures still to kick off alone
    np.testing.assert_array_equal(call["in_play"][0], [4, 5])
    np.testing.assert_array_equal(call["in_play"][2], [1, 0])
    assert call["in_play"][2].dtype == np.uint8 and call["in_play"][4].dtype == np.float64
    assert call["reweight"] is True and call["log_weights"].shape == (S,)
    assert call["head_to_head"] is True and call["pair_init"].shape == (n, n)
    # log_weights alone, an empty in_play and reweight=False alone go the same way
    for kw in (dict(log_weights=np.zeros(S)), dict(in_play={k: [] for k in IN_PLAY}), dict(reweight=False)):
        res = _query(m, which, keys=(1,), **kw)
        assert ctx.calls[-1]["method"] == KICK_OFF[which] + "_live" and len(ctx.calls[-1]["in_play"][0]) == 0
        assert {"ess", "log_evidence"} <= set(res)
    assert ctx.calls[-1]["reweight"] is False and ctx.calls[-1]["log_weights"] is None


@pytest.mark.parametrize("which", QUERIES)
def test_the_defaults_call_the_kick_off_entry_point(which):
    m = hand_posterior()
    ctx = _with_stand_in(m)
    res = _query(m, which, keys=(1,))
    res2 = _query(m, which, keys=(1,), in_play=None, reweight=True, log_weights=None)
    assert [c["method"] for c in ctx.calls] == [KICK_OFF[which]] * 2
    assert "in_play" not in ctx.calls[0] and "reweight" not in ctx.calls[0] and "log_weights" not in ctx.calls[0]
    assert set(res) == set(res2) and not {"ess", "log_evidence", "in_play"} & set(res)
    want = {"leverage": {"teams", "targets", "outcome_count", "outcome_proba", "target_count", "target_proba",
                         "joint_count", "conditional_proba", "conditional_se", "leverage"},
            "points": {"teams", "targets", "levels", "points", "team_points_count", "team_target_count",
                       "position_points_count", "gap_count", "team_points_proba", "target_count", "target_proba",
                       "proba_given_points", "se_given_points", "proba_given_at_least", "points_needed",
                       "position_points_mean", "position_points_quantile", "level_proba"},
            "scenarios": {"teams", "targets", "fixtures", "home", "away", "margin_cap", "shape", "margins",
                          "scenario_count", "joint_count", "scenario_proba", "target_count", "target_proba",
                          "conditional_proba", "conditional_se", "settled", "leverage"}}[which]
    assert set(res) == want


def test_key_fixtures_index_the_concatenated_list():
    m = hand_posterior()
    ctx = _with_stand_in(m)
    res = m.match_scenarios(HOME, AWAY, [4], num_simulations=5, random_state=1, in_play=IN_PLAY)     # F + 1: the last
    assert list(res["home"]) == ["t05"] and list(res["away"]) == ["t06"]
    np.testing.assert_array_equal(ctx.calls[-1]["key_fixture"], [4])
    with pytest.raises(ValueError):
        m.match_scenarios(HOME, AWAY, [5], num_simulations=5, random_state=1, in_play=IN_PLAY)       # F + L
    with pytest.raises(ValueError):
        m.match_scenarios(HOME, AWAY, [3], num_simulations=5, random_state=1)                        # F without in_play
    assert len(ctx.calls) == 1


def test_the_points_axis_counts_in_play_matches():
    m = hand_posterior()
    ctx = _with_stand_in(m)
    table = {"t00": (10, 0, 0)}
    plain = m.points_needed(HOME, AWAY, num_simulations=5, random_state=1, current_table=table,
                            teams=["t00", "t01", "t02", "t04", "t05", "t06"], targets=TARGETS)
    live = m.points_needed(HOME, AWAY, num_simulations=5, random_state=1, current_table=table, targets=TARGETS,
                           in_play=IN_PLAY)
    # t00 has two fixtures to come and one match in play: 10 .. 16 without it, 10 .. 19 with it
    assert plain["points"][-1] == 16 and live["points"][-1] == 19 and live["points"][0] == 0
    assert ctx.calls[-1]["points_min"] == 0 and ctx.calls[-1]["n_bins"] == 20
    # t04 plays only its match in play: 0 .. 3 points
    assert ctx.calls[-1]["method"] == "season_points_live"


def test_the_pair_bound_counts_in_play_matches_as_meetings():
    m = hand_posterior()
    _with_stand_in(m)
    played = {"home_team": ["t00"], "away_team": ["t01"], "home_goals": [65535 - 255], "away_goals": [0]}
    ip = {"home_team": ["t01"], "away_team": ["t00"], "home_goals": [0], "away_goals": [0], "elapsed": [0.1]}
    kw = dict(num_simulations=5, random_state=1, tiebreak="head_to_head", played=played, targets={"title": (0,)},
              current_table={"t00": (3, 9, 0), "t01": (0, 0, 9)})
    m.match_leverage([], [], in_play=ip, **kw)                        # one meeting to come: 255 more goals still fit
    with pytest.raises(ValueError, match="16 bits"):
        m.match_leverage(["t00"], ["t01"], in_play=ip, **kw)          # two


@pytest.mark.parametrize("which", QUERIES)
def test_every_argument_check_runs_before_a_context_is_touched(which):
    m = hand_posterior()
    S = m.attack.shape[0]
    good = {"home_team": ["t04"], "away_team": ["t05"], "home_goals": [1], "away_goals": [0], "elapsed": [0.4]}

    def bad(in_play=good, home=("t00",), away=("t01",), **kw):
        with pytest.raises(ValueError):
            _query(m, which, list(home), list(away), keys=(0,), in_play=in_play, **kw)
        assert m._predict_ctx is None

    for change in ({"elapsed": [1.0]}, {"elapsed": [-0.1]}, {"elapsed": [float("nan")]}, {"elapsed": ["x"]},
                   {"elapsed": [0.0]},                                   # 1-0 at elapsed = 0
                   {"home_goals": [64]}, {"away_goals": [-1]}, {"home_goals": [1.5]}, {"home_goals": [True]},
                   {"home_goals": [None]}, {"home_team": ["nope"]}, {"away_team": ["t04"]},
                   {"home_team": ["t04", "t05"]}, {"elapsed": [0.1, 0.2]}):
        bad(dict(good, **change))
    bad({k: v for k, v in good.items() if k != "elapsed"})
    bad("t04")
    bad(teams=["t00", "t01", "t04"])                                     # t05 is not a row of the table
    bad(log_weights=np.zeros(S + 1))
    bad(log_weights=np.full(S, np.inf))
    bad(log_weights=np.full(S, np.nan))
    bad(log_weights="x")
    # the same messages as simulate_season's
    for change, text in (({"elapsed": [0.0]}, "elapsed = 0 with a score other than 0-0"), ({"home_goals": [64]}, "0..63")):
        with pytest.raises(ValueError) as there:
            m.simulate_season(["t00"], ["t01"], num_simulations=10, in_play=dict(good, **change))
        with pytest.raises(ValueError, match=text) as here:
            _query(m, which, ["t00"], ["t01"], keys=(0,), in_play=dict(good, **change))
        assert str(here.value) == str(there.value)
    # F + L beyond the fixture bound
    big = LEVERAGE_MAX_FIXTURES
    with pytest.raises(ValueError, match="fixtures"):
        _query(m, which, np.zeros(big, np.uint16), np.ones(big, np.uint16), keys=(0,), in_play=good)
    assert m._predict_ctx is None
