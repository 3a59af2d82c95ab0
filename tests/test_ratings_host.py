"""team_ratings without a GPU (bpl/ratings.py): result keys, shapes and dtypes for each class through a stand-in
context whose `team_ratings` is the numpy restatement (tests/ratings_ref.py), every argument check, made on the
host before a device context is touched, the restatement itself on a posterior worked by hand, the invariants
of the rank counts, `format_table`, and the separation the exact rank comparisons of tests/test_gpu_ratings.py
rest on."""
import numpy as np
import pytest
from scipy.stats import skellam

import loglik_ref as LR
import ratings_ref as RR
from bpl import ratings as RT
from fake_ctx import FakePredictCtx


class FailCtx:
    """A device context that must never be touched."""

    def __getattr__(self, name):
        raise AssertionError(f"device call {name} before the host checks finished")


class RatingsCtx(FakePredictCtx):
    """FakePredictCtx plus `team_ratings`, computed by the restatement from the uploaded posterior."""

    def __init__(self):
        self.calls = []

    def team_ratings(self, teams, opponents, venue, max_goals, points, rank_by=0, quantiles=(), team_conf=None,
                     opponent_conf=None, return_draws=False, workspace_bytes=0):
        self.calls.append((len(teams), len(opponents), venue))
        log_rates = lambda h, a, neutral, conf: self._log_rates(h, a, neutral, conf)
        log_rates.plain = self.venue is None
        out = RR.device_part(log_rates, self.cc, list(teams), list(opponents), RR.VENUES[venue], max_goals, points,
                             RR.STATISTICS[rank_by], quantiles, team_conf, opponent_conf, return_draws)
        out.pop("top_rate")
        return out


def _extra(kind, m):
    return {"team_conf": RR.conf_of(m)} if kind == "wc" else {}


@pytest.mark.parametrize("kind", LR.KINDS)
def test_result_keys_shapes_and_dtypes(kind):
    S, T = 9, 6
    m = LR.hand_model(kind, S=S, T=T, seed=1)
    m._predict_ctx = ctx = RatingsCtx()
    qs = (0.0, 0.1, 0.5, 1.0)
    r = m.team_ratings(quantiles=qs, return_draws=True, max_goals=5, **_extra(kind, m))
    venue_model = kind in ("neutral", "wc", "dynamic")
    assert set(r) == {"kind", "teams", "opponents", "venue", "statistics", "quantiles", "mean", "sd", "quantile",
                      "rank_count", "rank_proba", "better_count", "better_proba", "expected_rank", "matches",
                      "draws"} | ({"gameweeks"} if kind == "dynamic" else set())
    assert r["kind"] == "ratings" and r["statistics"] == RR.STATISTICS == RT.STATISTICS
    assert r["teams"] == [f"t{i:02d}" for i in range(T)] == r["opponents"]
    assert r["venue"] == ("neutral" if venue_model else "both")           # the default per class
    assert ctx.calls == [(T, T, 3 if venue_model else 0)]
    assert r["quantiles"].dtype == np.float64 and r["quantiles"].tolist() == list(qs)
    assert r["matches"].shape == (T,) and r["matches"].dtype.kind == "i"
    assert r["matches"].tolist() == [(T - 1) * (1 if venue_model else 2)] * T
    lead = (1,) if kind == "dynamic" else ()
    for key, shape, dtype in (("mean", (5, T), np.float64), ("sd", (5, T), np.float64),
                              ("quantile", (5, 4, T), np.float64), ("rank_count", (T, T), np.int64),
                              ("rank_proba", (T, T), np.float64), ("better_count", (T, T), np.int64),
                              ("better_proba", (T, T), np.float64), ("expected_rank", (T,), np.float64),
                              ("draws", (S, 5, T), np.float64)):
        assert r[key].shape == lead + shape and r[key].dtype == dtype, key
    if kind == "dynamic":
        assert r["gameweeks"].tolist() == [m.num_gameweeks - 1] and r["gameweeks"].dtype == np.int64
    ref = RR.team_ratings(m, G=5, quantiles=qs, team_conf=_extra(kind, m).get("team_conf"),
                          week=m.num_gameweeks - 1 if kind == "dynamic" else None)
    first = (lambda a: a[0]) if kind == "dynamic" else (lambda a: a)
    for key in ("mean", "sd", "quantile", "draws", "rank_count", "better_count"):
        np.testing.assert_array_equal(first(r[key]), ref[key], err_msg=key)
    np.testing.assert_array_equal(r["rank_proba"], r["rank_count"] / S)
    np.testing.assert_array_equal(r["better_proba"], r["better_count"] / S)
    np.testing.assert_allclose(first(r["expected_rank"]), (first(r["rank_proba"]) * np.arange(T)).sum(axis=1), rtol=1e-14)
    # the goal difference is the difference of the two rates; without return_draws there are no draws; Q = 0 is allowed
    np.testing.assert_allclose(r["mean"][..., 4, :], r["mean"][..., 2, :] - r["mean"][..., 3, :], atol=1e-14)
    r2 = m.team_ratings(quantiles=(), max_goals=5, **_extra(kind, m))
    assert "draws" not in r2 and r2["quantile"].shape == lead + (5, 0, T) and r2["quantiles"].shape == (0,)
    np.testing.assert_array_equal(r2["mean"], r["mean"])


def test_dynamic_gameweeks_stack_the_single_calls():
    m = LR.hand_model("dynamic", S=9, T=5, seed=2, G=4)
    m._predict_ctx = ctx = RatingsCtx()
    both = m.team_ratings(gameweek=[0, 2], return_draws=True, max_goals=4)
    assert both["gameweeks"].tolist() == [0, 2] and len(ctx.calls) == 2 and both["mean"].shape == (2, 5, 5)
    for w, g in enumerate((0, 2)):
        one = m.team_ratings(gameweek=g, return_draws=True, max_goals=4)
        assert one["gameweeks"].tolist() == [g]
        for key in ("mean", "sd", "quantile", "rank_count", "rank_proba", "better_count", "better_proba",
                    "expected_rank", "draws"):
            assert one[key].shape[0] == 1 and one[key][0].tobytes() == both[key][w].tobytes(), key
    assert not np.array_equal(both["mean"][0], both["mean"][1])
    np.testing.assert_array_equal(m.team_ratings(max_goals=4)["mean"][0], m.team_ratings(gameweek=3, max_goals=4)["mean"][0])


@pytest.mark.parametrize("kind", LR.KINDS)
def test_team_order_subsets_and_matches(kind):
    m = LR.hand_model(kind, S=5, T=6, seed=3)
    m._predict_ctx = RatingsCtx()
    teams, opponents = ["t04", "t01", "t03"], ["t01", "t05", "t00", "t04"]   # t03 is absent from the field
    r = m.team_ratings(teams, opponents, venue="home", max_goals=4, return_draws=True, **_extra(kind, m))
    assert r["teams"] == teams and r["opponents"] == opponents and r["venue"] == "home"
    assert r["matches"].tolist() == [3, 3, 4]
    assert m.team_ratings(teams, opponents, venue="both", max_goals=4, **_extra(kind, m))["matches"].tolist() == [6, 6, 8]
    # the order given is kept: the reversed call is the reversed result
    rev = m.team_ratings(teams[::-1], opponents, venue="home", max_goals=4, return_draws=True, **_extra(kind, m))
    np.testing.assert_array_equal(rev["draws"][..., ::-1], r["draws"])
    # one name stands for a list of one
    one = m.team_ratings("t03", opponents, venue="away", max_goals=4, **_extra(kind, m))
    assert one["teams"] == ["t03"] and one["rank_count"].reshape(-1).tolist() == [5]


def _raises(m, **kwargs):
    m._predict_ctx = FailCtx()
    with pytest.raises(ValueError):
        m.team_ratings(**kwargs)


@pytest.mark.parametrize("kind", LR.KINDS)
def test_argument_checks_run_on_the_host(kind):
    m = LR.hand_model(kind, S=16)
    ok = _extra(kind, m)
    for key in ("teams", "opponents"):
        _raises(m, **{key: ["t00", "t01", "t00"]}, **ok)        # a duplicate
        _raises(m, **{key: ["t00", "nope"]}, **ok)              # an unknown team
        _raises(m, **{key: []}, **ok)                           # none
        _raises(m, **{key: [0, 1]}, **ok)                       # not names
        _raises(m, **{key: 3}, **ok)
    _raises(m, teams=["t00"], opponents=["t00"], **ok)          # its only opponent is itself
    _raises(m, teams=["t01", "t00"], opponents=["t00"], **ok)
    _raises(m, teams="t02", **ok)                               # (the field defaults to the rated teams)
    for v in ("nowhere", 0, 3, True, ("home",)):
        _raises(m, venue=v, **ok)
    if kind in ("basic", "extended"):
        _raises(m, venue="neutral")
    for g in (-1, 64, 2.0, True, None, "15"):
        _raises(m, max_goals=g, **ok)
    for p in ((3, 1), (3, 1, -1), "abc", (3.5, 1, 0), (3, 1, 0, 0), None, (1001, 1, 0)):
        _raises(m, points=p, **ok)
    for rb in ("elo", 0, None, ("points",)):
        _raises(m, rank_by=rb, **ok)
    _raises(m, quantiles=np.linspace(0, 1, 17), **ok)
    for q in (1.5, -0.1, np.nan, np.inf):
        _raises(m, quantiles=(0.5, q), **ok)
    _raises(m, quantiles=[[0.5]], **ok)
    _raises(m, quantiles=("a",), **ok)
    if kind == "wc":
        conf = ok["team_conf"]
        _raises(m)                                              # team_conf is required
        _raises(m, team_conf={k: v for k, v in conf.items() if k != "t03"})
        _raises(m, team_conf=dict(conf, t03="nope"))
        _raises(m, teams=["t00", "t01"], opponents=["t02", "t03"], team_conf={k: conf[k] for k in ("t00", "t01", "t02")})
    if kind == "dynamic":
        for g in (m.num_gameweeks, -1, "a", [], [0, m.num_gameweeks], True, 1.5, [0, None, 1.0]):
            _raises(m, gameweek=g)
    if kind == "neutral":
        with pytest.raises(TypeError):
            m.team_ratings(team_conf={})                        # only the World-Cup class takes it


def test_count_limits_run_on_the_host():
    big = LR.hand_model("neutral", S=65537, T=2)
    _raises(big)                                                # too many draws
    wide = LR.hand_model("basic", S=1, T=1026)
    names = [str(t) for t in wide.teams]
    _raises(wide)                                               # 1026 rated teams
    _raises(wide, teams=names[:3], opponents=names[:1025])      # 1025 opponents
    wide._predict_ctx = RatingsCtx()
    assert wide.team_ratings(teams=names[:2], opponents=names[:1024], max_goals=1)["matches"].tolist() == [2046, 2046]


# ---- the restatement itself
def test_restatement_on_a_posterior_worked_by_hand():
    # 3 teams, 2 draws, no home advantage, rho = 0.  Draw 0: every table 0, so every rate is 1 and all three teams
    # tie exactly.  Draw 1: attack = log(2, 1, 1/2), defence 0, so a team scores at its own rate 2, 1, 1/2 against
    # anybody, anywhere, and concedes at the mean of the others' rates
    m = LR.hand_model("basic", S=2, T=3)
    m.attack = np.array([[0.0, 0.0, 0.0], np.log([2.0, 1.0, 0.5])])
    m.defence = np.zeros((2, 3))
    m.home_advantage = np.zeros(2)
    m.corr_coef = np.zeros(2)
    r = RR.team_ratings(m, G=40, quantiles=(0.0, 0.5, 1.0))
    v = r["draws"]
    assert r["matches"].tolist() == [4, 4, 4]
    gf = np.array([[1.0, 1.0, 1.0], [2.0, 1.0, 0.5]])
    ga = np.array([[1.0, 1.0, 1.0], [0.75, 1.25, 1.5]])
    np.testing.assert_allclose(v[:, 2], gf, rtol=1e-15)
    np.testing.assert_allclose(v[:, 3], ga, rtol=1e-15)
    np.testing.assert_allclose(v[:, 4], gf - ga, rtol=0, atol=1e-15)
    win = lambda a, b: 1.0 - skellam.cdf(0, a, b)       # P(Poisson(a) > Poisson(b))
    draw = lambda a, b: skellam.pmf(0, a, b)
    rate = [2.0, 1.0, 0.5]
    for t in range(3):
        others = [u for u in range(3) if u != t]
        pw = np.mean([win(rate[t], rate[u]) for u in others])
        pd = np.mean([draw(rate[t], rate[u]) for u in others])
        np.testing.assert_allclose(v[1, 1, t], pw, rtol=0, atol=1e-13)
        np.testing.assert_allclose(v[1, 0, t], 3 * pw + pd, rtol=0, atol=1e-13)
    pd0 = draw(1.0, 1.0)
    np.testing.assert_allclose(v[0, 1], (1 - pd0) / 2, rtol=0, atol=1e-13)
    np.testing.assert_allclose(v[0, 0], 3 * (1 - pd0) / 2 + pd0, rtol=0, atol=1e-13)
    assert v[0, 0, 0] == v[0, 0, 1] == v[0, 0, 2]        # the exact tie: equal bits
    # ranks: the tie of draw 0 goes by the order of the teams, draw 1 by strength
    assert r["rank_count"].tolist() == [[2, 0, 0], [0, 2, 0], [0, 0, 2]]
    assert r["better_count"].tolist() == [[0, 1, 1], [0, 0, 1], [0, 0, 0]]
    rev = RR.team_ratings(m, teams=["t02", "t01", "t00"], G=40)
    assert rev["rank_count"].tolist() == [[1, 0, 1], [0, 2, 0], [1, 0, 1]]
    # summaries over the two draws
    np.testing.assert_allclose(r["mean"][2], [1.5, 1.0, 0.75], rtol=1e-15)
    np.testing.assert_allclose(r["sd"][2], np.array([1.0, 0.0, 0.5]) / np.sqrt(2.0), rtol=1e-15, atol=1e-16)
    np.testing.assert_allclose(r["quantile"][2], [[1.0, 1.0, 0.5], [1.5, 1.0, 0.75], [2.0, 1.0, 1.0]], rtol=1e-15)
    # points (2, 1, 0) and the other venues on the same posterior
    for venue, n in (("home", 2), ("away", 2)):
        alt = RR.team_ratings(m, venue=venue, G=40, points=(2, 1, 0))
        assert alt["matches"].tolist() == [n] * 3
        np.testing.assert_allclose(alt["draws"][:, 2:], v[:, 2:], rtol=1e-15, atol=1e-15)   # (no home advantage)
        np.testing.assert_allclose(alt["draws"][:, 0], 2 * v[:, 1] + (v[:, 0] - 3 * v[:, 1]), rtol=0, atol=1e-13)


@pytest.mark.parametrize("kind", LR.KINDS)
def test_rank_count_invariants(kind):
    S, T = 40, 7
    m = LR.hand_model(kind, S=S, T=T, seed=5)
    # two teams with equal columns tie exactly in every draw
    for nm in ("attack", "defence", "home_advantage", "home_attack", "away_attack", "home_defence", "away_defence"):
        a = getattr(m, nm, None)
        if a is not None and np.ndim(a) >= 2:
            a[..., 1] = a[..., 0]
    conf = _extra(kind, m).get("team_conf")
    if conf:
        conf["t01"] = conf["t00"]
    r = RR.team_ratings(m, G=6, team_conf=conf, week=0 if kind == "dynamic" else None)
    x = r["draws"][:, 0, :]
    assert (x[:, 0] == x[:, 1]).all()
    count, better = r["rank_count"].astype(np.int64), r["better_count"].astype(np.int64)
    assert (count.sum(axis=0) == S).all() and (count.sum(axis=1) == S).all()
    ties = np.array([[int((x[:, t] == x[:, u]).sum()) if t != u else S for u in range(T)] for t in range(T)])
    np.testing.assert_array_equal(better + better.T + ties, np.full((T, T), S))
    assert ties[0, 1] == S and better[0, 1] == better[1, 0] == 0 and (np.diag(better) == 0).all()


def test_format_table():
    result = {"kind": "ratings", "teams": ["Arsenal", "Bath", "C"], "opponents": ["Arsenal", "Bath", "C"],
              "venue": "both", "statistics": RT.STATISTICS, "quantiles": np.array([0.05, 0.5, 0.95]),
              "mean": np.array([[1.0, 2.125, 1.5], [0.2, 0.6, 0.4], [1, 2, 3], [3, 2, 1], [-2, 0, 2]], dtype=float),
              "quantile": np.arange(45, dtype=float).reshape(5, 3, 3) / 10,
              "expected_rank": np.array([1.75, 0.25, 1.0]),
              "rank_proba": np.array([[0.05, 0.15, 0.8], [0.8, 0.15, 0.05], [0.15, 0.7, 0.15]])}
    text = RT.format_table(result)
    lines = text.splitlines()
    assert len(lines) == 5 and lines[0].split() == ["team", "points", "q0.05", "q0.95", "E[rank]", "P(rank", "0)"]
    assert [ln.split()[0] for ln in lines[1:4]] == ["Bath", "C", "Arsenal"]       # best first by mean points
    assert lines[1].split()[1:] == ["2.125", "0.1", "0.7", "0.25", "0.800"]
    assert lines[4] == "3 teams against 3 opponents, venue both"
    by_gd = RT.format_table(result, sort_by="goal_difference", statistic="win").splitlines()
    assert by_gd[0].split()[1] == "win" and [ln.split()[0] for ln in by_gd[1:4]] == ["C", "Bath", "Arsenal"]
    assert by_gd[1].split()[1] == "0.4"
    assert len(RT.format_table(dict(result, quantiles=np.empty(0), quantile=np.empty((5, 0, 3)))).splitlines()[0].split()) == 5
    # a result of the dynamic class prints its last gameweek
    stacked = dict(result, gameweeks=np.array([0, 1]))
    for key in ("mean", "quantile", "expected_rank", "rank_proba"):
        stacked[key] = np.stack([np.zeros_like(result[key]), result[key]])
    assert RT.format_table(stacked) == text
    for bad in ("elo", None, 0):
        with pytest.raises(ValueError):
            RT.format_table(result, sort_by=bad)
    with pytest.raises(ValueError):
        RT.format_table(result, statistic="elo")


# ---- the separation precondition of the exact rank comparisons in tests/test_gpu_ratings.py
@pytest.mark.parametrize("G", [1, 2, 15])
@pytest.mark.parametrize("kind", LR.KINDS)
def test_ranked_values_are_separated(kind, G):
    # the device's points values are within points_gate of the restatement's, so two teams' device values keep the
    # restatement's order in a draw whenever the restatement's differ by more than twice the gate: asserted at 4 x
    m = LR.hand_model(kind, S=257, T=8, seed=3)
    for venue, points in RR.class_cases(kind, G):
        r = RR.team_ratings(m, venue=venue, G=G, points=points, team_conf=_extra(kind, m).get("team_conf"),
                            week=m.num_gameweeks - 1 if kind == "dynamic" else None)
        x = r["draws"][:, 0, :]
        gap = np.abs(x[:, :, None] - x[:, None, :])[:, ~np.eye(8, dtype=bool)].min()
        assert gap > 4 * RR.points_gate(points), (kind, venue, G, gap)
