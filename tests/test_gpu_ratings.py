"""team_ratings on the device (csrc/dc_ratings.hip.h, bpl/ratings.py) against the numpy restatement
(tests/ratings_ref.py: the full scoreline grid of every draw and match, the running sums match by match,
np.quantile and the rank rule as a double loop) for the five predictor classes, against predict_markets, and on
shape edges, exact ties, clipped tau, chunking, determinism and the library's own errors.

Gates, from the project's own: tests/test_gpu_scores.py holds each outcome probability to 1e-12 absolute, and a
mean over at most 2 046 matches adds at most 2 046 x 2^-53.  So "win" within 2e-12, "points" within
2e-12 max(1, |W| + |D| + |L|), the three goal statistics within 1e-12 max(1, the largest rate in the
restatement) (the log rates are bit-identical by construction: only the two exp implementations differ).
Summaries as tests/test_gpu_markets.py holds its own: the mean within the gate g, a quantile within g plus one
rounding, sd within 10 g.  The rank counts are compared exactly, with the rule applied to the device's own draws
and with the restatement's counts (tests/test_ratings_host.py asserts the separation that guarantees it)."""
import numpy as np
import pytest

import loglik_ref as LR
import ratings_ref as RR
from bpl import markets as MK
from bpl._ffi import BPLHIP_EINVAL, BPLHIP_ESTATE, BplHipError, HipContext

pytestmark = pytest.mark.gpu

QS = (0.0, 0.05, 0.5, 0.95, 1.0)
ARRAYS = ("mean", "sd", "quantile", "draws")
COUNTS = ("rank_count", "better_count")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _gates(points, top_rate):
    goal = 1e-12 * max(1.0, top_rate)
    return np.array([RR.points_gate(points), 2e-12, goal, goal, goal])   # g [5], in the order of the statistics


def _compare(got, ref, g, tag):
    """`got` (one gameweek, no leading axis) against the restatement `ref` within the gates; prints the measured
    maxima over the gate."""
    for key in ARRAYS:
        assert not np.isnan(got[key]).any(), key
        assert got[key].shape == ref[key].shape, (key, got[key].shape, ref[key].shape)
    S = ref["draws"].shape[0]
    one = 2.0 ** -52 * np.maximum(1.0, np.abs(ref["draws"]).max(axis=(0, 2)))   # one rounding of a value, per statistic
    err = {"draws": (np.abs(got["draws"] - ref["draws"]).max(axis=(0, 2)), g),
           "mean": (np.abs(got["mean"] - ref["mean"]).max(axis=1), g),
           "sd": (np.abs(got["sd"] - ref["sd"]).max(axis=1), 10 * g),
           "quantile": (np.abs(got["quantile"] - ref["quantile"]).reshape(5, -1).max(axis=1, initial=0.0), g + one)}
    for key, (e, gate) in err.items():
        print(f"{tag}: {key} error / gate {(e / gate).max():.3e} (S={S})")
    for key, (e, gate) in err.items():
        assert (e <= gate).all(), (key, (e / gate).max())
    np.testing.assert_array_equal(got["matches"], ref["matches"])


def _counts(got, ref, rank_by="points"):
    """The device's counts: the rank rule on the device's own draws, and the restatement's counts."""
    k = RR.STATISTICS.index(rank_by)
    S = got["draws"].shape[0]
    own = RR.ranks(got["draws"][:, k, :])
    for key, mine, theirs in zip(COUNTS, own, (ref["rank_count"], ref["better_count"])):
        assert got[key].dtype == np.int64
        np.testing.assert_array_equal(got[key], mine, err_msg=f"{key}: the rule on the device's own draws")
        np.testing.assert_array_equal(got[key], theirs, err_msg=f"{key}: the restatement's counts")
    assert (got["rank_count"].sum(axis=0) == S).all() and (got["rank_count"].sum(axis=1) == S).all()
    np.testing.assert_array_equal(got["rank_proba"], got["rank_count"] / S)
    np.testing.assert_array_equal(got["better_proba"], got["better_count"] / S)
    R = got["rank_count"].shape[0]
    np.testing.assert_allclose(got["expected_rank"], (got["rank_proba"] * np.arange(R)).sum(axis=1), rtol=1e-14)


def _first(r):
    """A dynamic result's single gameweek without the leading axis."""
    if "gameweeks" not in r:
        return r
    lead = ARRAYS + COUNTS + ("rank_proba", "better_proba", "expected_rank")
    return {k: (v[0] if k in lead else v) for k, v in r.items()}


def _extra(kind, m):
    return {"team_conf": RR.conf_of(m)} if kind == "wc" else {}


def _check(kind, m, tag, teams=None, opponents=None, venue=None, G=15, points=(3, 1, 0), rank_by="points",
           quantiles=QS, team_conf=None, counts=True):
    extra = {"team_conf": team_conf} if team_conf is not None else {}
    got = _first(m.team_ratings(teams, opponents, venue=venue, max_goals=G, points=points, rank_by=rank_by,
                                quantiles=quantiles, return_draws=True, **extra))
    ref = RR.team_ratings(m, teams, opponents, venue, G, points, rank_by, quantiles, team_conf,
                          week=m.num_gameweeks - 1 if kind == "dynamic" else None)
    assert got["kind"] == "ratings" and got["statistics"] == RR.STATISTICS
    _compare(got, ref, _gates(points, ref["top_rate"]), tag)
    if counts:
        _counts(got, ref, rank_by)
    return got, ref


# 1
@pytest.mark.parametrize("G", [1, 2, 15])
@pytest.mark.parametrize("kind", LR.KINDS)
def test_all_classes_against_restatement(kind, G):
    m = LR.hand_model(kind, S=257, T=8, seed=3)
    for venue, points in RR.class_cases(kind, G):
        _check(kind, m, f"{kind} G={G} {venue} {points}", venue=venue, G=G, points=points,
               team_conf=_extra(kind, m).get("team_conf"))


# 2
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 257])
@pytest.mark.parametrize("kind", ["basic", "wc"])
def test_draw_count_edges(kind, S):
    # across the 64-draw tile and the 256-draw workgroup; G over its range; subsets in non-model order with an
    # overlapping field: t04 is absent from it, t01 and t03 are in it
    m = LR.hand_model(kind, S=S, T=6, seed=S)
    conf = _extra(kind, m).get("team_conf")
    teams, field = ["t04", "t01", "t03"], ["t01", "t05", "t00", "t03"]
    for G in (0, 1, 63):
        # (draws that round to equal points are not excluded here: the counts are held to the rule on the device's
        # own draws in _edge_counts, not to the restatement's)
        got, _ = _check(kind, m, f"{kind} S={S} G={G}", teams, field, venue="both", G=G, team_conf=conf, counts=False)
        _edge_counts(got, S)
        assert got["matches"].tolist() == [8, 6, 6] and got["teams"] == teams and got["opponents"] == field
    if S == 1:
        assert (got["sd"] == 0.0).all()
        assert (got["quantile"] == got["draws"][0][:, None, :]).all()   # every quantile is the single value
        assert sorted(got["rank_count"].sum(axis=0).tolist()) == [1, 1, 1] and set(got["rank_count"].ravel()) == {0, 1}


def _edge_counts(got, S):
    own = RR.ranks(got["draws"][:, 0, :])
    np.testing.assert_array_equal(got["rank_count"], own[0])
    np.testing.assert_array_equal(got["better_count"], own[1])
    assert (got["rank_count"].sum(axis=0) == S).all() and (got["rank_count"].sum(axis=1) == S).all()


@pytest.mark.parametrize("R", [1, 2, 3, 65])
def test_team_count_edges(R):
    # R = 65 is the first size past one lane-width of rank bins (T = 65); R = 1 is rated against two opponents
    T = max(R, 3)
    m = LR.hand_model("neutral", S=70, T=T, seed=R)
    names = [str(t) for t in m.teams]
    teams = names[:R][::-1]
    field = names[1:3] if R == 1 else None
    got, _ = _check("neutral", m, f"R={R}", teams, field, venue="neutral", G=6, counts=False)
    _edge_counts(got, 70)
    assert got["rank_count"].shape == (R, R) and got["matches"].tolist() == [2 if R == 1 else R - 1] * R
    if R == 1:
        assert got["rank_count"].tolist() == [[70]] and got["better_count"].tolist() == [[0]]


# 3
@pytest.mark.parametrize("kind", ["extended", "wc"])
def test_exact_ties_rank_in_the_order_given(kind):
    S, T = 130, 5
    m = LR.hand_model(kind, S=S, T=T, seed=7)
    for nm in ("attack", "defence", "home_advantage", "home_attack", "away_attack", "home_defence", "away_defence"):
        a = getattr(m, nm, None)
        if a is not None and np.ndim(a) == 2:
            a[:, 1] = a[:, 0]
    conf = _extra(kind, m).get("team_conf")
    if conf:
        conf["t01"] = conf["t00"]
    names = [str(t) for t in m.teams]
    field = names[2:]   # neither twin is in the field: the two play the same matches
    for order in (names, [names[1], names[0]] + names[2:]):
        got, _ = _check(kind, m, f"ties {kind} {order[0]} first", order, field, venue="both", G=10, team_conf=conf)
        v = got["draws"][:, 0, :]
        assert v[:, 0].tobytes() == v[:, 1].tobytes()                # bitwise equal values
        assert got["better_count"][0, 1] == got["better_count"][1, 0] == 0
        rank_of = lambda t: (got["rank_count"][t] * np.arange(T)).sum()   # the sum of the ranks over the draws
        assert rank_of(1) - rank_of(0) == S                          # the one listed first is one rank better, always
        for r in range(T - 1):
            assert got["rank_count"][0, r] == got["rank_count"][1, r + 1]


# 4
def test_clipped_tau_agrees_and_has_no_nan():
    m = LR.hand_model("basic", S=64, T=4, seed=2)
    m.corr_coef = np.where(np.arange(64) % 3 == 0, 5.0, 0.01)   # 1 - rho lh la < 0 and 1 - rho < 0 on some draws
    for G in (0, 1, 15):
        got, _ = _check("basic", m, f"clipped G={G}", G=G, counts=False)
        _edge_counts(got, 64)
        # everything but the goal difference (statistic 4) is non-negative
        for key, v in (("draws", got["draws"][:, :4]), ("mean", got["mean"][:4]), ("quantile", got["quantile"][:4])):
            assert np.isfinite(got[key]).all() and (v >= 0.0).all(), key
        assert (got["sd"] >= 0.0).all()


# 5
def test_points_against_predict_markets():
    # an independent device path: the market with weights W, D, L on the three triangles, per draw, averaged over the
    # same pairings in the same order.  Gate: the markets gate 1e-12 max(1, max|w|) plus the points gate
    S, T, G, pts = 130, 6, 15, (3, 1, 0)
    m = LR.hand_model("basic", S=S, T=T, seed=11)
    names = [str(t) for t in m.teams]
    got = m.team_ratings(max_goals=G, points=pts, return_draws=True)
    x, y = np.meshgrid(np.arange(G + 1), np.arange(G + 1), indexing="ij")
    w_home = pts[0] * (x > y) + pts[1] * (x == y) + pts[2] * (x < y)    # the home side's points
    w_away = pts[0] * (x < y) + pts[1] * (x == y) + pts[2] * (x > y)
    rows, n = RR.fixtures_of(list(range(T)), list(range(T)), "both")
    d = {"home_team": [names[r[0]] for r in rows], "away_team": [names[r[1]] for r in rows]}
    mk = m.predict_markets(d, {"home": w_home.astype(float), "away": w_away.astype(float)}, max_goals=G, quantiles=(),
                           return_draws=True)["draws"]                 # [S, 2, n]
    want = np.zeros((S, T))
    for j, r in enumerate(rows):
        want[:, r[6]] = want[:, r[6]] + mk[:, 0 if r[5] else 1, j]
    want = want / n
    gate = 1e-12 * max(1.0, float(max(pts))) + RR.points_gate(pts)
    err = np.abs(got["draws"][:, 0, :] - want).max()
    print(f"points against predict_markets: error / gate {err / gate:.3e}")
    assert err <= gate, err / gate


# 6
def _bits_equal(a, b, keys):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("kind", ["basic", "wc"])
def test_chunked_workspace_and_two_runs_are_byte_identical(kind):
    S, T = 257, 8
    m = LR.hand_model(kind, S=S, T=T, seed=3)
    ctx = m._device()
    t = np.array([5, 0, 7, 2, 3, 1, 6], dtype=np.uint16)
    o = np.arange(T, dtype=np.uint16)[::-1].copy()
    conf = {"team_conf": t % 3, "opponent_conf": o % 3} if kind == "wc" else {}
    kw = dict(venue=0, max_goals=15, points=(3, 1, 0), rank_by=4, quantiles=QS, return_draws=True, **conf)
    keys = ARRAYS + COUNTS + ("matches",)
    whole = ctx.team_ratings(t, o, **kw)
    _bits_equal(whole, ctx.team_ratings(t, o, **kw), keys)                                   # two runs
    _bits_equal(whole, ctx.team_ratings(t, o, workspace_bytes=5 * S * 8, **kw), keys)        # exactly one team
    _bits_equal(whole, ctx.team_ratings(t, o, workspace_bytes=3 * 5 * S * 8 + 5, **kw), keys)   # chunks of 3, 3, 1
    assert whole["draws"].shape == (S, 5, 7) and whole["rank_count"].dtype == np.int32
    np.testing.assert_array_equal(whole["rank_count"], RR.ranks(whole["draws"][:, 4, :])[0])   # ranked by goal difference


# 7
def test_world_cup_confederations_enter_the_values():
    m = LR.hand_model("wc", S=65, T=6, seed=13)
    conf = RR.conf_of(m)
    got, _ = _check("wc", m, "wc", venue="neutral", G=10, team_conf=conf)
    swapped = dict(conf, t00=conf["t01"], t01=conf["t00"])    # (t00 in c0, t01 in c1)
    assert swapped != conf
    other, _ = _check("wc", m, "wc swapped", venue="neutral", G=10, team_conf=swapped)
    for t in (0, 1):
        assert not np.array_equal(got["draws"][:, :, t], other["draws"][:, :, t])
    flat = dict.fromkeys(conf, "c0")                          # one confederation: the terms cancel
    none, _ = _check("wc", m, "wc one confederation", venue="neutral", G=10, team_conf=flat)
    assert not np.array_equal(none["draws"], got["draws"])


# 8
def test_dynamic_gameweeks_stack_the_single_calls():
    m = LR.hand_model("dynamic", S=130, T=6, seed=17, G=4)
    both = m.team_ratings(gameweek=[0, 2], return_draws=True)
    assert both["gameweeks"].tolist() == [0, 2] and both["draws"].shape == (2, 130, 5, 6)
    lead = ARRAYS + COUNTS + ("rank_proba", "better_proba", "expected_rank")
    for w, g in enumerate((0, 2)):
        one = m.team_ratings(gameweek=g, return_draws=True)
        for key in lead:
            assert one[key][0].tobytes() == both[key][w].tobytes(), (key, g)
        ref = RR.team_ratings(m, quantiles=(0.05, 0.5, 0.95), week=g)
        _compare(_first(one), ref, _gates((3, 1, 0), ref["top_rate"]), f"dynamic week {g}")
    assert not np.array_equal(both["draws"][0], both["draws"][1])


# 9
def test_library_errors():
    t = np.array([0, 1], dtype=np.uint16)
    ctx = HipContext(0)
    base = dict(venue=0, max_goals=15, points=(3, 1, 0))

    def fails(code, teams, opponents, **kwargs):
        with pytest.raises(BplHipError) as e:
            ctx.team_ratings(teams, opponents, **{**base, **kwargs})
        assert e.value.code == code, (e.value.code, kwargs)

    fails(BPLHIP_ESTATE, t, t)                                   # no posterior uploaded
    rs = np.random.RandomState(0)
    S, T = 10, 3
    ctx.predict_set_posterior(rs.normal(0, 0.2, (S, T)), rs.normal(0, 0.2, (S, T)), rs.normal(0, 0.1, S),
                              rs.uniform(-0.05, 0.05, S))
    fails(BPLHIP_EINVAL, t, t, workspace_bytes=5 * S * 8 - 1)    # holds no team
    fails(BPLHIP_EINVAL, t, t, workspace_bytes=-1)
    fails(BPLHIP_EINVAL, np.array([0, 1, 0], dtype=np.uint16), t)    # a duplicate team
    fails(BPLHIP_EINVAL, t, np.array([1, 1], dtype=np.uint16))       # a duplicate opponent
    fails(BPLHIP_EINVAL, np.array([0, T], dtype=np.uint16), t)       # an index beyond T
    fails(BPLHIP_EINVAL, t, t, venue=3)                              # neutral ground on a plain posterior
    fails(BPLHIP_EINVAL, t, t, venue=4)
    fails(BPLHIP_EINVAL, t[:1], t[:1])                               # its only opponent is itself
    fails(BPLHIP_EINVAL, t[:0], t)
    fails(BPLHIP_EINVAL, t, t, max_goals=64)
    fails(BPLHIP_EINVAL, t, t, rank_by=5)
    fails(BPLHIP_EINVAL, t, t, points=(3, np.inf, 0))
    fails(BPLHIP_EINVAL, t, t, quantiles=[0.5, 1.5])
    fails(BPLHIP_EINVAL, t, t, quantiles=np.linspace(0, 1, 17))
    fails(BPLHIP_EINVAL, t, t, team_conf=t, opponent_conf=t)         # confederations on a posterior without them
    out = ctx.team_ratings(t, t, workspace_bytes=5 * S * 8, quantiles=[0.1, 0.9], return_draws=True, **base)
    assert out["mean"].shape == (5, 2) and out["quantile"].shape == (5, 2, 2) and out["draws"].shape == (S, 5, 2)
    assert out["matches"].tolist() == [2, 2] and np.isfinite(out["draws"]).all()
    ctx.close()
