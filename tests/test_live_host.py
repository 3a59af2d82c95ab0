"""simulate_season(..., in_play=..., log_weights=...) without a GPU: the numpy restatement (tests/live_ref.py) against
the separately written in-play restatement and against season_ref's kick-off sampler, systematic resampling's
counts, the flag share of the configurations tests/test_gpu_live.py runs, the result's keys through a stand-in
context, and every argument check (all made on the host before a context is touched)."""
import numpy as np
import pytest

import inplay_ref as IR
import live_cases as LC
import live_ref as LR
import season_ref as SR
from bpl.base import SEASON_MAX_FIXTURES, _prng_key
from test_playoff_host import hand_posterior


# ---- the conditional law
@pytest.mark.parametrize("rho", [-0.08, 0.9, -1.1])   # unclipped; clipped at (1, 1); clipped at (0, 1) / (1, 0)
def test_conditional_law_sums_to_one_and_is_the_in_play_grid(rho):
    lh, la, G = 1.7, 1.2, 40
    cells = np.eye((G + 1) ** 2).reshape((G + 1) ** 2, G + 1, G + 1)   # one "market" per final score
    for a in range(4):
        for b in range(4):
            for t in (0.0, 0.25, 0.999):
                if t == 0.0 and (a or b):
                    continue
                p = LR.conditional_pmf(lh, la, rho, a, b, t, G)
                assert abs(p.sum() - 1.0) < 1e-13, (a, b, t, p.sum())     # (the tail beyond 40 goals is below 1e-30)
                assert (p[:a] == 0).all() and (p[:, :b] == 0).all() and (p >= 0).all()
                val, _, Z, A = IR.one_fixture(np.array([lh]), np.array([la]), np.array([rho]), a, b, t, cells, G)
                # inplay_ref.gates' value bound with unit weights: the closed form of Z (4 + 204 A roundings over Z),
                # the grid-summed Z of that restatement (40) and a cell's own products and division here (8)
                rel = IR.EPS * ((4.0 + 204.0 * A[0]) / Z[0] + 40.0 + 8.0)
                # away from the mass that restatement's closed-form pmfs exp(k log mu - mu - lgamma(k + 1)) carry the
                # absolute rounding of their exponent's three terms: 4 EPS times their sizes, per side
                r, k = 1.0 - t, np.arange(G + 1, dtype=np.float64)
                eh = np.abs(k * np.log(lh * r)) + lh * r + IR.lgf(k)
                ea = np.abs(k * np.log(la * r)) + la * r + IR.lgf(k)
                expo = np.zeros((G + 1, G + 1))
                expo[a:, b:] = eh[:G + 1 - a, None] + ea[None, :G + 1 - b]
                assert np.all(np.abs(p.ravel() - val[0]) <= (rel + 4.0 * IR.EPS * expo.ravel()) * val[0]), (a, b, t)
    if rho == -1.1:
        assert LR.conditional_pmf(lh, la, rho, 0, 0, 0.25, G)[0, 1] == 0.0   # 1 + lh rho < 0: the cell is clipped


def test_kick_off_state_is_the_season_sampler_bit_for_bit():
    rs = np.random.RandomState(0)
    n = 10_000
    lh, la = np.exp(rs.normal(0.2, 0.5, n)), np.exp(rs.normal(0.0, 0.5, n))
    rho = np.where(rs.uniform(size=n) < 0.5, rs.uniform(-0.1, 0.1, n), rs.uniform(-1.5, 1.5, n))
    u1, u2 = SR.unit_open(rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)), rs.uniform(size=n)
    zero = np.zeros(n, dtype=np.int64)
    x, y, fl = LR.sample_conditional(lh, la, rho, zero, zero, np.full(n, 1.0 - 0.0), u1, u2)
    xs, ys, fs = SR.sample_scorelines(lh, la, rho, u1, u2)
    np.testing.assert_array_equal(x, xs)
    np.testing.assert_array_equal(y, ys)
    np.testing.assert_array_equal(fl, fs)
    assert x.max() > 3 and y.max() > 3


@pytest.mark.parametrize("state,rho", [((1, 0, 0.5), 0.05), ((0, 0, 0.25), 0.05), ((1, 0, 0.5), -1.1), ((0, 0, 0.25), 0.9)])
def test_the_restatements_sample_follows_its_conditional_law(state, rho):
    a, b, t = state
    lh, la, n, G = 1.6, 1.1, 200_000, 12
    rs = np.random.RandomState(3)
    x, y, _ = LR.sample_conditional(np.full(n, lh), np.full(n, la), np.full(n, rho), np.full(n, a), np.full(n, b),
                                    np.full(n, 1.0 - t), rs.uniform(size=n), rs.uniform(size=n))
    assert x.min() >= a and y.min() >= b
    check_frequencies(x, y, LR.conditional_pmf(lh, la, rho, a, b, t, G), n)


def check_frequencies(x, y, p, n):
    """Scoreline frequencies within 5 binomial standard deviations of the exact probabilities `p` [G+1, G+1], on the
    cells with expectation >= 50 (shared with tests/test_gpu_live.py)."""
    G = p.shape[0] - 1
    inside = (x <= G) & (y <= G)
    counts = np.bincount(x[inside].astype(np.int64) * (G + 1) + y[inside].astype(np.int64),
                         minlength=(G + 1) ** 2).reshape(G + 1, G + 1)
    cells = n * p >= 50
    assert cells.sum() >= 8
    bad = cells & (np.abs(counts - n * p) > 5 * np.sqrt(n * p * (1 - p)))
    assert not bad.any(), (np.argwhere(bad), counts[bad], (n * p)[bad])


# ---- the weights, the scan and the resampling
def test_scan_association_and_summaries():
    rs = np.random.RandomState(1)
    for S in (1, 2, 255, 256, 257, 1000, 5000):
        L, L0 = rs.normal(0, 3, S), rs.normal(-10, 2, S)
        w = LR.weights(L, L0)
        om = np.exp(L - L.max())
        assert np.all(np.diff(w["C"]) >= 0) and w["C"][-1] == w["W"]
        np.testing.assert_allclose(w["C"], np.cumsum(om), rtol=1e-13)
        np.testing.assert_allclose(w["ess"], om.sum() ** 2 / (om ** 2).sum(), rtol=1e-12)
        np.testing.assert_allclose(w["log_evidence"], np.log(np.mean(np.exp(L0))), rtol=1e-12)
    w = LR.weights(np.zeros(7), np.zeros(7))
    assert w["ess"] == 7.0 and w["log_evidence"] == 0.0


@pytest.mark.parametrize("S,N", [(257, 4096), (1000, 999), (3, 10), (64, 64)])
def test_systematic_resampling_counts_are_floor_or_ceil(S, N):
    rs = np.random.RandomState(S)
    L = rs.normal(0, 2.0, S)
    L[rs.randint(0, S)] = -1e4            # one draw of weight exactly 0
    w = LR.weights(L, np.zeros(S))
    assert (w["omega"] == 0).sum() == 1
    s, _ = LR.resample(w["C"], N, _prng_key(5))
    assert np.all(np.diff(s) >= 0)
    used = np.bincount(s, minlength=S)
    expect = N * w["omega"] / w["W"]
    # (1e-9: a target within that of a C[s] may fall either side; far below the spacing of these weights)
    assert np.all(used >= np.floor(expect - 1e-9)) and np.all(used <= np.ceil(expect + 1e-9)), (used, expect)
    assert used[w["omega"] == 0].sum() == 0


def test_all_mass_on_one_draw_and_constant_weights():
    S, N = 257, 4096
    L = np.full(S, -1e4)
    L[100] = 0.0
    s, _ = LR.resample(LR.weights(L, np.zeros(S))["C"], N, _prng_key(9))
    assert (s == 100).all()
    s, _ = LR.resample(LR.weights(np.full(S, 3.5), np.zeros(S))["C"], N, _prng_key(9))
    used = np.bincount(s, minlength=S)
    assert used.min() >= N // S and used.max() <= -(-N // S)


# ---- the configurations of tests/test_gpu_live.py: the restatement alone flags at most 1 % of the simulations
@pytest.mark.parametrize("kind", LC.KINDS)
@pytest.mark.parametrize("with_log_weights", [False, True])
def test_flag_share_of_the_gpu_configurations(kind, with_log_weights):
    m, ref = LC.restatement(kind, with_log_weights, "overall")
    flagged = int(ref["flagged"].sum())
    print(f"{kind} log_weights={with_log_weights}: flagged {flagged} of {LC.N}, ess {ref['ess']:.1f}")
    assert flagged <= 0.01 * LC.N
    assert 1.0 < ref["ess"] < LC.S and np.isfinite(ref["log_evidence"])
    # every in-play final score is at or beyond its state, and t = 0.999 (rates <= 3) all but freezes the score
    hg, ag = ref["in_play_home_goals"], ref["in_play_away_goals"]
    for i, (a, b, _) in enumerate(LC.STATES):
        assert hg[:, i].min() >= a and ag[:, i].min() >= b
    assert np.mean((hg[:, 5] == 0) & (ag[:, 5] == 3)) >= 0.99
    # the draws used are those of systematic resampling on the restatement's own weights
    used = np.bincount(ref["draw"], minlength=LC.S)
    expect = LC.N * ref["weights"]["omega"] / ref["weights"]["W"]
    assert np.all(used >= np.floor(expect - 1e-6)) and np.all(used <= np.ceil(expect + 1e-6))
    # the same simulations, head to head: the scores and draws are the same, only the ranking may differ
    _, h2h = LC.restatement(kind, with_log_weights, "head_to_head")
    for key in ("draw", "home_goals", "in_play_home_goals", "in_play_away_goals", "points", "flagged"):
        np.testing.assert_array_equal(ref[key], h2h[key], err_msg=key)


# ---- the public method through a stand-in context
class StandInCtx:
    """TEST-ONLY stand-in for HipContext.simulate_season_live: records the call and answers with arrays of the
    documented shapes and dtypes (tests/fake_ctx.py is left as it is)."""

    def __init__(self, draws):
        self.calls, self.draws = [], draws

    def simulate_season_live(self, home_idx, away_idx, table_idx, table, points, n_sims, key, in_play=None,
                             reweight=True, log_weights=None, return_tables=False, return_scores=False,
                             return_weights=False, pair_init=None, head_to_head=False):
        self.calls.append(dict(home_idx=np.array(home_idx), away_idx=np.array(away_idx), in_play=in_play,
                               reweight=reweight, log_weights=log_weights, head_to_head=head_to_head,
                               pair_init=pair_init, table_idx=np.array(table_idx)))
        n, nf, L = len(table_idx), len(home_idx), len(in_play[0])
        out = {"counts": np.full((n, n), n_sims // n, dtype=np.uint64), "points_sum": np.zeros(n, dtype=np.int64),
               "gd_sum": np.zeros(n, dtype=np.int64), "ess": 3.5, "log_evidence": -7.25}
        if return_tables:
            out.update(points=np.zeros((n_sims, n), np.int32), position=np.zeros((n_sims, n), np.uint8),
                       draw=np.zeros(n_sims, np.int32))
        if return_scores:
            out.update(home_goals=np.zeros((n_sims, nf), np.uint8), away_goals=np.zeros((n_sims, nf), np.uint8),
                       in_play_home_goals=np.zeros((n_sims, L), np.uint8),
                       in_play_away_goals=np.zeros((n_sims, L), np.uint8))
        if return_weights:
            out.update(L=np.arange(self.draws, dtype=np.float64), L0=np.zeros(self.draws))
        return out

    def simulate_season(self, *args, **kwargs):
        raise AssertionError("the plain entry point was called for a live request")


def _with_stand_in(m):
    ctx = StandInCtx(m.attack.shape[0])
    m._device = lambda: ctx
    return ctx


def test_result_keys_shapes_and_dtypes():
    m = hand_posterior()
    ctx = _with_stand_in(m)
    S, N = m.attack.shape[0], 12
    ip = {"home_team": ["t04", "t05"], "away_team": ["t00", "t06"], "home_goals": [1, 0], "away_goals": [0, 0],
          "elapsed": [0.4, 0.0]}
    res = m.simulate_season(["t00", "t01", "t02"], ["t01", "t02", "t00"], num_simulations=N, random_state=1, in_play=ip,
                            log_weights=np.zeros(S), return_tables=True, return_scores=True, return_weights=True,
                            tiebreak="head_to_head")
    assert list(res["teams"]) == ["t00", "t01", "t02", "t04", "t05", "t06"]   # the in-play teams are table rows
    n = 6
    want = {"teams": (n,), "position_proba": (n, n), "expected_points": (n,), "expected_goal_difference": (n,),
            "points": (N, n), "position": (N, n), "draw": (N,), "home_goals": (N, 3), "away_goals": (N, 3),
            "in_play_home_goals": (N, 2), "in_play_away_goals": (N, 2), "log_weights": (S,)}
    assert set(res) == set(want) | {"ess", "log_evidence"}
    for key, shape in want.items():
        assert res[key].shape == shape, key
    assert res["draw"].dtype == np.int32 and res["in_play_home_goals"].dtype == np.uint8
    assert res["log_weights"].dtype == np.float64 and res["log_weights"].max() == 0.0
    np.testing.assert_array_equal(res["log_weights"], np.arange(S) - (S - 1.0))
    assert isinstance(res["ess"], float) and res["ess"] == 3.5 and res["log_evidence"] == -7.25
    call = ctx.calls[0]
    np.testing.assert_array_equal(call["home_idx"], [0, 1, 2])
    np.testing.assert_array_equal(call["in_play"][0], [4, 5])
    np.testing.assert_array_equal(call["in_play"][2], [1, 0])
    assert call["in_play"][2].dtype == np.uint8 and call["in_play"][4].dtype == np.float64
    assert call["head_to_head"] is True and call["pair_init"].shape == (n, n)
    # log_weights alone, and an empty in_play, go the same way; the minimal result has the two new floats only
    res = m.simulate_season(["t00"], ["t01"], num_simulations=N, random_state=1, log_weights=np.zeros(S))
    assert set(res) == {"teams", "position_proba", "expected_points", "expected_goal_difference", "ess", "log_evidence"}
    empty = {k: [] for k in ip}
    res = m.simulate_season(["t00"], ["t01"], num_simulations=N, random_state=1, in_play=empty, return_scores=True)
    assert res["in_play_home_goals"].shape == (N, 0) and len(ctx.calls) == 3 and ctx.calls[2]["log_weights"] is None


def test_the_pair_bound_counts_in_play_matches_as_meetings():
    m = hand_posterior()
    _with_stand_in(m)
    played = {"home_team": ["t00"], "away_team": ["t01"], "home_goals": [65535 - 255], "away_goals": [0]}
    ip = {"home_team": ["t01"], "away_team": ["t00"], "home_goals": [0], "away_goals": [0], "elapsed": [0.1]}
    kw = dict(num_simulations=5, random_state=1, tiebreak="head_to_head", played=played,
              current_table={"t00": (3, 9, 0), "t01": (0, 0, 9)})
    m.simulate_season([], [], in_play=ip, **kw)                       # one meeting to come: 255 more goals still fit
    with pytest.raises(ValueError, match="16 bits"):
        m.simulate_season(["t00"], ["t01"], in_play=ip, **kw)         # two


def test_every_argument_check_runs_before_a_context_is_touched():
    m = hand_posterior()
    S = m.attack.shape[0]
    good = {"home_team": ["t04"], "away_team": ["t05"], "home_goals": [1], "away_goals": [0], "elapsed": [0.4]}

    def bad(in_play=good, home=("t00",), away=("t01",), **kw):
        with pytest.raises(ValueError):
            m.simulate_season(list(home), list(away), num_simulations=10, random_state=1, in_play=in_play, **kw)
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
    with pytest.raises(ValueError, match="not supported together"):
        m.simulate_season(["t00"], ["t01"], in_play=good, playoffs={"bracket": [0, 1]})
    with pytest.raises(ValueError, match="not supported together"):
        m.simulate_season(["t00"], ["t01"], log_weights=np.zeros(S), playoffs={"bracket": [0, 1]})
    # F + L beyond the fixture bound
    F = SEASON_MAX_FIXTURES
    with pytest.raises(ValueError, match="fixtures"):
        m.simulate_season(np.zeros(F, np.uint16), np.ones(F, np.uint16), num_simulations=10, in_play=good)
    assert m._predict_ctx is None
