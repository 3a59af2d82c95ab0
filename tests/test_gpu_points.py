"""points_needed on the device (csrc/dc_points.hip.h) against simulate_season: under one random_state simulation
j here is simulation j there, so the four count tables must equal, integer for integer, the numpy cross-tabulation
(tests/points_ref.py) of simulate_season's per-simulation points and positions.  Every comparison is of integers,
and every derived float is one operation on the same integers on both sides: compared exactly."""
import numpy as np
import pytest

import leverage_ref as L
import points_ref as R
from bpl import DixonColesMatchPredictor, ExtendedDixonColesMatchPredictor
from bpl._ffi import BPLHIP_EINVAL, BPLHIP_ESTATE, BplHipError, HipContext, prng_key
from bpl.base import LEVERAGE_TARGETS, leverage_targets, points_axis

pytestmark = pytest.mark.gpu

EIGHT = {"title": (0,), "top_two": (0, 1), "top_half": range(0, 32), "odd": range(1, 64, 2), "last": (-1,),
         "bottom_three": (-3, -2, -1), "all": range(64), "second": (1,)}
TABLES = ("team_points_count", "team_target_count", "position_points_count", "gap_count")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _model(cls, attack, defence, home_advantage, corr_coef):
    m = cls()
    T = attack.shape[1]
    m.teams = np.array([f"t{i:02d}" for i in range(T)])
    m._teams_dict = {t: i for i, t in enumerate(m.teams)}
    m.attack, m.defence = np.asarray(attack, float), np.asarray(defence, float)
    m.home_advantage, m.corr_coef = np.asarray(home_advantage, float), np.asarray(corr_coef, float)
    return m


def _round_robin(T):
    h, a = np.nonzero(~np.eye(T, dtype=bool))
    return h.astype(np.uint16), a.astype(np.uint16)


def _pairings(T, F, seed):
    rs = np.random.RandomState(seed)
    h = rs.randint(0, T, F)
    a = (h + rs.randint(1, T, F)) % T
    return h.astype(np.uint16), a.astype(np.uint16)


def _posterior(kind, T=20, S=64, seed=0):
    rs = np.random.RandomState(seed)
    att, dfn = rs.normal(0, 0.3, (S, T)), rs.normal(0, 0.3, (S, T))
    if kind == "extended":
        return _model(ExtendedDixonColesMatchPredictor, att, dfn, rs.normal(0.25, 0.1, (S, T)), rs.uniform(-0.1, 0.1, S))
    m = _model(DixonColesMatchPredictor, att, dfn, rs.normal(0.25, 0.05, S), rs.uniform(-0.1, 0.1, S))
    if kind == "clipped":   # tau clips for some pairs: rho beyond the bounds in both directions
        m.corr_coef = np.where(np.arange(S) % 2 == 0, 0.9, -1.1)
    return m


def _table(m, seed=3):
    rs = np.random.RandomState(seed)
    return {t: (int(rs.randint(0, 60)), int(rs.randint(0, 70)), int(rs.randint(0, 70))) for t in m.teams[::2]}


def _season_tables(m, h, a, N, seed, targets=None, **kw):
    """The yardstick: simulate_season's per-simulation points and positions, cross-tabulated in numpy on the axis
    restated from the table the season ran on."""
    season = m.simulate_season(h, a, num_simulations=N, random_state=seed, return_tables=True, **kw)
    n = len(season["teams"])
    inside = L.target_masks(LEVERAGE_TARGETS if targets is None else targets, n)
    args = m._season_h2h_inputs(h, a, N, kw.get("current_table"), kw.get("teams"), kw.get("points", (3, 1, 0)),
                                kw.get("tiebreak", "overall"), kw.get("played"))
    hh, aa, table_idx, table, points = args[:5]
    slot = {int(t): i for i, t in enumerate(table_idx)}
    points_min, P = R.axis(table[:, 0], [slot[int(v)] for v in hh], [slot[int(v)] for v in aa], points)
    return season, points_min, R.counts(season["points"], season["position"], inside, points_min, P)


def _assert_identity(m, h, a, N, seed=1234, targets=None, **kw):
    season, points_min, want = _season_tables(m, h, a, N, seed, targets, **kw)
    res = m.points_needed(h, a, num_simulations=N, random_state=seed, targets=targets, **kw)
    assert list(res["teams"]) == list(season["teams"])
    np.testing.assert_array_equal(res["points"], points_min + np.arange(want[0].shape[1]))
    for key, ref in zip(TABLES, want):
        assert res[key].dtype == np.int64 and res[key].shape == ref.shape, (key, res[key].shape, ref.shape)
        np.testing.assert_array_equal(res[key], ref, err_msg=key)
    return res


def _assert_conserved(res, N):
    for key in ("team_points_count", "position_points_count", "gap_count"):
        np.testing.assert_array_equal(res[key].sum(axis=1), N, err_msg=key)
    np.testing.assert_array_equal(res["team_points_count"].sum(axis=0), res["position_points_count"].sum(axis=0))
    assert (res["team_target_count"] <= res["team_points_count"][:, :, None]).all()


# ---------------------------------------------------------------- 1. identity with the season kernel
@pytest.mark.parametrize("kind", ["basic", "extended", "clipped"])
def test_tables_are_the_season_kernels(kind):
    m = _posterior(kind)
    h, a = _round_robin(20)
    table = _table(m)
    res = _assert_identity(m, h, a, 3000, current_table=table)
    assert res["team_target_count"].shape[::2] == (20, 3) and list(res["targets"]) == ["title", "top_four", "relegation"]
    lev = m.match_leverage(h, a, num_simulations=3000, random_state=1234, current_table=table)
    np.testing.assert_array_equal(res["target_count"], lev["target_count"])
    _assert_conserved(res, 3000)
    # the derived floats: one operation per cell on the same integers, cell by cell
    small = {k: res[k][:3] for k in ("team_points_count", "team_target_count", "position_points_count")}
    ref = R.derived(small["team_points_count"], small["team_target_count"], small["position_points_count"],
                    res["gap_count"][:2], int(res["points"][0]), 3000, res["levels"])
    for key, want in ref.items():
        got = res[key][:, :3] if key == "position_points_quantile" else res[key][:len(want)]
        np.testing.assert_array_equal(got, want, err_msg=key)


# ---------------------------------------------------------------- 2. conservation
def test_conservation_on_the_device_output():
    m = _posterior("extended", seed=2)
    h, a = _round_robin(20)
    N = 2000
    res = m.points_needed(h, a, num_simulations=N, random_state=42, current_table=_table(m, 4),
                          targets={"all": range(64), "title": (0,)})
    _assert_conserved(res, N)
    np.testing.assert_array_equal(res["team_target_count"][:, :, 0], res["team_points_count"])
    np.testing.assert_array_equal(res["target_count"][:, 0], N)
    assert res["target_count"][:, 1].sum() == N and (res["gap_count"][:, 0] > 0).any()


# ---------------------------------------------------------------- 3.-6. shape edges
@pytest.mark.parametrize("F", [1, 63, 64, 65, 129])
def test_fixture_counts_around_the_block_of_64(F):
    m = _posterior("basic", T=12, S=16, seed=F)
    h, a = _pairings(12, F, seed=F)
    _assert_identity(m, h, a, 300, seed=F, teams=list(m.teams))


@pytest.mark.parametrize("n,F", [(2, 3), (3, 6), (64, 130)])
def test_table_sizes(n, F):
    m = _posterior("extended", T=n, S=8, seed=n)
    h, a = _pairings(n, F, seed=n)
    res = _assert_identity(m, h, a, 400, seed=n, teams=list(m.teams))
    assert res["gap_count"].shape[0] == n - 1
    _assert_conserved(res, 400)


def test_a_table_of_one():
    m = _posterior("basic", T=4, S=8, seed=1)
    none = np.zeros(0, dtype=np.uint16)
    res = _assert_identity(m, none, none, 100, teams=["t02"], current_table={"t02": (7, 3, 1)}, targets={"title": (0,)})
    assert res["gap_count"].shape == (0, 1) and res["level_proba"].shape == (0,)
    np.testing.assert_array_equal(res["points"], [7])
    np.testing.assert_array_equal(res["team_points_count"], [[100]])
    np.testing.assert_array_equal(res["team_target_count"], [[[100]]])
    np.testing.assert_array_equal(res["points_needed"], 7.0)


@pytest.mark.parametrize("n", [7, 64])
def test_one_and_eight_overlapping_targets(n):
    m = _posterior("basic", T=n, S=8, seed=n)
    h, a = _pairings(n, 70, seed=n + 1)
    _assert_identity(m, h, a, 300, targets={"top_three": (0, 1, 2)}, teams=list(m.teams))
    res = _assert_identity(m, h, a, 300, targets=EIGHT, teams=list(m.teams))
    assert res["team_target_count"].shape[::2] == (n, 8)
    np.testing.assert_array_equal(res["team_target_count"][:, :, 6], res["team_points_count"])   # "all"


@pytest.mark.parametrize("N,S", [(1, 64), (7, 64), (257, 64), (4097, 64), (257, 1)])
def test_simulation_counts(N, S):
    m = _posterior("basic", T=8, S=S, seed=N)
    h, a = _pairings(8, 40, seed=N)
    res = _assert_identity(m, h, a, N, seed=N)
    _assert_conserved(res, N)


# ---------------------------------------------------------------- 7. the points axis at its edges
def test_an_axis_of_1024_bins_and_one_more():
    m = _posterior("basic", T=3, S=8, seed=7)
    h, a = ["t00", "t01"], ["t01", "t02"]
    table = {"t00": (0, 0, 0), "t02": (1020, 5, 5)}
    res = _assert_identity(m, h, a, 200, current_table=table, targets={"title": (0,), "last": (-1,)})
    assert res["points"].shape == (1024,) and res["points"][-1] == 1023
    np.testing.assert_array_equal(res["target_count"][:, 0], [0, 0, 200])       # 1020 points ahead: always champion
    assert res["target_count"][2, 1] == 0 and res["target_count"][:, 1].sum() == 200
    _assert_conserved(res, 200)
    m._predict_ctx.close()
    m._predict_ctx = None
    with pytest.raises(ValueError):
        m.points_needed(h, a, num_simulations=200, current_table={"t00": (0, 0, 0), "t02": (1021, 5, 5)})
    assert m._predict_ctx is None                                   # raised before any device call


def test_points_that_move_nothing_and_other_points():
    m = _posterior("extended", T=20, S=16, seed=5)
    h, a = _pairings(10, 45, seed=5)                                # teams 0..9 play
    table = _table(m)
    res = _assert_identity(m, h, a, 500, points=(0, 0, 0), current_table=table, teams=list(m.teams))
    current = [table.get(t, (0, 0, 0))[0] for t in m.teams]
    assert res["points"].size == max(current) - min(current) + 1   # the spread of the current table only
    assert (res["team_points_count"].max(axis=1) == 500).all()
    res = _assert_identity(m, h, a, 500, points=(2, 1, 0), current_table=table, teams=list(m.teams))
    _assert_conserved(res, 500)
    _assert_identity(m, h, a, 500, points=(1, 3, 0))


# ---------------------------------------------------------------- 8. chunking
def test_chunking_changes_nothing():
    m = _posterior("basic", T=14, S=32, seed=8)
    h, a = _pairings(14, 65, seed=8)
    N, seed = 1000, 77
    hh, aa, table_idx, table, points, n_sims = m._season_inputs(h, a, N, _table(m), None, (3, 1, 0))
    _, masks = leverage_targets(None, table_idx.size)
    slot = np.full(len(m.teams), -1)
    slot[table_idx.astype(int)] = np.arange(table_idx.size)
    points_min, P = points_axis(table[:, 0], slot[hh], slot[aa], points)
    _, ref_min, want = _season_tables(m, h, a, N, seed, current_table=_table(m))
    assert (points_min, P) == (ref_min, want[0].shape[1])
    ctx = m._device()
    whole = ctx.season_points(hh, aa, table_idx, table, points, n_sims, prng_key(seed), masks, points_min, P, chunk_sims=0)
    for key, ref in zip(("team_points", "team_target", "position_points", "gap"), want):
        np.testing.assert_array_equal(whole[key].astype(np.int64), ref, err_msg=key)
    for chunk in (1, 64, 100, 4096):
        raw = ctx.season_points(hh, aa, table_idx, table, points, n_sims, prng_key(seed), masks, points_min, P,
                                chunk_sims=chunk)
        for key in whole:
            np.testing.assert_array_equal(raw[key], whole[key], err_msg=f"{key} at chunk_sims={chunk}")


# ---------------------------------------------------------------- 9. head to head
def _half_season(m, seed):
    """A single round robin already played: simulate_season's `played`."""
    T = len(m.teams)
    rs = np.random.RandomState(seed)
    h, a = np.nonzero(np.triu(np.ones((T, T), dtype=bool), 1))
    swap = rs.rand(h.size) < 0.5
    h, a = np.where(swap, a, h), np.where(swap, h, a)
    return {"home_team": list(m.teams[h]), "away_team": list(m.teams[a]),
            "home_goals": [int(v) for v in rs.poisson(1.4, h.size)], "away_goals": [int(v) for v in rs.poisson(1.1, h.size)]}


@pytest.mark.parametrize("n", [20, 40, 56])      # (dch::H2H_SMALL_TEAMS = 48: four waves per workgroup up to it, two above)
def test_head_to_head_order(n):
    m = _posterior("extended", T=n, S=16, seed=n)
    h, a = _pairings(n, 6 * n, seed=n)
    played = _half_season(m, seed=n + 1)
    N = 600
    res = _assert_identity(m, h, a, N, seed=n, tiebreak="head_to_head", played=played)
    _assert_conserved(res, N)
    overall = m.points_needed(h, a, num_simulations=N, random_state=n, played=played)
    np.testing.assert_array_equal(res["team_points_count"], overall["team_points_count"])   # the order alone differs
    assert not np.array_equal(res["team_target_count"], overall["team_target_count"])
    level = _assert_identity(m, h, a, N, seed=n, tiebreak="head_to_head", played=played, points=(0, 0, 0),
                             current_table={t: (5, 0, 0) for t in m.teams})
    np.testing.assert_array_equal(level["gap_count"][:, 0], N)
    assert level["points"].tolist() == [5]


# ---------------------------------------------------------------- 10. errors
def test_context_state_and_argument_errors():
    ctx = HipContext(0)
    try:
        args = ([0], [1], [0, 1], np.zeros((2, 3)), (3, 1, 0), 10, (0, 1), [1])
        with pytest.raises(BplHipError) as e:
            ctx.season_points(*args, 0, 4)
        assert e.value.code == BPLHIP_ESTATE
        S, T = 4, 3
        ctx.predict_set_posterior_venue(*[np.zeros((S, T)) for _ in range(6)], np.zeros(S))
        with pytest.raises(BplHipError) as e:
            ctx.season_points(*args, 0, 4)
        assert e.value.code == BPLHIP_ESTATE
        ctx.predict_set_posterior(np.zeros((S, T)), np.zeros((S, T)), np.zeros(S), np.zeros(S))
        # the axis a simulated total could leave: too few bins, a floor above the least total, more than the bound
        for points_min, n_bins in ((0, 3), (1, 4), (0, 0), (0, 1025), (-1, 4)):
            with pytest.raises(BplHipError) as e:
                ctx.season_points(*args, points_min, n_bins)
            assert e.value.code == BPLHIP_EINVAL, (points_min, n_bins)
        with pytest.raises(BplHipError) as e:
            ctx.season_points(*args, 0, 4, chunk_sims=-1)
        assert e.value.code == BPLHIP_EINVAL
        for masks in ([], [1] * 9, [1, 0], [0b100]):          # K = 0, K = 9, a zero mask, a position outside the table
            with pytest.raises(BplHipError) as e:
                ctx.season_points(*args[:-1], masks, 0, 4)
            assert e.value.code == BPLHIP_EINVAL, masks
        out = ctx.season_points(*args, 0, 4)                   # and the context stays usable; a wider axis is fine too
        assert out["team_points"].sum() == 20 and out["gap"].sum() == 10
        wide = ctx.season_points(*args, -2, 8)
        np.testing.assert_array_equal(wide["team_points"][:, 2:6], out["team_points"])
    finally:
        ctx.close()


# ---------------------------------------------------------------- 11. determinism
def test_reproducible_and_the_context_stays_usable():
    m = _posterior("extended", T=10, S=16, seed=6)
    h, a = _round_robin(10)
    kw = dict(num_simulations=1500, current_table=_table(m, 9))
    before = m.simulate_season(h, a, random_state=21, return_tables=True, **kw)
    r1 = m.points_needed(h, a, random_state=21, **kw)
    r2 = m.points_needed(h, a, random_state=21, **kw)
    r3 = m.points_needed(h, a, random_state=22, **kw)
    for key in r1:
        np.testing.assert_array_equal(r1[key], r2[key], err_msg=key)
    assert not np.array_equal(r1["team_points_count"], r3["team_points_count"])
    after = m.simulate_season(h, a, random_state=21, return_tables=True, **kw)
    for key in before:
        np.testing.assert_array_equal(before[key], after[key], err_msg=key)
