"""season_trajectory on the device (csrc/dc_trajectory.hip.h) against simulate_season: under one random_state
simulation j here is simulation j there, so the eight count tables must equal, integer for integer, the numpy
restatement (tests/trajectory_ref.py) that rebuilds and re-ranks the table after every matchday from
simulate_season's per-simulation scorelines.  Every comparison is of integers, and every derived float is formed from
the same integers on both sides: compared exactly.

(The scorelines of a fixture are keyed by its place in the list given, so the same fixtures in another order are
another set of simulations: "labels in shuffled fixture order" is checked against the reference on the SAME list,
against the same list under order-preserving relabelling, and in its last row against simulate_season.)"""
import numpy as np
import pytest

import leverage_ref as L
import trajectory_ref as R
from bpl import DixonColesMatchPredictor, ExtendedDixonColesMatchPredictor
from bpl._ffi import BPLHIP_EINVAL, BPLHIP_ESTATE, BplHipError, HipContext, prng_key
from bpl.base import LEVERAGE_TARGETS, TRAJECTORY_MAX_ROUNDS, leverage_targets, trajectory_axis, trajectory_rounds

pytestmark = pytest.mark.gpu

EIGHT = {"title": (0,), "top_two": (0, 1), "top_half": range(0, 32), "odd": range(1, 64, 2), "last": (-1,),
         "bottom_three": (-3, -2, -1), "all": range(64), "second": (1,)}
TABLES = ("position_count", "target_count", "target_final_count", "points_sum", "points_sq_sum",
          "rounds_inside_count", "secured_count", "lead_changes_count")
RAW = ("position", "target", "target_final", "points_sum", "points_sq_sum", "rounds_inside", "secured", "lead_changes")


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


def _sizes(sizes):
    """Sorted labels: matchday i has sizes[i] fixtures."""
    return np.repeat(np.arange(len(sizes)), sizes)


def _season_paths(m, h, a, md, N, seed, **kw):
    """The yardstick's per-simulation part: simulate_season's scorelines, re-ranked after every matchday in numpy."""
    season = m.simulate_season(h, a, num_simulations=N, random_state=seed, return_tables=True, return_scores=True, **kw)
    hh, aa, table_idx, table, points, _, h2h, pair = m._season_h2h_inputs(
        h, a, N, kw.get("current_table"), kw.get("teams"), kw.get("points", (3, 1, 0)), kw.get("tiebreak", "overall"),
        kw.get("played"))
    slot = {int(t): i for i, t in enumerate(table_idx)}
    days, pos, pts = R.paths([slot[int(v)] for v in hh], [slot[int(v)] for v in aa], md, season["home_goals"],
                             season["away_goals"], table, points, prng_key(seed), h2h, pair)
    # the yardstick itself ends on simulate_season's table
    np.testing.assert_array_equal(pos[:, -1], season["position"])
    np.testing.assert_array_equal(pts[:, -1], season["points"])
    return season, days, pos, pts


def _assert_equal(res, days, pos, pts, targets):
    n = pos.shape[2]
    want = R.counts(pos, pts, L.target_masks(LEVERAGE_TARGETS if targets is None else targets, n))
    np.testing.assert_array_equal(res["matchdays"], days)
    for key in TABLES:
        assert res[key].dtype == np.int64 and res[key].shape == want[key].shape, (key, res[key].shape, want[key].shape)
        np.testing.assert_array_equal(res[key], want[key], err_msg=key)
    return want


def _assert_identity(m, h, a, md, N, seed=1234, targets=None, **kw):
    season, days, pos, pts = _season_paths(m, h, a, md, N, seed, **kw)
    res = m.season_trajectory(h, a, md, num_simulations=N, random_state=seed, targets=targets, **kw)
    assert list(res["teams"]) == list(season["teams"])
    _assert_equal(res, days, pos, pts, targets)
    return res, season


def _assert_conserved(res, N):
    R_, n, K = res["target_count"].shape
    np.testing.assert_array_equal(res["position_count"].sum(axis=2), N)
    np.testing.assert_array_equal(res["position_count"].sum(axis=1), N)
    np.testing.assert_array_equal(res["rounds_inside_count"].sum(axis=-1), N)
    np.testing.assert_array_equal(res["secured_count"].sum(axis=-1), N)
    assert res["lead_changes_count"].sum() == N and res["lead_changes_count"].shape == (R_,)
    assert (res["target_final_count"] <= res["target_count"]).all()
    np.testing.assert_array_equal(res["target_final_count"][-1], res["target_count"][-1])
    np.testing.assert_array_equal(res["secured_count"][..., R_], N - res["target_count"][-1])
    np.testing.assert_array_equal(res["rounds_inside_count"] @ np.arange(R_ + 1), res["target_count"].sum(axis=0))
    np.testing.assert_array_equal(res["secured_by_proba"][..., -1], res["target_proba"][-1])


def _position_counts(position, n):
    out = np.zeros((n, n), dtype=np.int64)
    np.add.at(out, (np.broadcast_to(np.arange(n), position.shape), position.astype(np.int64)), 1)
    return out


# ---------------------------------------------------------------- 1. identity with the season kernel
@pytest.mark.parametrize("kind", ["basic", "extended", "clipped"])
def test_tables_are_the_season_kernels(kind):
    m = _posterior(kind)
    h, a = _round_robin(20)
    md = np.random.RandomState(11).permutation(380) // 10          # 38 matchdays of 10
    table = _table(m)
    N = 3000
    res, season = _assert_identity(m, h, a, md, N, current_table=table)
    assert res["position_count"].shape == (38, 20, 20) and list(res["targets"]) == ["title", "top_four", "relegation"]
    np.testing.assert_array_equal(res["position_count"][-1], _position_counts(season["position"], 20))
    np.testing.assert_array_equal(res["position_proba"][-1], season["position_proba"])
    need = m.points_needed(h, a, num_simulations=N, random_state=1234, current_table=table)
    lev = m.match_leverage(h, a, num_simulations=N, random_state=1234, current_table=table)
    np.testing.assert_array_equal(res["target_count"][-1], need["target_count"])
    np.testing.assert_array_equal(res["target_count"][-1], lev["target_count"])
    np.testing.assert_array_equal(res["points_sum"][-1], need["team_points_count"] @ need["points"])
    _assert_conserved(res, N)
    # the derived floats: formed from the same integers, cell by cell
    small = {k: res[k][:, :3] for k in TABLES[:5]}
    small.update({k: res[k][:3] for k in TABLES[5:7]}, lead_changes_count=res["lead_changes_count"])
    small["position_count"] = small["position_count"][:, :, :3]
    for key, want in R.derived(small, N).items():
        got = res[key]
        if key == "position_proba":
            got = got[:, :3, :3]
        elif key in ("expected_rounds_inside", "secured_by_proba"):
            got = got[:3]
        elif key != "expected_lead_changes":
            got = got[:, :3]
        np.testing.assert_array_equal(got, want, err_msg=key)


# ---------------------------------------------------------------- 2. the 64-lane window
@pytest.mark.parametrize("sizes", [[1, 63, 64, 65, 1], [3, 130, 5], [40], [1] * 70, [10] * 12 + [9]],
                         ids=["1-63-64-65-1", "130-over-three-windows", "one-matchday", "a-matchday-each", "tens-of-129"])
def test_matchdays_around_the_window_of_64(sizes):
    F = int(np.sum(sizes))
    m = _posterior("basic", T=12, S=16, seed=F)
    h, a = _pairings(12, F, seed=F)
    res, season = _assert_identity(m, h, a, _sizes(sizes), 300, seed=F, teams=list(m.teams))
    _assert_conserved(res, 300)
    if len(sizes) == 1:                                             # everything collapses onto simulate_season
        np.testing.assert_array_equal(res["position_count"][0], _position_counts(season["position"], 12))
        np.testing.assert_array_equal(res["lead_changes_count"], [300])
        np.testing.assert_array_equal(res["points_sum"][0], season["points"].sum(axis=0))


# ---------------------------------------------------------------- 3. labels
def test_negative_sparse_labels_in_shuffled_order():
    m = _posterior("extended", T=10, S=16, seed=3)
    h, a = _round_robin(10)                                         # 90 fixtures
    rs = np.random.RandomState(5)
    values = np.array([-1000, -7, -1, 0, 3, 4, 90, 2 ** 40, 2 ** 62])
    md = values[rs.randint(0, values.size, 90)]
    N = 400
    res, season = _assert_identity(m, h, a, md, N, seed=9, current_table=_table(m))
    np.testing.assert_array_equal(res["matchdays"], np.unique(md))
    # the labels' order is all that matters: the same list under dense labels, and as a Python list
    dense = m.season_trajectory(h, a, list(np.searchsorted(np.unique(md), md)), num_simulations=N, random_state=9,
                                current_table=_table(m))
    for key in TABLES:
        np.testing.assert_array_equal(dense[key], res[key], err_msg=key)
    # the last row is simulate_season's whatever the labels: a fixture keeps the random block of its place in the list
    np.testing.assert_array_equal(res["position_count"][-1], _position_counts(season["position"], 10))
    ordered = m.season_trajectory(h, a, np.arange(90) // 9, num_simulations=N, random_state=9, current_table=_table(m))
    np.testing.assert_array_equal(ordered["position_count"][-1], res["position_count"][-1])
    np.testing.assert_array_equal(ordered["points_sum"][-1], res["points_sum"][-1])
    np.testing.assert_array_equal(ordered["points_sq_sum"][-1], res["points_sq_sum"][-1])


def test_256_matchdays_and_one_more():
    m = _posterior("basic", T=4, S=8, seed=4)
    h, a = _pairings(4, 256, seed=4)
    res, _ = _assert_identity(m, h, a, np.arange(256)[::-1].copy(), 100, seed=4)
    assert res["position_count"].shape == (TRAJECTORY_MAX_ROUNDS, 4, 4) and res["secured_count"].shape == (4, 3, 257)
    _assert_conserved(res, 100)
    m._predict_ctx.close()
    m._predict_ctx = None
    h2, a2 = _pairings(4, 257, seed=4)
    for hh, aa, md in ((h2, a2, np.arange(257)), (h, a, np.arange(256.0)), (h, a, np.arange(255)),
                       (h, a, np.arange(256) > 7), (h, a, [True] * 256), (h[:0], a[:0], [])):
        with pytest.raises(ValueError):
            m.season_trajectory(hh, aa, md, num_simulations=100)
        assert m._predict_ctx is None                               # raised before any device call


# ---------------------------------------------------------------- 4. table sizes and target counts
@pytest.mark.parametrize("n,F", [(2, 13), (3, 26), (64, 130)])
def test_table_sizes_with_one_and_eight_targets(n, F):
    m = _posterior("extended", T=n, S=8, seed=n)
    h, a = _pairings(n, F, seed=n)
    md = np.random.RandomState(n).randint(0, 13, F)
    N = 300
    kw = dict(teams=list(m.teams))
    _, days, pos, pts = _season_paths(m, h, a, md, N, n, **kw)
    for targets in ({"top": (0,)}, EIGHT):
        res = m.season_trajectory(h, a, md, num_simulations=N, random_state=n, targets=targets, **kw)
        _assert_equal(res, days, pos, pts, targets)
        _assert_conserved(res, N)
    assert res["target_count"].shape == (days.size, n, 8)
    np.testing.assert_array_equal(res["target_count"][:, :, 6], N)                       # "all"
    np.testing.assert_array_equal(res["rounds_inside_count"][:, 6, :-1], 0)
    np.testing.assert_array_equal(res["secured_count"][:, 6, 0], N)


# ---------------------------------------------------------------- 5. simulation counts
@pytest.mark.parametrize("N,S", [(1, 64), (7, 64), (257, 64), (4097, 64), (257, 1)])
def test_simulation_counts(N, S):
    m = _posterior("basic", T=8, S=S, seed=N)
    h, a = _pairings(8, 40, seed=N)
    res, _ = _assert_identity(m, h, a, np.arange(40) % 5, N, seed=N)
    _assert_conserved(res, N)


# ---------------------------------------------------------------- 6. conservation
def test_conservation_on_the_device_output():
    m = _posterior("extended", seed=2)
    h, a = _round_robin(20)
    N = 2000
    res = m.season_trajectory(h, a, np.arange(380) // 10, num_simulations=N, random_state=42, current_table=_table(m, 4),
                              targets={"all": range(64), "title": (0,), "bottom_three": (-3, -2, -1)})
    _assert_conserved(res, N)
    np.testing.assert_array_equal(res["target_count"][:, :, 0], N)
    np.testing.assert_array_equal(res["target_count"][:, :, 1].sum(axis=1), N)
    np.testing.assert_array_equal(res["target_count"][:, :, 2].sum(axis=1), 3 * N)
    assert res["lead_changes_count"][1:].sum() > 0
    one = m.season_trajectory(h, a, np.zeros(380, dtype=np.int32), num_simulations=N, random_state=42)
    _assert_conserved(one, N)
    np.testing.assert_array_equal(one["lead_changes_count"], [N])


# ---------------------------------------------------------------- 7. chunking
def test_chunking_changes_nothing():
    m = _posterior("basic", T=14, S=32, seed=8)
    h, a = _pairings(14, 65, seed=8)
    md = np.random.RandomState(8).randint(0, 7, 65)
    N, seed = 1000, 77
    hh, aa, table_idx, table, points, n_sims = m._season_inputs(h, a, N, _table(m), None, (3, 1, 0))
    _, masks = leverage_targets(None, table_idx.size)
    slot = np.full(len(m.teams), -1)
    slot[table_idx.astype(int)] = np.arange(table_idx.size)
    points_min, P = trajectory_axis(table[:, 0], slot[hh], slot[aa], points)
    days, fix_id, round_end = trajectory_rounds(md, 65)
    assert days.size == 7
    _, _, pos, pts = _season_paths(m, h, a, md, N, seed, current_table=_table(m))
    want = R.counts(pos, pts, L.target_masks(LEVERAGE_TARGETS, table_idx.size))
    ctx = m._device()
    call = lambda chunk: ctx.season_trajectory(hh, aa, table_idx, table, points, n_sims, prng_key(seed), masks,
                                               points_min, P, fix_id, round_end, chunk_sims=chunk)
    whole = call(0)
    for raw, key in zip(RAW, TABLES):
        ref = want[key]
        if key == "points_sum":
            ref = ref - N * points_min
        elif key == "points_sq_sum":
            ref = ref - 2 * points_min * want["points_sum"] + N * points_min * points_min
        np.testing.assert_array_equal(whole[raw].astype(np.int64), ref, err_msg=key)
    for chunk in (1, 64, 100, 4096):
        got = call(chunk)
        for key in whole:
            np.testing.assert_array_equal(got[key], whole[key], err_msg=f"{key} at chunk_sims={chunk}")


# ---------------------------------------------------------------- 8. head to head
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
    md = np.random.RandomState(n).randint(0, 8, h.size)
    played = _half_season(m, seed=n + 1)
    N = 300
    res, _ = _assert_identity(m, h, a, md, N, seed=n, tiebreak="head_to_head", played=played)
    _assert_conserved(res, N)
    overall = m.season_trajectory(h, a, md, num_simulations=N, random_state=n, played=played)
    np.testing.assert_array_equal(res["points_sum"], overall["points_sum"])              # the order alone differs
    np.testing.assert_array_equal(res["points_sq_sum"], overall["points_sq_sum"])
    assert not np.array_equal(res["position_count"], overall["position_count"])
    # no points at all and a level table: the head-to-head and goal keys alone move the leader
    level, _ = _assert_identity(m, h, a, md, N, seed=n, tiebreak="head_to_head", played=played, points=(0, 0, 0),
                                current_table={t: (5, 0, 0) for t in m.teams})
    np.testing.assert_array_equal(level["points_sum"], 5 * N)
    np.testing.assert_array_equal(level["points_sd"], 0.0)
    assert level["lead_changes_count"][1:].sum() > 0


# ---------------------------------------------------------------- 9. errors
def test_context_state_and_argument_errors():
    ctx = HipContext(0)
    try:
        # two fixtures of slots 0 and 1, two matchdays; totals run from 0 to 6 points
        args = ([0, 1], [1, 0], [0, 1], np.zeros((2, 3)), (3, 1, 0), 10, (0, 1), [1], 0, 7)
        good = ([0, 1], [1, 2])

        def refused(code, *a, **kw):
            with pytest.raises(BplHipError) as e:
                ctx.season_trajectory(*a, **kw)
            assert e.value.code == code, (a, kw)

        refused(BPLHIP_ESTATE, *args, *good)
        S, T = 4, 3
        ctx.predict_set_posterior_venue(*[np.zeros((S, T)) for _ in range(6)], np.zeros(S))
        refused(BPLHIP_ESTATE, *args, *good)
        ctx.predict_set_posterior(np.zeros((S, T)), np.zeros((S, T)), np.zeros(S), np.zeros(S))
        refused(BPLHIP_EINVAL, *args, [0, 1], [])                                        # R = 0
        refused(BPLHIP_EINVAL, *args, [0, 1], [0] * 256 + [2])                           # R = 257
        refused(BPLHIP_EINVAL, *args, [0, 1], [2, 1])                                    # decreasing
        refused(BPLHIP_EINVAL, *args, [0, 1], [-1, 2])                                   # below the fixtures
        refused(BPLHIP_EINVAL, *args, [0, 1], [1, 1])                                    # does not end at n_fixtures
        refused(BPLHIP_EINVAL, *args, [0, 1], [1, 3])                                    # ends past them
        for ids in ([0, 0], [1, 2], [-1, 0]):                                            # not a permutation
            refused(BPLHIP_EINVAL, *args, ids, [1, 2])
        for masks in ([], [1] * 9, [1, 0], [0b100]):      # K = 0, K = 9, a zero mask, a position outside the table
            refused(BPLHIP_EINVAL, *args[:7], masks, 0, 7, *good)
        # the axis a total on the way could leave: too few bins, a floor above the current totals, more than the bound
        for points_min, n_bins in ((0, 6), (1, 7), (0, 0), (0, 1025)):
            refused(BPLHIP_EINVAL, *args[:8], points_min, n_bins, *good)
        refused(BPLHIP_EINVAL, *args, *good, chunk_sims=-1)
        out = ctx.season_trajectory(*args, *good)                 # and the context stays usable; a wider axis is fine too
        assert out["position"].shape == (2, 2, 2) and out["position"].sum() == 40 and out["lead_changes"].sum() == 10
        wide = ctx.season_trajectory(*args[:8], -2, 12, *good)
        np.testing.assert_array_equal(wide["position"], out["position"])
        np.testing.assert_array_equal(wide["points_sum"], out["points_sum"] + 2 * 10)
        empty = ctx.season_trajectory(*args, [0, 1], [0, 2])      # an empty matchday repeats the table before it
        np.testing.assert_array_equal(empty["position"][1], out["position"][1])
        np.testing.assert_array_equal(empty["points_sum"][0], 0)                         # the current table itself
        np.testing.assert_array_equal(empty["position"][0].sum(axis=1), 10)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 10. determinism
def test_reproducible_and_the_context_stays_usable():
    m = _posterior("extended", T=10, S=16, seed=6)
    h, a = _round_robin(10)
    md = np.arange(90) // 5
    kw = dict(num_simulations=1500, current_table=_table(m, 9))
    before = m.simulate_season(h, a, random_state=21, return_tables=True, **kw)
    r1 = m.season_trajectory(h, a, md, random_state=21, **kw)
    r2 = m.season_trajectory(h, a, md, random_state=21, **kw)
    r3 = m.season_trajectory(h, a, md, random_state=22, **kw)
    for key in r1:
        np.testing.assert_array_equal(r1[key], r2[key], err_msg=key)
    assert not np.array_equal(r1["position_count"], r3["position_count"])
    after = m.simulate_season(h, a, random_state=21, return_tables=True, **kw)
    for key in before:
        np.testing.assert_array_equal(before[key], after[key], err_msg=key)
