"""season_trajectory without a GPU: the matchday labels, the points axis, the derived floats and the argument checks,
all host work (bpl/base.py).  The device is a stand-in in the manner of tests/fake_ctx.py whose counts are
tests/trajectory_ref.py's from fixed per-simulation paths."""
import numpy as np
import pytest

import trajectory_ref as R
from bpl import DixonColesMatchPredictor, ExtendedDixonColesMatchPredictor
from bpl.base import (LEVERAGE_MAX_FIXTURES, POINTS_MAX_BINS, TRAJECTORY_MAX_ROUNDS, trajectory_axis,
                      trajectory_from_counts, trajectory_rounds)
from fake_ctx import FakePredictCtx

RAW = {"position": "position_count", "target": "target_count", "target_final": "target_final_count",
       "points_sum": "points_sum", "points_sq_sum": "points_sq_sum", "rounds_inside": "rounds_inside_count",
       "secured": "secured_count", "lead_changes": "lead_changes_count"}


class TrajectoryCtx(FakePredictCtx):
    """Stands in for bpl._ffi.HipContext: `season_trajectory` cross-tabulates the fixed per-simulation paths it was
    made with under the masks and the axis it is given, and records its arguments."""

    def __init__(self, position, points):
        self.sim_position, self.sim_points = np.asarray(position), np.asarray(points)
        self.calls = []

    def season_trajectory(self, home_idx, away_idx, table_idx, table, points, n_sims, key, target_masks, points_min,
                          n_bins, fix_id, round_end, chunk_sims=0):
        self.calls.append(dict(home=np.asarray(home_idx), away=np.asarray(away_idx), table=np.asarray(table),
                               points=points, n_sims=n_sims, key=key, masks=list(target_masks), points_min=points_min,
                               n_bins=n_bins, fix_id=np.asarray(fix_id), round_end=np.asarray(round_end)))
        n = len(table_idx)
        assert self.sim_position.shape == (n_sims, len(round_end), n)
        inside = np.array([[(int(m) >> p) & 1 for p in range(n)] for m in target_masks], dtype=bool)
        tables = R.counts(self.sim_position, self.sim_points - points_min, inside)      # the device sums v, not points
        return {raw: tables[key].astype(np.uint64) for raw, key in RAW.items()}


def _hand_posterior(cls=DixonColesMatchPredictor, T=6, S=8):
    rs = np.random.RandomState(1)
    m = cls()
    m.teams = np.array([f"t{i:02d}" for i in range(T)])
    m._teams_dict = {t: i for i, t in enumerate(m.teams)}
    m.attack = rs.normal(0, 0.2, (S, T))
    m.defence = rs.normal(0, 0.2, (S, T))
    m.home_advantage = rs.normal(0.2, 0.05, S if cls is DixonColesMatchPredictor else (S, T))
    m.corr_coef = rs.uniform(-0.05, 0.05, S)
    return m


# ---------------------------------------------------------------- the matchday labels
def test_rounds_sort_the_fixtures_stably_by_label():
    days, fix_id, round_end = trajectory_rounds([7, -3, 7, 100, -3, 7], 6)
    np.testing.assert_array_equal(days, [-3, 7, 100])
    np.testing.assert_array_equal(fix_id, [1, 4, 0, 2, 5, 3])          # within a label: the order given
    np.testing.assert_array_equal(round_end, [2, 5, 6])
    assert days.dtype == np.int64 and fix_id.dtype == np.int32 and round_end.dtype == np.int32
    days, fix_id, round_end = trajectory_rounds(np.array([5, 5, 5], dtype=np.uint8), 3)
    assert (list(days), list(fix_id), list(round_end)) == ([5], [0, 1, 2], [3])
    days, fix_id, round_end = trajectory_rounds(np.arange(4)[::-1], 4)
    assert (list(days), list(fix_id), list(round_end)) == ([0, 1, 2, 3], [3, 2, 1, 0], [1, 2, 3, 4])
    days, _, round_end = trajectory_rounds(np.arange(TRAJECTORY_MAX_ROUNDS) * 3 - 50, TRAJECTORY_MAX_ROUNDS)
    assert days.size == 256 and round_end[-1] == 256


@pytest.mark.parametrize("bad,nf", [([0.0, 1.0], 2), (np.array([0.5, 1.0]), 2), ([True, False], 2), ([0, True], 2),
                                    (np.array([True, False]), 2), ([0, 1, 2], 2), ([[0, 1]], 2), ([], 0), (["a", "b"], 2),
                                    ([None, 1], 2), (np.arange(TRAJECTORY_MAX_ROUNDS + 1), TRAJECTORY_MAX_ROUNDS + 1)])
def test_rounds_refuse(bad, nf):
    with pytest.raises(ValueError):
        trajectory_rounds(bad, nf)


def test_the_axis_reaches_down_to_the_current_totals():
    # (2, 1, 1): every match gives at least 1, so points_axis starts at 3 -- on the way slot 0 stands on 0, 1, 2 too
    assert trajectory_axis([0, 10], [0, 0, 0], [1, 1, 1], (2, 1, 1)) == (0, 17)
    assert trajectory_axis([10, 4, 30], [0, 0, 2], [1, 2, 0], (3, 1, 0)) == (4, 33)
    assert trajectory_axis([5, 9, 7, 6], [], [], (3, 1, 0)) == (5, 5)


# ---------------------------------------------------------------- derived quantities
def _hand_paths():
    """Three teams, two matchdays, four simulations: (position, points) [N, R, n].  Team 2 is never top."""
    position = np.array([[[0, 1, 2], [0, 1, 2]], [[1, 0, 2], [0, 1, 2]], [[0, 1, 2], [1, 0, 2]], [[0, 2, 1], [0, 2, 1]]])
    points = np.array([[[3, 1, 0], [6, 2, 0]], [[0, 3, 0], [3, 3, 1]], [[3, 1, 0], [3, 4, 1]], [[3, 0, 1], [6, 0, 2]]])
    return position, points


def test_hand_written_example_cell_by_cell():
    position, points = _hand_paths()
    inside = np.array([[True, False, False], [True, True, True]])        # "top" and "all"
    t = R.counts(position, points, inside)
    np.testing.assert_array_equal(t["position_count"], [[[3, 1, 0], [1, 2, 1], [0, 1, 3]]] * 2)
    np.testing.assert_array_equal(t["target_count"][:, :, 0], [[3, 1, 0], [3, 1, 0]])
    np.testing.assert_array_equal(t["target_final_count"][:, :, 0], [[2, 0, 0], [3, 1, 0]])
    np.testing.assert_array_equal(t["rounds_inside_count"][:, 0], [[0, 2, 2], [2, 2, 0], [4, 0, 0]])
    np.testing.assert_array_equal(t["secured_count"][:, 0], [[2, 1, 1], [0, 1, 3], [0, 0, 4]])
    np.testing.assert_array_equal(t["secured_count"][:, 1], [[4, 0, 0]] * 3)
    np.testing.assert_array_equal(t["lead_changes_count"], [2, 2])
    np.testing.assert_array_equal(t["points_sum"], [[9, 5, 1], [18, 9, 4]])
    np.testing.assert_array_equal(t["points_sq_sum"], [[27, 11, 1], [90, 29, 6]])
    # the device's sums are of v = points + 1 here
    N, low = 4, -1
    got = trajectory_from_counts(t["position_count"], t["target_count"], t["target_final_count"],
                                 t["points_sum"] + N, t["points_sq_sum"] + 2 * t["points_sum"] + N,
                                 t["rounds_inside_count"], t["secured_count"], t["lead_changes_count"], low, N)
    for key in RAW.values():
        assert got[key].dtype == np.int64, key
        np.testing.assert_array_equal(got[key], t[key], err_msg=key)
    np.testing.assert_array_equal(got["position_proba"][0], [[0.75, 0.25, 0.0], [0.25, 0.5, 0.25], [0.0, 0.25, 0.75]])
    np.testing.assert_array_equal(got["target_proba"][:, :, 0], [[0.75, 0.25, 0.0]] * 2)
    np.testing.assert_array_equal(got["target_proba"][:, :, 1], 1.0)
    # a team that is never inside: NaN there and only there; a target nobody is ever outside: NaN throughout
    np.testing.assert_array_equal(got["final_given_inside"][:, :, 0], [[2 / 3, 0.0, np.nan], [1.0, 1.0, np.nan]])
    np.testing.assert_array_equal(got["final_given_inside_se"][:, :, 0],
                                  [[np.sqrt((2 / 3) * (1.0 - 2 / 3) / 3), 0.0, np.nan], [0.0, 0.0, np.nan]])
    np.testing.assert_array_equal(got["final_given_outside"][:, :, 0], [[1.0, 1 / 3, 0.0], [0.0, 0.0, 0.0]])
    np.testing.assert_array_equal(got["final_given_outside_se"][0, :, 0], [0.0, np.sqrt((1 / 3) * (1.0 - 1 / 3) / 3), 0.0])
    np.testing.assert_array_equal(got["final_given_inside"][:, :, 1], 1.0)
    assert np.isnan(got["final_given_outside"][:, :, 1]).all() and np.isnan(got["final_given_outside_se"][:, :, 1]).all()
    np.testing.assert_array_equal(got["points_mean"], [[2.25, 1.25, 0.25], [4.5, 2.25, 1.0]])
    np.testing.assert_array_equal(got["points_sd"], [[np.sqrt(27.0) / 4, np.sqrt(19.0) / 4, np.sqrt(3.0) / 4],
                                                     [1.5, np.sqrt(35.0) / 4, np.sqrt(8.0) / 4]])
    np.testing.assert_array_equal(got["expected_rounds_inside"], [[1.5, 2.0], [0.5, 2.0], [0.0, 2.0]])
    np.testing.assert_array_equal(got["secured_by_proba"][:, 0], [[0.5, 0.75], [0.0, 0.25], [0.0, 0.0]])
    np.testing.assert_array_equal(got["secured_by_proba"][..., -1], got["target_proba"][-1])
    assert got["expected_lead_changes"] == 0.5
    for key, want in R.derived(t, N).items():
        np.testing.assert_array_equal(got[key], want, err_msg=key)     # (NaN == NaN in assert_array_equal)


def test_sums_beyond_64_bits_on_the_way_to_the_deviation():
    # N sum(p^2) passes 2^63 here (sum(p^2) itself does not): 2^31 - 1 simulations all on 60 000 points
    N, p = 2 ** 31 - 1, 60_000
    one = np.ones((1, 1, 1), dtype=np.int64) * N
    got = trajectory_from_counts(one, one, one, [[N * p]], [[N * p * p]], [[[0, N]]], [[[N, 0]]], [N], 0, N)
    assert got["points_mean"][0, 0] == float(p) and got["points_sd"][0, 0] == 0.0


def test_the_method_through_a_stand_in_device():
    rs = np.random.RandomState(4)
    N, n, Rn = 500, 5, 6
    gain = rs.randint(0, 4, (N, Rn, n))
    start = np.array([3, 0, 7, 1, 30])
    pts = start + gain.cumsum(axis=1)                                    # slot 4 is top throughout
    order = np.lexsort((rs.rand(N, Rn, n), -pts), axis=2)
    position = np.empty_like(order)
    np.put_along_axis(position, order, np.broadcast_to(np.arange(n), order.shape), axis=2)
    m = _hand_posterior()
    m._predict_ctx = ctx = TrajectoryCtx(position, pts)
    # five teams, six matches each (a pentagon three times over), six matchdays given out of order
    h = ["t00", "t01", "t02", "t03", "t04"] * 3
    a = ["t01", "t02", "t03", "t04", "t00"] * 3
    md = [40, 40, 40, 10, 10, 10, 30, 30, 20, 20, 20, 20, 50, -1, -1]
    table = {f"t{i:02d}": (int(v), 0, 0) for i, v in enumerate(start)}
    res = m.season_trajectory(h, a, md, num_simulations=N, random_state=5, current_table=table)
    call = ctx.calls[0]
    assert (call["points_min"], call["n_bins"]) == (0, 49) and call["key"] == (0, 5) and call["n_sims"] == N
    assert call["masks"] == [1, 0b1111, 0b11100]
    np.testing.assert_array_equal(call["home"], [0, 1, 2, 3, 4] * 3)     # the fixtures stay in the order given
    np.testing.assert_array_equal(call["fix_id"], [13, 14, 3, 4, 5, 8, 9, 10, 11, 6, 7, 0, 1, 2, 12])
    np.testing.assert_array_equal(call["round_end"], [2, 5, 9, 11, 14, 15])
    np.testing.assert_array_equal(res["matchdays"], [-1, 10, 20, 30, 40, 50])
    assert list(res["teams"]) == [f"t{i:02d}" for i in range(5)] and list(res["targets"]) == ["title", "top_four", "relegation"]
    want = R.counts(position, pts, np.array([[(mask >> p) & 1 for p in range(n)] for mask in call["masks"]], dtype=bool))
    for key in RAW.values():
        assert res[key].dtype == np.int64, key
        np.testing.assert_array_equal(res[key], want[key], err_msg=key)
    for key, ref in R.derived(want, N).items():
        assert np.shape(res[key]) == np.shape(ref), key
        np.testing.assert_array_equal(res[key], ref, err_msg=key)
    np.testing.assert_array_equal(res["target_count"][:, 4], [[N, N, 0]] * Rn)           # 30 points ahead
    np.testing.assert_array_equal(res["secured_count"][4, 0], [N] + [0] * Rn)
    assert res["lead_changes_count"][0] == N and res["expected_lead_changes"] == 0.0
    assert set(res) == {"teams", "targets", "matchdays", "position_count", "position_proba", "target_count",
                        "target_proba", "target_final_count", "final_given_inside", "final_given_inside_se",
                        "final_given_outside", "final_given_outside_se", "points_sum", "points_sq_sum", "points_mean",
                        "points_sd", "rounds_inside_count", "expected_rounds_inside", "secured_count",
                        "secured_by_proba", "lead_changes_count", "expected_lead_changes"}


# ---------------------------------------------------------------- the argument checks
def _raises(m, exc, *args, **kwargs):
    with pytest.raises(exc):
        m.season_trajectory(*args, **kwargs)
    assert m._predict_ctx is None   # no device context was ever made


@pytest.mark.parametrize("cls", [DixonColesMatchPredictor, ExtendedDixonColesMatchPredictor])
def test_argument_errors_come_before_the_device(cls):
    m = _hand_posterior(cls)
    H, A, D = ["t00", "t01"], ["t01", "t02"], [0, 1]
    _raises(m, KeyError, ["t00", "nope"], ["t01", "t02"], D, num_simulations=10)
    _raises(m, ValueError, [], [], [], num_simulations=10)
    _raises(m, ValueError, [], [], [], num_simulations=10, teams=["t00", "t01"])         # a table, but no fixture
    _raises(m, ValueError, H, A, [0], num_simulations=10)
    _raises(m, ValueError, H, A, [0, 1, 2], num_simulations=10)
    _raises(m, ValueError, H, A, [0.0, 1.0], num_simulations=10)
    _raises(m, ValueError, H, A, [False, True], num_simulations=10)
    _raises(m, ValueError, H, A, D, num_simulations=10, teams=["t00", "t01"])
    _raises(m, ValueError, ["t00", "t01"], ["t00", "t02"], D, num_simulations=10)
    _raises(m, ValueError, H, A, D, num_simulations=0)
    _raises(m, ValueError, H, A, D, num_simulations=10, current_table={"t00": (-1, 0, 0)})
    _raises(m, ValueError, H, A, D, num_simulations=10, points=(3, -1, 0))
    _raises(m, ValueError, H, A, D, num_simulations=10, tiebreak="away_goals")
    _raises(m, ValueError, H, A, D, num_simulations=10, targets={})
    _raises(m, ValueError, H, A, D, num_simulations=10, targets={"fourth": (3,)})        # three rows
    _raises(m, ValueError, H, A, D, num_simulations=10, targets={f"k{i}": (0,) for i in range(9)})
    h = np.tile([0, 1, 2], LEVERAGE_MAX_FIXTURES // 3 + 1)[:LEVERAGE_MAX_FIXTURES + 1]
    _raises(m, ValueError, h, (h + 1) % 3, np.zeros(h.size, dtype=int), num_simulations=10)
    many = np.tile([0, 1, 2], 86)[:TRAJECTORY_MAX_ROUNDS + 1]
    _raises(m, ValueError, many, (many + 1) % 3, np.arange(many.size), num_simulations=10)
    assert POINTS_MAX_BINS == 1024
    _raises(m, ValueError, H, A, D, num_simulations=10, current_table={"t00": (0, 0, 0), "t02": (1021, 0, 0)})
    # (2, 1, 1): every match gives at least 1, so the totals at the END start at 2 -- those on the way at t01's 0
    m._predict_ctx = ctx = TrajectoryCtx(np.zeros((2, 2, 3), dtype=int) + [1, 2, 0], np.zeros((2, 2, 3), dtype=int) + [2, 2, 1019])
    m.season_trajectory(H, A, D, num_simulations=2, points=(2, 1, 1), current_table={"t00": (1, 0, 0), "t02": (1017, 0, 0)})
    assert (ctx.calls[0]["points_min"], ctx.calls[0]["n_bins"]) == (0, 1020)
    m._predict_ctx = None
    _raises(m, ValueError, H, A, D, num_simulations=10, points=(2, 1, 1), current_table={"t02": (1022, 0, 0)})
