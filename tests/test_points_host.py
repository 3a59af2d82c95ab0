"""points_needed without a GPU: the points axis, the derived floats, `levels` and `targets` validation and the
argument checks, all host work (bpl/base.py), plus the new kernels' resources read from the built library.  The
device is a stand-in in the manner of tests/fake_ctx.py whose counts are tests/points_ref.py's from fixed
per-simulation arrays."""
import numpy as np
import pytest

import code_object
import points_ref as R
from bpl import DixonColesMatchPredictor, ExtendedDixonColesMatchPredictor
from bpl.base import LEVERAGE_MAX_FIXTURES, POINTS_MAX_BINS, check_levels, points_axis, points_from_counts
from fake_ctx import FakePredictCtx


class PointsCtx(FakePredictCtx):
    """Stands in for bpl._ffi.HipContext: `season_points` cross-tabulates the fixed per-simulation arrays it was
    made with under the masks and the axis it is given, and records its arguments."""

    def __init__(self, points, position):
        self.sim_points, self.sim_position = np.asarray(points), np.asarray(position)
        self.calls = []

    def season_points(self, home_idx, away_idx, table_idx, table, points, n_sims, key, target_masks, points_min,
                      n_bins, chunk_sims=0):
        self.calls.append(dict(home=np.asarray(home_idx), away=np.asarray(away_idx), table=np.asarray(table),
                               points=points, n_sims=n_sims, key=key, masks=list(target_masks),
                               points_min=points_min, n_bins=n_bins))
        n = len(table_idx)
        assert self.sim_points.shape == (n_sims, n)
        inside = np.array([[(int(m) >> p) & 1 for p in range(n)] for m in target_masks], dtype=bool)
        tables = R.counts(self.sim_points, self.sim_position, inside, points_min, n_bins)
        return dict(zip(("team_points", "team_target", "position_points", "gap"), (t.astype(np.uint64) for t in tables)))


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


# ---------------------------------------------------------------- the points axis
def test_axis_with_uneven_remaining_matches():
    # slot 0: 10 points, 3 matches -> 10..19; slot 1: 4 points, 1 match -> 4..7; slot 2: 30 points, 2 matches -> 30..36
    assert points_axis([10, 4, 30], [0, 0, 2], [1, 2, 0], (3, 1, 0)) == (4, 33)
    assert points_axis([10, 4, 30], [0, 0, 2], [1, 2, 0], (3, 1, 0)) == R.axis([10, 4, 30], [0, 0, 2], [1, 2, 0], (3, 1, 0))


def test_axis_with_teams_without_fixtures():
    # slots 1 and 3 do not play: their current points are both ends of their range, and can be either end of the axis
    assert points_axis([5, 0, 7, 50], [0], [2], (3, 1, 0)) == (0, 51)
    assert points_axis([5, 9, 7, 6], [0], [2], (3, 1, 0)) == (5, 6)          # 5..8, 9, 7..10, 6
    assert points_axis([5, 9, 7, 6], [], [], (3, 1, 0)) == (5, 5)            # no fixture at all: the table's spread
    assert points_axis([12], [], [], (3, 1, 0)) == (12, 1)


def test_axis_when_the_least_points_are_not_the_losers():
    # (win, draw, loss) = (1, 3, 0): the most a match gives is the draw's 3, the least the loss's 0
    assert points_axis([0, 0], [0, 1], [1, 0], (1, 3, 0)) == (0, 7)
    # (2, 1, 1): every match gives at least 1 -- the lower end moves up with the matches played
    assert points_axis([0, 10], [0, 0, 0], [1, 1, 1], (2, 1, 1)) == (3, 14)  # 3..6 and 13..16
    assert points_axis([3, 8], [0], [1], (0, 0, 0)) == (3, 6)
    for init, h, a, pts in (([0, 0], [0, 1], [1, 0], (1, 3, 0)), ([0, 10], [0, 0, 0], [1, 1, 1], (2, 1, 1))):
        assert points_axis(init, h, a, pts) == R.axis(init, h, a, pts)


# ---------------------------------------------------------------- derived quantities
def _hand_tables():
    """Two teams, one target, P = 4 (points 10..13), N = 10.  Team 0 never ends on 12 and never on 10 (bin 0);
    team 1 is inside the target in every simulation."""
    team_points = np.array([[0, 4, 0, 6], [5, 0, 5, 0]])
    team_target = np.array([[[0], [1], [0], [6]], [[5], [0], [5], [0]]])
    position_points = np.array([[0, 2, 2, 6], [5, 2, 3, 0]])
    gap = np.array([[3, 4, 2, 1]])
    return team_points, team_target, position_points, gap


def test_hand_written_tables_cell_by_cell():
    tables = _hand_tables()
    levels = np.array([0.5, 0.8, 1.0])
    got = points_from_counts(*tables, 10, 10, levels)
    np.testing.assert_array_equal(got["points"], [10, 11, 12, 13])
    np.testing.assert_array_equal(got["target_count"], [[7], [10]])
    np.testing.assert_array_equal(got["target_proba"], [[0.7], [1.0]])
    np.testing.assert_array_equal(got["team_points_proba"], [[0.0, 0.4, 0.0, 0.6], [0.5, 0.0, 0.5, 0.0]])
    # a team that never ended on a bin: NaN there and only there
    np.testing.assert_array_equal(got["proba_given_points"][:, :, 0], [[np.nan, 0.25, np.nan, 1.0], [1.0, np.nan, 1.0, np.nan]])
    np.testing.assert_array_equal(got["se_given_points"][0, :, 0], [np.nan, np.sqrt(0.25 * 0.75 / 4), np.nan, 0.0])
    # at least p: team 0 7/10, 7/10, 6/6, 6/6; team 1 reaches nothing above 12
    np.testing.assert_array_equal(got["proba_given_at_least"][:, :, 0], [[0.7, 0.7, 1.0, 1.0], [1.0, 1.0, 1.0, np.nan]])
    # team 0: 0.5 is reached at the LOWEST bin, 0.8 and 1.0 first at 12 points; team 1 at the lowest bin throughout
    np.testing.assert_array_equal(got["points_needed"], [[[10.0, 12.0, 12.0]], [[10.0, 10.0, 10.0]]])
    np.testing.assert_array_equal(got["position_points_mean"], [(2 * 11 + 2 * 12 + 6 * 13) / 10, (50 + 22 + 36) / 10])
    np.testing.assert_array_equal(got["position_points_quantile"], [[13, 10], [13, 12], [13, 12]])
    assert got["position_points_quantile"].dtype == np.int64
    np.testing.assert_array_equal(got["level_proba"], [0.3])
    ref = R.derived(*tables, 10, 10, levels)
    for key, want in ref.items():
        np.testing.assert_array_equal(got[key], want, err_msg=key)     # (NaN == NaN in assert_array_equal)


def test_a_level_no_bin_reaches():
    team_points = np.array([[4, 4, 2]])
    team_target = np.array([[[1, 0], [2, 0], [1, 0]]])                   # target 1 is never met
    got = points_from_counts(team_points, team_target, team_points, np.zeros((0, 3), dtype=np.int64), 0, 10,
                             np.array([0.4, 0.5, 0.9]))
    # at least 0: 4/10, at least 1: 3/6, at least 2: 1/2
    np.testing.assert_array_equal(got["proba_given_at_least"][0, :, 0], [0.4, 0.5, 0.5])
    np.testing.assert_array_equal(got["points_needed"][0, 0], [0.0, 1.0, np.nan])
    np.testing.assert_array_equal(got["points_needed"][0, 1], [np.nan, np.nan, np.nan])
    assert got["level_proba"].shape == (0,) and got["gap_count"].shape == (0, 3)
    ref = R.derived(team_points, team_target, team_points, np.zeros((0, 3), dtype=np.int64), 0, 10, [0.4, 0.5, 0.9])
    for key, want in ref.items():
        np.testing.assert_array_equal(got[key], want, err_msg=key)


def test_derived_quantities_against_the_restatement():
    rs = np.random.RandomState(4)
    N, n = 700, 5
    pts = rs.binomial(12, rs.uniform(0.2, 0.8, n), (N, n)) + np.array([3, 0, 7, 1, 30])   # slot 4 is always top
    order = np.lexsort((rs.rand(N, n), -pts), axis=1)                   # slots by points descending, random ties
    position = np.empty_like(order)
    np.put_along_axis(position, order, np.broadcast_to(np.arange(n), (N, n)), axis=1)
    m = _hand_posterior()
    m._predict_ctx = ctx = PointsCtx(pts, position)
    # five teams, four matches each (a double-round pentagon); the table carries the offsets
    h = ["t00", "t01", "t02", "t03", "t04"] * 2
    a = ["t01", "t02", "t03", "t04", "t00"] * 2
    table = {f"t{i:02d}": (int(v), 0, 0) for i, v in enumerate([3, 0, 7, 1, 30])}
    levels = (0.25, 0.5, 0.9, 1.0)
    res = m.points_needed(h, a, num_simulations=N, random_state=5, current_table=table, levels=levels)
    call = ctx.calls[0]
    assert (call["points_min"], call["n_bins"]) == (0, 43) and call["key"] == (0, 5) and call["n_sims"] == N
    assert call["masks"] == [1, 0b1111, 0b11100]
    assert list(res["teams"]) == [f"t{i:02d}" for i in range(5)] and list(res["targets"]) == ["title", "top_four", "relegation"]
    np.testing.assert_array_equal(res["points"], np.arange(43))
    np.testing.assert_array_equal(res["levels"], levels)
    for key in ("team_points_count", "team_target_count", "position_points_count", "gap_count", "target_count"):
        assert res[key].dtype == np.int64, key
    ref = R.derived(res["team_points_count"], res["team_target_count"], res["position_points_count"], res["gap_count"],
                    0, N, levels)
    for key, want in ref.items():
        assert res[key].shape == want.shape, key
        np.testing.assert_array_equal(res[key], want, err_msg=key)
    assert res["points_needed"].shape == (5, 3, 4) and res["position_points_quantile"].shape == (4, 5)
    np.testing.assert_array_equal(res["target_count"][4], [N, N, 0])     # 30 points ahead: always champion
    np.testing.assert_array_equal(res["points_needed"][4, 0], 0.0)       # ... whatever it ends on: the lowest bin
    assert np.isnan(res["points_needed"][4, 2]).all()
    for key in ("team_points_count", "position_points_count", "gap_count"):
        np.testing.assert_array_equal(res[key].sum(axis=1), N, err_msg=key)
    assert set(res) == {"teams", "targets", "levels", "points", "team_points_count", "team_points_proba",
                        "team_target_count", "target_count", "target_proba", "proba_given_points", "se_given_points",
                        "proba_given_at_least", "points_needed", "position_points_count", "position_points_mean",
                        "position_points_quantile", "gap_count", "level_proba"}


# ---------------------------------------------------------------- levels, targets and the other arguments
def test_levels_validation():
    np.testing.assert_array_equal(check_levels((0.5, 1)), [0.5, 1.0])
    np.testing.assert_array_equal(check_levels(np.array([1e-9])), [1e-9])
    for bad in ((), [], (0.0,), (0.5, 1.0000001), (-0.1,), (float("nan"),), ("half",), 0.5, None):
        with pytest.raises(ValueError):
            check_levels(bad)


def _raises(m, exc, *args, **kwargs):
    with pytest.raises(exc):
        m.points_needed(*args, **kwargs)
    assert m._predict_ctx is None   # no device context was ever made


@pytest.mark.parametrize("cls", [DixonColesMatchPredictor, ExtendedDixonColesMatchPredictor])
def test_argument_errors_come_before_the_device(cls):
    m = _hand_posterior(cls)
    H, A = ["t00", "t01"], ["t01", "t02"]
    _raises(m, KeyError, ["t00", "nope"], ["t01", "t02"], num_simulations=10)
    _raises(m, ValueError, [], [], num_simulations=10)
    _raises(m, ValueError, H, A, num_simulations=10, teams=["t00", "t01"])
    _raises(m, ValueError, ["t00", "t01"], ["t00", "t02"], num_simulations=10)
    _raises(m, ValueError, H, A, num_simulations=0)
    _raises(m, ValueError, H, A, num_simulations=10, current_table={"t00": (-1, 0, 0)})
    _raises(m, ValueError, H, A, num_simulations=10, points=(3, -1, 0))
    _raises(m, ValueError, H, A, num_simulations=10, tiebreak="away_goals")
    _raises(m, ValueError, H, A, num_simulations=10, targets={})
    _raises(m, ValueError, H, A, num_simulations=10, targets={"fourth": (3,)})          # three rows
    _raises(m, ValueError, H, A, num_simulations=10, targets={f"k{i}": (0,) for i in range(9)})
    _raises(m, ValueError, H, A, num_simulations=10, levels=())
    _raises(m, ValueError, H, A, num_simulations=10, levels=(0.5, 0.0))
    _raises(m, ValueError, H, A, num_simulations=10, levels=(1.5,))
    h = np.tile([0, 1, 2], LEVERAGE_MAX_FIXTURES // 3 + 1)[:LEVERAGE_MAX_FIXTURES + 1]
    _raises(m, ValueError, h, (h + 1) % 3, num_simulations=10)
    # the points axis: 0 .. 1020 + 3 is 1024 bins, one more point is one too many
    assert POINTS_MAX_BINS == 1024
    _raises(m, ValueError, H, A, num_simulations=10, current_table={"t00": (0, 0, 0), "t02": (1021, 0, 0)})
    _raises(m, ValueError, H, A, num_simulations=10, points=(600, 1, 0))                # t01 plays twice: 0..1200


def test_an_axis_of_exactly_1024_bins_is_accepted():
    m = _hand_posterior()
    m._predict_ctx = ctx = PointsCtx(np.array([[3, 1, 1020]] * 2), np.array([[1, 2, 0]] * 2))
    res = m.points_needed(["t00", "t01"], ["t01", "t02"], num_simulations=2,
                          current_table={"t00": (0, 0, 0), "t02": (1020, 0, 0)}, targets={"title": (0,)})
    assert (ctx.calls[0]["points_min"], ctx.calls[0]["n_bins"]) == (0, 1024) and res["points"][-1] == 1023
    np.testing.assert_array_equal(res["gap_count"][:, [2, 1017]], [[0, 2], [2, 0]])


# ---------------------------------------------------------------- the built kernels
def test_points_kernels_have_no_scratch_and_fit_the_lds(tmp_path_factory):
    kernels = {k: v for k, v in code_object.read_kernels(tmp_path_factory).items() if "dc_points" in k}
    assert sum("dc_points_sim" in k for k in kernels) == 2 and sum("dc_points_count" in k for k in kernels) == 1, kernels
    for name, k in kernels.items():
        assert k["scratch"] == 0, (name, k)
        assert k["lds"] <= 64 * 1024, (name, k)
