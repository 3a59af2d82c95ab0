"""match_leverage without a GPU: the `targets` parsing, the derived floats and the argument checks, all
host work (bpl/base.py).  The device is a stand-in whose counts are tests/leverage_ref.py's from fixed
per-simulation arrays."""
import numpy as np
import pytest

import leverage_ref as L
from bpl import DixonColesMatchPredictor, ExtendedDixonColesMatchPredictor
from bpl.base import LEVERAGE_MAX_FIXTURES, leverage_targets


class LeverageCtx:
    """Stands in for bpl._ffi.HipContext: `match_leverage` cross-tabulates the fixed per-simulation arrays
    it was made with under the masks it is given, and records its arguments."""

    def __init__(self, position, home_goals, away_goals):
        self.position, self.x, self.y = (np.asarray(v) for v in (position, home_goals, away_goals))
        self.calls = []

    def predict_set_posterior(self, *arrays):
        pass

    def match_leverage(self, home_idx, away_idx, table_idx, table, points, n_sims, key, target_masks, chunk_sims=0):
        self.calls.append(dict(home=np.asarray(home_idx), away=np.asarray(away_idx), table_idx=np.asarray(table_idx),
                               table=np.asarray(table), points=points, n_sims=n_sims, key=key,
                               masks=list(target_masks)))
        n = len(table_idx)
        assert self.position.shape == (n_sims, n) and self.x.shape == (n_sims, len(home_idx))
        inside = np.array([[(int(m) >> p) & 1 for p in range(n)] for m in target_masks], dtype=bool)
        outcome, target, joint = L.counts(self.position, self.x, self.y, inside)
        return {"outcome": outcome.astype(np.uint64), "target": target.astype(np.uint64),
                "joint": joint.astype(np.uint64)}


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


# ---------------------------------------------------------------- targets
def test_targets_negatives_duplicates_and_positions_outside_the_table():
    names, masks = leverage_targets({"a": (0, -1), "b": [1, 1, 1, -5], "c": (2, 7, -9, 99), "d": range(5)}, 5)
    assert names == ["a", "b", "c", "d"]
    assert masks == [0b10001, 0b00011, 0b00100, 0b11111]
    assert leverage_targets({"last": np.array([-1])}, 64) == (["last"], [1 << 63])


def test_an_emptied_target_raises():
    for positions in ((), (5,), (-6,), (7, -9)):
        with pytest.raises(ValueError):
            leverage_targets({"ok": (0,), "gone": positions}, 5)
    with pytest.raises(ValueError):
        leverage_targets({"half": (0.5,)}, 5)


def test_target_count_limits():
    with pytest.raises(ValueError):
        leverage_targets({}, 5)
    with pytest.raises(ValueError):
        leverage_targets({f"k{i}": (0,) for i in range(9)}, 5)
    assert len(leverage_targets({f"k{i}": (i % 5,) for i in range(8)}, 5)[1]) == 8


def test_default_targets():
    names, masks = leverage_targets(None, 20)
    assert names == ["title", "top_four", "relegation"]
    assert masks == [1, 0b1111, 0b111 << 17]
    # three rows: the top four are the whole table, and so are the bottom three
    assert leverage_targets(None, 3)[1] == [1, 0b111, 0b111]
    assert leverage_targets(None, 2)[1] == [1, 0b11, 0b11]


# ---------------------------------------------------------------- derived quantities
def _two_by_two():
    """Two fixtures, two teams, N = 8.  Fixture 0 (t00 v t01): 4 home wins, 2 draws, 2 away wins; fixture 1
    (t01 v t00) never ends in an away win.  t00 is top in simulations 0-4."""
    position = np.array([[0, 1]] * 5 + [[1, 0]] * 3)
    x = np.array([[2, 1], [1, 1], [3, 2], [1, 2], [0, 0], [1, 1], [0, 3], [0, 2]])
    y = np.array([[0, 0], [0, 0], [1, 1], [0, 1], [0, 0], [1, 1], [1, 1], [2, 0]])
    return position, x, y


def test_hand_computed_two_fixture_table():
    position, x, y = _two_by_two()
    m = _hand_posterior()
    m._predict_ctx = ctx = LeverageCtx(position, x, y)
    res = m.match_leverage(["t00", "t01"], ["t01", "t00"], num_simulations=8, random_state=5,
                           targets={"title": (0,), "bottom": (-1,)})
    assert list(res["teams"]) == ["t00", "t01"] and list(res["targets"]) == ["title", "bottom"]
    assert ctx.calls[0]["masks"] == [0b01, 0b10] and ctx.calls[0]["key"] == (0, 5) and ctx.calls[0]["n_sims"] == 8
    assert res["outcome_count"].dtype == np.int64 and res["joint_count"].dtype == np.int64
    np.testing.assert_array_equal(res["outcome_count"], [[4, 2, 2], [6, 2, 0]])
    np.testing.assert_array_equal(res["outcome_proba"], [[0.5, 0.25, 0.25], [0.75, 0.25, 0.0]])
    np.testing.assert_array_equal(res["target_count"], [[5, 3], [3, 5]])
    np.testing.assert_array_equal(res["target_proba"], [[0.625, 0.375], [0.375, 0.625]])
    # fixture 0: home wins are simulations 0-3 (t00 top in all), draws 4, 5 (t00 top in 4), away wins 6, 7
    np.testing.assert_array_equal(res["joint_count"][0, :, 0, 0], [4, 1, 0])
    np.testing.assert_array_equal(res["joint_count"][0, :, 1, 0], [0, 1, 2])
    np.testing.assert_array_equal(res["conditional_proba"][0, :, 0, 0], [1.0, 0.5, 0.0])
    np.testing.assert_array_equal(res["conditional_se"][0, :, 0, 0], [0.0, np.sqrt(0.25 / 2), 0.0])
    # leverage = 0.5 |1 - 5/8| + 0.25 |0.5 - 5/8| + 0.25 |0 - 5/8|
    assert res["leverage"][0, 0, 0] == 0.5 * 0.375 + 0.25 * 0.125 + 0.25 * 0.625
    # fixture 1: home wins are simulations 0-3, 6, 7 (t00 top in four of them), draws 4, 5 (t00 top in 4)
    np.testing.assert_array_equal(res["joint_count"][1, :, 0, 0], [4, 1, 0])
    # the away win never occurred: NaN there and only there, and the leverage is finite without it
    nan = np.isnan(res["conditional_proba"])
    assert nan[1, 2].all() and nan.sum() == 4
    np.testing.assert_array_equal(np.isnan(res["conditional_se"]), nan)
    assert np.isfinite(res["leverage"]).all()
    p_home, p_draw = res["conditional_proba"][1, 0, 0, 0], res["conditional_proba"][1, 1, 0, 0]
    assert (p_home, p_draw) == (4 / 6, 0.5)
    assert res["leverage"][1, 0, 0] == pytest.approx(0.75 * (4 / 6 - 0.625) + 0.25 * 0.125, rel=1e-15)
    # the restatement, cell by cell
    ref = L.derived(res["outcome_count"], res["target_count"], res["joint_count"], 8)
    for key, want in ref.items():
        np.testing.assert_allclose(res[key], want, rtol=1e-15, atol=0, err_msg=key)
    assert set(res) == {"teams", "targets", "outcome_count", "outcome_proba", "target_count", "target_proba",
                        "joint_count", "conditional_proba", "conditional_se", "leverage"}


def test_derived_quantities_against_the_restatement():
    rs = np.random.RandomState(3)
    N, n, F = 500, 5, 7
    position = np.argsort(rs.rand(N, n), axis=1)
    x, y = rs.poisson(1.4, (N, F)), rs.poisson(1.1, (N, F))
    x[:, 2], y[:, 2] = 3, 0                      # fixture 2 is always a home win
    m = _hand_posterior()
    m._predict_ctx = LeverageCtx(position, x, y)
    h = ["t00", "t01", "t02", "t03", "t04", "t00", "t02"]
    a = ["t01", "t02", "t03", "t04", "t00", "t03", "t04"]
    res = m.match_leverage(h, a, num_simulations=N, random_state=1)
    assert res["joint_count"].shape == (F, 3, n, 3) and res["leverage"].shape == (F, n, 3)
    ref = L.derived(res["outcome_count"], res["target_count"], res["joint_count"], N)
    for key, want in ref.items():
        np.testing.assert_allclose(res[key], want, rtol=1e-14, atol=0, err_msg=key)
    np.testing.assert_array_equal(res["outcome_count"].sum(axis=1), N)
    np.testing.assert_array_equal(res["joint_count"].sum(axis=1), np.broadcast_to(res["target_count"], (F, n, 3)))
    # a fixture whose result is known in advance moves nothing
    assert np.isnan(res["conditional_proba"][2, 1:]).all() and not np.isnan(res["conditional_proba"][2, 0]).any()
    np.testing.assert_array_equal(res["leverage"][2], 0.0)
    assert (res["leverage"] >= 0).all() and np.isfinite(res["leverage"]).all()


# ---------------------------------------------------------------- argument checks
def _raises(m, exc, *args, **kwargs):
    with pytest.raises(exc):
        m.match_leverage(*args, **kwargs)
    assert m._predict_ctx is None   # no device context was ever made


@pytest.mark.parametrize("cls", [DixonColesMatchPredictor, ExtendedDixonColesMatchPredictor])
def test_season_argument_errors_surface_unchanged(cls):
    m = _hand_posterior(cls)
    H, A = ["t00", "t01"], ["t01", "t02"]
    _raises(m, KeyError, ["t00", "nope"], ["t01", "t02"], num_simulations=10)
    _raises(m, KeyError, H, A, num_simulations=10, current_table={"nope": (1, 1, 1)})
    _raises(m, ValueError, [], [], num_simulations=10)
    _raises(m, ValueError, H, A, num_simulations=10, teams=["t00", "t01"])
    _raises(m, ValueError, ["t00", "t01"], ["t00", "t02"], num_simulations=10)
    _raises(m, ValueError, H, A, num_simulations=0)
    _raises(m, ValueError, H, A, num_simulations=2 ** 31)
    _raises(m, ValueError, H, A, num_simulations=10, current_table={"t00": (-1, 0, 0)})
    _raises(m, ValueError, H, A, num_simulations=10, points=(3, -1, 0))
    _raises(m, ValueError, [0, 1], [1, 9], num_simulations=10)
    # the targets are checked on the host too, against the table the season arguments resolve to
    _raises(m, ValueError, H, A, num_simulations=10, targets={})
    _raises(m, ValueError, H, A, num_simulations=10, targets={"fourth": (3,)})          # three rows
    _raises(m, ValueError, H, A, num_simulations=10, targets={f"k{i}": (0,) for i in range(9)})


def test_more_than_4096_fixtures_raises():
    m = _hand_posterior()
    h = np.tile([0, 1, 2], LEVERAGE_MAX_FIXTURES // 3 + 1)[:LEVERAGE_MAX_FIXTURES + 1]
    assert LEVERAGE_MAX_FIXTURES == 4096
    _raises(m, ValueError, h, (h + 1) % 3, num_simulations=10)
    position = np.zeros((2, 3), dtype=np.int64) + np.arange(3)
    m._predict_ctx = LeverageCtx(position, np.zeros((2, 4096), int), np.zeros((2, 4096), int))
    assert m.match_leverage(h[:4096], (h[:4096] + 1) % 3, num_simulations=2)["joint_count"].shape == (4096, 3, 3, 3)
