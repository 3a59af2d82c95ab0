"""match_scenarios without a GPU: the scenario index, the derived arrays, the helpers of bpl/scenarios.py and the
argument checks, all host work, plus the new kernels' resources read from the built library.  The device is a
stand-in in the manner of tests/fake_ctx.py whose counts are tests/scenarios_ref.py's from fixed per-simulation
arrays."""
import numpy as np
import pytest

import code_object
import scenarios_ref as R
from bpl import DixonColesMatchPredictor, ExtendedDixonColesMatchPredictor, scenarios
from bpl.base import LEVERAGE_MAX_FIXTURES
from bpl.scenarios import (SCENARIO_MAX_CELLS, check_keys, coarsen, format_table, marginal, requirements,
                           scenario_from_counts, scenario_margins, scenario_shape)
from fake_ctx import FakePredictCtx

RESULT_KEYS = {"teams", "targets", "fixtures", "home", "away", "margin_cap", "shape", "margins", "scenario_count",
               "scenario_proba", "target_count", "target_proba", "joint_count", "conditional_proba", "conditional_se",
               "settled", "leverage"}


class ScenarioCtx(FakePredictCtx):
    """Stands in for bpl._ffi.HipContext: `season_scenarios` cross-tabulates the fixed per-simulation arrays it was
    made with under the masks and the keys it is given, and records its arguments."""

    def __init__(self, position, home_goals, away_goals):
        self.position, self.x, self.y = np.asarray(position), np.asarray(home_goals), np.asarray(away_goals)
        self.calls = []

    def season_scenarios(self, home_idx, away_idx, table_idx, table, points, n_sims, key, target_masks, key_fixture,
                         key_cap, chunk_sims=0):
        self.calls.append(dict(home=np.asarray(home_idx), away=np.asarray(away_idx), n_sims=n_sims, key=key,
                               masks=list(target_masks), key_fixture=list(key_fixture), key_cap=list(key_cap)))
        n = len(table_idx)
        assert self.position.shape == (n_sims, n) and self.x.shape == (n_sims, len(home_idx))
        inside = np.array([[(int(m) >> p) & 1 for p in range(n)] for m in target_masks], dtype=bool)
        sc, jc = R.counts(self.position, self.x, self.y, inside, key_fixture, key_cap)
        return {"scenario": sc.astype(np.uint64), "joint": jc.astype(np.uint64)}


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


def _assert_equal_results(got, want, keys=None):
    for key in (RESULT_KEYS if keys is None else keys):
        if key == "shape":
            assert tuple(got[key]) == tuple(want[key])
        else:
            assert np.asarray(got[key]).shape == np.asarray(want[key]).shape, key
            np.testing.assert_array_equal(got[key], want[key], err_msg=key)     # (NaN == NaN in assert_array_equal)


# ---------------------------------------------------------------- the scenario index
def test_index_margins_and_shape_for_mixed_caps():
    caps = (3, 1, 2)
    assert scenario_shape(caps) == (7, 3, 5) == R.shape_of(caps)
    mg = scenario_margins(caps)
    assert mg.shape == (105, 3) and mg.dtype == np.int64
    np.testing.assert_array_equal(mg, R.margins(caps))
    np.testing.assert_array_equal(mg[0], [3, 1, 2])              # class 0 everywhere: home by the cap or more
    np.testing.assert_array_equal(mg[-1], [-3, -1, -2])
    np.testing.assert_array_equal(mg[1], [3, 1, 1])              # the last key fixture runs fastest
    # m = class_0 * 15 + class_1 * 5 + class_2: a 5-0, a 1-1 and a 0-1 are classes 0, 1 and 3
    x, y = np.array([[5, 1, 0], [0, 0, 4], [2, 3, 1]]), np.array([[0, 1, 1], [2, 1, 0], [2, 0, 1]])
    np.testing.assert_array_equal(R.index(x, y, (0, 1, 2), caps), [0 * 15 + 1 * 5 + 3, 5 * 15 + 2 * 5 + 0, 3 * 15 + 0 * 5 + 2])
    np.testing.assert_array_equal(mg[[8, 85, 47]], [[3, 0, -1], [-2, -1, 2], [0, 1, 0]])
    # the key fixtures in another order: the index follows the order given
    np.testing.assert_array_equal(R.index(x, y, (2, 0), (2, 3)), [3 * 7 + 0, 0 * 7 + 5, 2 * 7 + 3])
    np.testing.assert_array_equal(scenario_margins((1,)), [[1], [0], [-1]])     # match_leverage's outcome order
    assert np.asarray(scenario_margins(caps)).reshape(7, 3, 5, 3)[4, 2, 1].tolist() == [-1, -1, 1]


# ---------------------------------------------------------------- derived quantities
def _hand_tables():
    """One key fixture with cap 1, two teams, two targets, N = 10: the draw never occurs; after a home win team 0 is
    always inside target 0 and never inside target 1."""
    scenario = np.array([4, 0, 6])
    joint = np.array([[[4, 0], [1, 4]], [[0, 0], [0, 0]], [[3, 3], [6, 0]]])
    return scenario, joint


def test_hand_written_tables_cell_by_cell():
    sc, jc = _hand_tables()
    got = scenario_from_counts(sc, jc, 10)
    np.testing.assert_array_equal(got["scenario_proba"], [0.4, 0.0, 0.6])
    np.testing.assert_array_equal(got["target_count"], [[7, 3], [7, 4]])
    np.testing.assert_array_equal(got["target_proba"], [[0.7, 0.3], [0.7, 0.4]])
    np.testing.assert_array_equal(got["conditional_proba"],
                                  [[[1.0, 0.0], [0.25, 1.0]], [[np.nan] * 2] * 2, [[0.5, 0.5], [1.0, 0.0]]])
    assert np.isnan(got["conditional_proba"]).sum() == 4 and np.isnan(got["conditional_se"]).sum() == 4
    np.testing.assert_array_equal(got["conditional_se"][0], [[0.0, 0.0], [np.sqrt(0.25 * 0.75 / 4), 0.0]])
    np.testing.assert_array_equal(got["conditional_se"][2, 0], [np.sqrt(0.5 * 0.5 / 6)] * 2)
    np.testing.assert_array_equal(got["settled"], [[[1, -1], [0, 1]], [[0, 0], [0, 0]], [[0, 0], [1, -1]]])
    assert got["settled"].dtype == np.int8
    lev = np.array([[0.4 * abs(1.0 - 0.7) + 0.6 * abs(0.5 - 0.7), 0.4 * abs(0.0 - 0.3) + 0.6 * abs(0.5 - 0.3)],
                    [0.4 * abs(0.25 - 0.7) + 0.6 * abs(1.0 - 0.7), 0.4 * abs(1.0 - 0.4) + 0.6 * abs(0.0 - 0.4)]])
    np.testing.assert_array_equal(got["leverage"], lev)
    for key in ("scenario_count", "joint_count", "target_count"):
        assert got[key].dtype == np.int64, key
    ref = R.derived(sc, jc, 10)
    for key, want in ref.items():
        np.testing.assert_array_equal(got[key], want, err_msg=key)


def _random_tables(caps, n, K, N, seed, never=()):
    """Tables of N simulations spread at random over the scenarios, none in the scenarios `never`."""
    rs = np.random.RandomState(seed)
    M = int(np.prod(R.shape_of(caps)))
    allowed = np.setdiff1d(np.arange(M), never)
    m = allowed[rs.randint(0, allowed.size, N)]
    inside = rs.rand(N, n, K) < rs.uniform(0.0, 1.0, (1, n, K))
    inside[:, 0, 0] = True                                       # team 0 is always inside target 0
    sc = np.zeros(M, dtype=np.int64)
    np.add.at(sc, m, 1)
    jc = np.zeros((M, n, K), dtype=np.int64)
    np.add.at(jc, m, inside.astype(np.int64))
    return sc, jc


def _result(caps, n, K, N, seed, never=()):
    sc, jc = _random_tables(caps, n, K, N, seed, never)
    k = len(caps)
    out = {"teams": np.array([f"t{i:02d}" for i in range(n)]), "targets": np.array([f"k{i}" for i in range(K)]),
           "fixtures": np.arange(10, 10 + k), "home": np.array([f"h{i}" for i in range(k)]),
           "away": np.array([f"a{i}" for i in range(k)]), "margin_cap": np.array(caps, dtype=np.int64),
           "shape": scenario_shape(caps), "margins": scenario_margins(caps)}
    out.update(scenario_from_counts(sc, jc, N))
    return out


def test_derived_arrays_against_the_restatement():
    res = _result((3, 1, 2), 4, 3, 500, seed=3, never=(0, 17, 104))
    ref = R.derived(res["scenario_count"], res["joint_count"], 500)
    for key, want in ref.items():
        assert res[key].shape == want.shape and res[key].dtype == want.dtype, key
        np.testing.assert_array_equal(res[key], want, err_msg=key)
    never = res["scenario_count"] == 0
    assert never[[0, 17, 104]].all()
    np.testing.assert_array_equal(np.isnan(res["conditional_proba"]), np.broadcast_to(never[:, None, None], (105, 4, 3)))
    np.testing.assert_array_equal(res["settled"][:, 0, 0], np.where(never, 0, 1))
    assert res["scenario_count"].sum() == 500


# ---------------------------------------------------------------- marginal and coarsen
@pytest.mark.parametrize("keep", [(0,), (2,), (0, 1), (1, 0), (2, 0), (0, 2, 1), (0, 1, 2)])
def test_marginal_against_the_loops(keep):
    caps = (3, 1, 2)
    res = _result(caps, 3, 2, 800, seed=5, never=(3, 50))
    got = marginal(res, keep)
    sc, jc = R.marginal(res["scenario_count"], res["joint_count"], caps, keep)
    np.testing.assert_array_equal(got["scenario_count"], sc)
    np.testing.assert_array_equal(got["joint_count"], jc)
    kept = [caps[q] for q in keep]
    assert got["shape"] == R.shape_of(kept) and got["margin_cap"].tolist() == kept
    np.testing.assert_array_equal(got["margins"], R.margins(kept))
    assert got["fixtures"].tolist() == [10 + q for q in keep] and got["home"].tolist() == [f"h{q}" for q in keep]
    for key, want in R.derived(sc, jc, 800).items():
        np.testing.assert_array_equal(got[key], want, err_msg=key)
    np.testing.assert_array_equal(got["target_count"], res["target_count"])
    assert set(got) == RESULT_KEYS


def test_marginal_refuses_bad_positions():
    res = _result((1, 1), 2, 1, 50, seed=1)
    for bad in ((), (0, 0), (2,), (-1,), (True,), (0.0,)):
        with pytest.raises(ValueError):
            marginal(res, bad)


@pytest.mark.parametrize("new", [1, (3, 1, 2), (1, 1, 1), (2, 1, 1), (3, 1, 1)])
def test_coarsen_against_the_loops(new):
    caps = (3, 1, 2)
    res = _result(caps, 3, 2, 900, seed=6, never=(1, 2, 60))
    got = coarsen(res, new)
    new_caps = [new] * 3 if isinstance(new, int) else list(new)
    sc, jc = R.coarsen(res["scenario_count"], res["joint_count"], caps, new_caps)
    np.testing.assert_array_equal(got["scenario_count"], sc)
    np.testing.assert_array_equal(got["joint_count"], jc)
    assert got["shape"] == R.shape_of(new_caps) and got["margin_cap"].tolist() == new_caps
    np.testing.assert_array_equal(got["margins"], R.margins(new_caps))
    for key, want in R.derived(sc, jc, 900).items():
        np.testing.assert_array_equal(got[key], want, err_msg=key)
    assert got["scenario_count"].sum() == 900 and set(got) == RESULT_KEYS
    if new_caps == list(caps):
        _assert_equal_results(got, res)


def test_coarsen_refuses_larger_or_malformed_caps():
    res = _result((2, 1), 2, 1, 50, seed=2)
    for bad in (3, 0, (2, 2), (1,), (1, 1, 1), (True, 1), (1.0, 1), 1.0):
        with pytest.raises(ValueError):
            coarsen(res, bad)


# ---------------------------------------------------------------- requirements and the table
def test_requirements_with_level_and_min_count():
    # two key fixtures with cap 1; team 0 / target 0 by scenario: count and inside
    sc = np.array([10, 1, 0, 4, 8, 2, 0, 0, 5])
    inside = np.array([10, 1, 0, 3, 4, 0, 0, 0, 5])
    jc = np.stack([inside, sc - inside], axis=1)[:, :, None]                  # team 1 is the complement
    res = {"teams": np.array(["us", "them"]), "targets": np.array(["safe"]), "margin_cap": np.array([1, 1]),
           "shape": (3, 3), "margins": scenario_margins((1, 1)), "home": np.array(["us", "them"]),
           "away": np.array(["x", "y"]), "fixtures": np.array([0, 1])}
    res.update(scenario_from_counts(sc, jc, 30))
    np.testing.assert_array_equal(requirements(res, "us", "safe"), [[1, 1], [1, 0], [-1, -1]])
    np.testing.assert_array_equal(requirements(res, "us", "safe", min_count=2), [[1, 1], [-1, -1]])
    np.testing.assert_array_equal(requirements(res, 0, 0, min_count=6), [[1, 1]])
    np.testing.assert_array_equal(requirements(res, "us", "safe", level=0.75), [[1, 1], [1, 0], [0, 1], [-1, -1]])
    np.testing.assert_array_equal(requirements(res, "us", "safe", level=0.5, min_count=5), [[1, 1], [0, 0], [-1, -1]])
    np.testing.assert_array_equal(requirements(res, "them", "safe"), [[0, -1]])
    assert requirements(res, "them", "safe", min_count=3).shape == (0, 2)
    # level 1.0 is settled = +1
    np.testing.assert_array_equal(requirements(res, "us", "safe"), res["margins"][res["settled"][:, 0, 0] == 1])
    for kw in (dict(level=0.0), dict(level=1.5), dict(min_count=0), dict(min_count=True), dict(min_count=1.5)):
        with pytest.raises(ValueError):
            requirements(res, "us", "safe", **kw)
    for team, target in (("nobody", "safe"), ("us", "title"), (2, 0), (0, 1)):
        with pytest.raises(ValueError):
            requirements(res, team, target)
    text = format_table(res, "us", "safe")
    lines = text.splitlines()
    assert lines[0].startswith("us: safe") and "6 of 9 scenarios occurred" in lines[0]
    assert "us v x" in lines[1] and "them v y" in lines[1] and len(lines) == 2 + 6
    assert lines[2].split()[:6] == ["home", "by", "1+", "home", "by", "1+"] and lines[2].rstrip().endswith("yes")
    assert "draw" in lines[3] and lines[3].split()[-1] == "0.5000"          # the 8 draw-draw simulations: 4 inside


# ---------------------------------------------------------------- the public method on a stand-in device
def _sims(N, n, F, seed):
    rs = np.random.RandomState(seed)
    position = np.argsort(rs.rand(N, n), axis=1)
    return position, rs.poisson(1.6, (N, F)), rs.poisson(1.1, (N, F))


def test_public_method_result_keys_and_tables():
    N = 400
    position, x, y = _sims(N, 5, 6, seed=8)
    m = _hand_posterior()
    m._predict_ctx = ctx = ScenarioCtx(position, x, y)
    h = ["t00", "t01", "t02", "t03", "t04", "t00"]
    a = ["t01", "t02", "t03", "t04", "t00", "t02"]
    res = m.match_scenarios(h, a, [5, 0, 3], num_simulations=N, random_state=5, margin_cap=(3, 1, 2))
    call = ctx.calls[0]
    assert call["key"] == (0, 5) and call["n_sims"] == N and call["masks"] == [1, 0b1111, 0b11100]
    assert call["key_fixture"] == [5, 0, 3] and call["key_cap"] == [3, 1, 2]
    assert set(res) == RESULT_KEYS
    assert list(res["teams"]) == [f"t{i:02d}" for i in range(5)] and list(res["targets"]) == ["title", "top_four", "relegation"]
    assert res["fixtures"].tolist() == [5, 0, 3] and res["fixtures"].dtype == np.int64
    assert list(res["home"]) == ["t00", "t00", "t03"] and list(res["away"]) == ["t02", "t01", "t04"]
    assert res["margin_cap"].tolist() == [3, 1, 2] and res["shape"] == (7, 3, 5)
    np.testing.assert_array_equal(res["margins"], R.margins((3, 1, 2)))
    inside = np.array([[(mask >> p) & 1 for p in range(5)] for mask in call["masks"]], dtype=bool)
    sc, jc = R.counts(position, x, y, inside, [5, 0, 3], [3, 1, 2])
    np.testing.assert_array_equal(res["scenario_count"], sc)
    np.testing.assert_array_equal(res["joint_count"], jc)
    for key in ("scenario_count", "joint_count", "target_count"):
        assert res[key].dtype == np.int64, key
    for key, want in R.derived(sc, jc, N).items():
        np.testing.assert_array_equal(res[key], want, err_msg=key)
    assert res["scenario_count"].sum() == N and res["joint_count"].shape == (105, 5, 3)
    assert res["joint_count"].reshape(7, 3, 5, 5, 3).shape[:3] == res["shape"]
    # one cap for all; the scenario axis of a single key fixture with cap 1 is match_leverage's outcome axis
    one = m.match_scenarios(h, a, [2], num_simulations=N, random_state=5)
    assert ctx.calls[-1]["key_cap"] == [1] and one["shape"] == (3,)
    outcome = np.where(x[:, 2] > y[:, 2], 0, np.where(x[:, 2] == y[:, 2], 1, 2))
    np.testing.assert_array_equal(one["scenario_count"], np.bincount(outcome, minlength=3))
    # the helpers agree with narrower calls on the same simulations
    two = m.match_scenarios(h, a, [3, 5], num_simulations=N, random_state=5, margin_cap=(2, 3))
    _assert_equal_results(marginal(res, (2, 0)), two)
    low = m.match_scenarios(h, a, [5, 0, 3], num_simulations=N, random_state=5, margin_cap=1)
    _assert_equal_results(coarsen(res, 1), low)
    assert scenarios.marginal is marginal


# ---------------------------------------------------------------- argument errors
def test_check_keys():
    keys, caps = check_keys([4, 0], 2, 5)
    assert keys.tolist() == [4, 0] and caps.tolist() == [2, 2] and keys.dtype == caps.dtype == np.int64
    keys, caps = check_keys(np.array([1, 2, 3]), np.array([3, 1, 2]), 4)
    assert keys.tolist() == [1, 2, 3] and caps.tolist() == [3, 1, 2]
    assert check_keys(range(8), 1, 8)[1].tolist() == [1] * 8                    # 3^8 = 6561 scenarios: the bound
    assert SCENARIO_MAX_CELLS == 6561 == 3 ** 8
    assert check_keys(range(4), 3, 4)[1].tolist() == [3] * 4                    # 7^4 = 2401
    for fixtures, cap, F in (([], 1, 5), (range(9), 1, 20), ([1, 1], 1, 5), ([5], 1, 5), ([-1], 1, 5), ([True], 1, 5),
                             ([1.0], 1, 5), ([0.5], 1, 5), (["0"], 1, 5), (3, 1, 5), ([0], 0, 5), ([0], 4, 5),
                             ([0], True, 5), ([0], 1.0, 5), ([0, 1], (1,), 5), ([0, 1], (1, 1, 1), 5), ([0, 1], (1, 4), 5),
                             ([0], None, 5), (range(5), 3, 5), (range(8), (1,) * 7 + (2,), 8), ([0], 1, 0)):
        with pytest.raises(ValueError):
            check_keys(fixtures, cap, F)


def _raises(m, exc, *args, **kwargs):
    with pytest.raises(exc):
        m.match_scenarios(*args, **kwargs)
    assert m._predict_ctx is None   # no device context was ever made


@pytest.mark.parametrize("cls", [DixonColesMatchPredictor, ExtendedDixonColesMatchPredictor])
def test_argument_errors_come_before_the_device(cls):
    m = _hand_posterior(cls)
    H, A = ["t00", "t01", "t02"], ["t01", "t02", "t00"]
    # the keys and the caps
    _raises(m, ValueError, H, A, [], num_simulations=10)
    _raises(m, ValueError, H, A, [0, 0], num_simulations=10)
    _raises(m, ValueError, H, A, [3], num_simulations=10)                       # an index equal to F
    _raises(m, ValueError, H, A, [True], num_simulations=10)
    _raises(m, ValueError, H, A, [1.0], num_simulations=10)
    _raises(m, ValueError, H, A, [0], num_simulations=10, margin_cap=0)
    _raises(m, ValueError, H, A, [0], num_simulations=10, margin_cap=4)
    _raises(m, ValueError, H, A, [0, 1], num_simulations=10, margin_cap=(1,))
    _raises(m, ValueError, H, A, [0, 1], num_simulations=10, margin_cap=(1, 2, 3))
    nine_h, nine_a = [f"t{i % 6:02d}" for i in range(9)], [f"t{(i + 1) % 6:02d}" for i in range(9)]
    _raises(m, ValueError, nine_h, nine_a, list(range(9)), num_simulations=10)  # 9 keys
    _raises(m, ValueError, nine_h, nine_a, list(range(5)), num_simulations=10, margin_cap=3)   # M = 7^5
    # match_leverage's own
    _raises(m, KeyError, ["t00", "nope"], ["t01", "t02"], [0], num_simulations=10)
    _raises(m, ValueError, [], [], [0], num_simulations=10)
    _raises(m, ValueError, H, A, [0], num_simulations=10, teams=["t00", "t01"])
    _raises(m, ValueError, ["t00", "t01"], ["t00", "t02"], [0], num_simulations=10)
    _raises(m, ValueError, H, A, [0], num_simulations=0)
    _raises(m, ValueError, H, A, [0], num_simulations=10, current_table={"t00": (-1, 0, 0)})
    _raises(m, ValueError, H, A, [0], num_simulations=10, points=(3, -1, 0))
    _raises(m, ValueError, H, A, [0], num_simulations=10, tiebreak="away_goals")
    _raises(m, ValueError, H, A, [0], num_simulations=10, targets={})
    _raises(m, ValueError, H, A, [0], num_simulations=10, targets={"fourth": (3,)})          # three rows
    _raises(m, ValueError, H, A, [0], num_simulations=10, targets={f"k{i}": (0,) for i in range(9)})
    h = np.tile([0, 1, 2], LEVERAGE_MAX_FIXTURES // 3 + 1)[:LEVERAGE_MAX_FIXTURES + 1]
    _raises(m, ValueError, h, (h + 1) % 3, [0], num_simulations=10)


# ---------------------------------------------------------------- the built kernels and the ABI
def test_scenario_kernels_have_no_scratch_and_fit_the_lds(tmp_path_factory):
    kernels = {k: v for k, v in code_object.read_kernels(tmp_path_factory).items() if "dc_scenario" in k}
    assert sum("dc_scenario_sim" in k for k in kernels) == 2 and sum("dc_scenario_count" in k for k in kernels) == 1, kernels
    for name, k in kernels.items():
        assert k["scratch"] == 0, (name, k)
        assert k["lds"] <= 64 * 1024, (name, k)


def test_the_abi_gains_one_symbol_in_both_places():
    import os
    import re

    from bpl import _ffi

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "bplhip.h")).read()
    declared = set(re.findall(r"\b(bplhip_[a-z_0-9]+)\s*\(", header)) - {"bplhip_ctx"}
    assert "bplhip_season_scenarios" in declared and declared == set(_ffi.ABI_SYMBOLS)
    for name, value in (("KEYS", _ffi.SCENARIO_MAX_KEYS), ("CAP", _ffi.SCENARIO_MAX_CAP), ("CELLS", SCENARIO_MAX_CELLS)):
        assert int(re.search(rf"#define BPLHIP_SCENARIO_MAX_{name} (\d+)", header).group(1)) == value
    decl = re.search(r"int bplhip_season_scenarios\((.*?)\);", header, re.S).group(1)
    params = [p.strip() for p in decl.split(",")]
    restype, argtypes = _ffi._SIGNATURES["bplhip_season_scenarios"]
    assert len(argtypes) == len(params) and [a is _ffi.C.c_void_p for a in argtypes] == ["*" in p for p in params]
    assert [p.split()[-1].lstrip("*") for p in params][-8:] == ["chunk_sims", "n_key", "key_fixture", "key_cap", "scenario",
                                                                "joint", "stream", "pair_init"]
    assert _ffi.ABI_VERSION == 2
