"""simulate_season on the device (csrc/dc_season.hip.h) at the edges of its shapes, of the shared sampler
(csrc/dc_sampler.hip.h) and of the shared league table (csrc/dc_table.hip.h), against the numpy
restatement (tests/season_ref.py).  The cases are tests/sim_edge_cases.py's; tests/test_sim_edge_cases_host.py
shows on the CPU that each sits on its edge and that the restatement flags no simulation of any, so every
comparison here is exact equality over every simulation."""
import numpy as np
import pytest

import sim_edge_cases as E
from bpl.base import _prng_key

pytestmark = pytest.mark.gpu

SEASON = {c.name: c for c in E.season_cases()}
PER_SIMULATION = ("home_goals", "away_goals", "points", "position")
AGGREGATES = ("position_proba", "expected_points", "expected_goal_difference")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _run(c, **extra):
    try:
        return c.model.simulate_season(**c.call, **extra)
    finally:
        E.release(c.model)


def _equal(res, ref, keys=PER_SIMULATION + AGGREGATES):
    for key in keys:
        assert res[key].shape == ref[key].shape and res[key].dtype == ref[key].dtype, key
        np.testing.assert_array_equal(res[key], ref[key], err_msg=key)


@pytest.mark.parametrize("name", list(SEASON))
def test_bit_exact_against_restatement(name):
    c = SEASON[name]
    ref, table_idx = E.season_reference(c)
    assert not ref["flagged"].any()
    res = _run(c, return_tables=True, return_scores=True)
    assert list(res["teams"]) == list(np.asarray(c.model.teams)[table_idx])
    _equal(res, ref)
    N, n = res["position"].shape
    np.testing.assert_array_equal(np.sort(res["position"], axis=1), np.tile(np.arange(n, dtype=np.uint8), (N, 1)))


def test_slots_out_of_model_order():
    # the context takes the table in any slot order: the 300-team case with its slots as listed
    c = SEASON["shape_T300_n64_nf129_N65_S3"]
    listed = c.facts["listed"]
    ref, tab = E.season_reference_in_order(c, listed)
    assert not ref["flagged"].any()
    kw = c.call
    try:
        raw = c.model._device().simulate_season(kw["home_team"], kw["away_team"], listed, tab, (3, 1, 0),
                                                kw["num_simulations"], _prng_key(kw["random_state"]),
                                                return_tables=True, return_scores=True)
    finally:
        E.release(c.model)
    N = kw["num_simulations"]
    _equal(raw, ref, PER_SIMULATION)
    np.testing.assert_array_equal(raw["counts"] / N, ref["position_proba"])
    np.testing.assert_array_equal(raw["points_sum"] / N, ref["expected_points"])
    np.testing.assert_array_equal(raw["gd_sum"] / N, ref["expected_goal_difference"])


@pytest.mark.parametrize("kind", E.RHO_KINDS)
def test_ladder_reaches_both_ends_of_the_walk(kind):
    c = SEASON["ladder_" + kind]
    ref, _ = E.season_reference(c)
    res = _run(c, return_tables=True, return_scores=True)
    for key in ("home_goals", "away_goals"):
        g = res[key]
        assert g.dtype == np.uint8 and g.min() == 0 and g.max() == 255      # 255 as stored, not wrapped
        assert ((g > 63) & (g < 255)).any()
        np.testing.assert_array_equal(g, ref[key], err_msg=key)
    # ... and as booked: the points and the goal difference carry the capped scorelines
    np.testing.assert_array_equal(res["points"], ref["points"])
    np.testing.assert_array_equal(res["expected_goal_difference"], ref["expected_goal_difference"])
    assert res["expected_goal_difference"][9] > 255


def test_equal_words_leave_it_to_the_slot():
    c = SEASON["level_equal_words"]
    ref, _ = E.season_reference(c)
    a, b = c.facts["equal_slots"]
    res = _run(c, return_tables=True)
    assert res["position"][0, b] == res["position"][0, a] + 1
    np.testing.assert_array_equal(res["position"], ref["position"])


@pytest.mark.parametrize("points", [(1000, 1, 0), (0, 0, 0)])
def test_keys_at_the_table_limits_order_as_integers(points):
    c = SEASON["limits_%d_%d_%d" % points]
    ref, _ = E.season_reference(c)
    res = _run(c, return_tables=True)
    pts, gd, gf = E.season_keys(c)
    np.testing.assert_array_equal(res["points"], pts)
    np.testing.assert_array_equal(res["position"], ref["position"])
    # whoever is ahead has the larger key, as whole numbers
    for j in range(pts.shape[0]):
        order = np.argsort(res["position"][j])
        keys = [(int(pts[j, i]), int(gd[j, i]), int(gf[j, i])) for i in order]
        assert keys == sorted(keys, reverse=True)


@pytest.mark.parametrize("shape", E.SEASON_SMALL)
def test_aggregates_without_the_optional_outputs(shape):
    c = SEASON["shape_T%d_n%d_nf%d_N%d_S%d" % shape]
    ref, _ = E.season_reference(c)
    res = _run(c)
    assert set(res) == {"teams"} | set(AGGREGATES)
    _equal(res, ref, AGGREGATES)
