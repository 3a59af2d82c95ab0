"""simulate_tournament on the device (csrc/dc_tournament.hip.h) at the edges of its formats -- group
sizes, qualifier counts, bracket sizes, simulation and draw counts, hosts, the rule after 32 level
attempts, tables level or at their limits -- against the numpy restatement (tests/tournament_ref.py).
The cases are tests/sim_edge_cases.py's; tests/test_sim_edge_cases_host.py shows on the CPU that each sits
on its edge and that the restatement flags no simulation of any, so every comparison is exact equality."""
import numpy as np
import pytest

import sim_edge_cases as E

pytestmark = pytest.mark.gpu

TOURNAMENT = {c.name: c for c in E.tournament_cases()}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _run(c, **extra):
    try:
        return c.model.simulate_tournament(**c.call, **extra)
    finally:
        E.release(c.model)


def _equal(res, inp, want):
    assert list(res["teams"]) == list(inp["teams"])
    keys = ["stage", "round_proba"] + (["group_position_proba"] if inp["group"] is not None else [])
    assert set(res) == set(keys) | {"teams"}
    for key in keys:
        assert res[key].shape == want[key].shape and res[key].dtype == want[key].dtype, key
        np.testing.assert_array_equal(res[key], want[key], err_msg=key)


@pytest.mark.parametrize("name", list(TOURNAMENT))
def test_bit_exact_against_restatement(name):
    c = TOURNAMENT[name]
    inp, ref, want = E.tournament_reference(c)
    assert not ref["flagged"].any()
    res = _run(c, return_stages=True)
    _equal(res, inp, want)


@pytest.mark.parametrize("nb", [2, 8, 64])
def test_first_listed_side_goes_through_after_32_level_attempts(nb):
    c = TOURNAMENT["level_knockout_%d" % nb]
    inp, _, _ = E.tournament_reference(c)
    res = _run(c, return_stages=True)
    N, R = inp["num_simulations"], inp["rounds"]
    np.testing.assert_array_equal(res["stage"], np.tile(E.level_knockout_stage(nb), (N, 1)))
    assert (res["stage"][:, 0] == R + 1).all() and res["round_proba"][0, R] == 1.0   # entry 0 wins the final
    for r in range(R):
        assert (res["stage"][:, 1 << r] == r + 1).all()                              # entry 2^r goes out in round r
    assert (res["stage"][:, 1] == 1).all()    # the host listed second is at home, and still the second-listed side


@pytest.mark.parametrize("fmt", [(8, 8, 2, 0, 16), (8, 8, 4, 0, 32)])
def test_all_eight_group_places(fmt):
    c = TOURNAMENT["format_%dx%d_adv%d_best%d_ko%d_N257_S3" % fmt]
    inp, ref, want = E.tournament_reference(c)
    res = _run(c)
    P = res["group_position_proba"]
    assert P.shape == (64, 8) and (P > 0).any(axis=0).all()
    np.testing.assert_array_equal(P, want["group_position_proba"])
    np.testing.assert_array_equal(np.rint(P * 257).sum(axis=0), np.full(8, 8 * 257.0))
    # without the stages: the same aggregates
    np.testing.assert_array_equal(res["round_proba"], want["round_proba"])


def test_equal_words_leave_it_to_the_slot():
    c = TOURNAMENT["level_groups_8x8_equal_words"]
    inp, ref, want = E.tournament_reference(c)
    a, b = c.facts["equal_slots"]
    res = _run(c, return_stages=True)
    N = inp["num_simulations"]
    place = np.rint(res["group_position_proba"] * N).astype(np.int64)
    np.testing.assert_array_equal(place, ref["position_counts"])
    # simulation 0 alone put slot a in the place just above slot b's
    rest = np.zeros((64, 8), dtype=np.int64)
    np.add.at(rest, (np.tile(np.arange(64), N - 1), ref["position"][1:].ravel()), 1)
    first = place - rest
    assert first[a].argmax() + 1 == first[b].argmax() and first[a].sum() == 1
    np.testing.assert_array_equal(res["stage"], want["stage"])
