"""posterior_predictive_check on the device (csrc/dc_ppc.hip.h) at the edges of its shapes -- fixture
counts around the workgroup's 256-thread stride, 2 and 130 team slots, grids of depth 1 and 15 with goals
beyond them up to the cap of 255, replication and draw counts, arbitrary fixture ids -- against the numpy
restatement (tests/ppc_ref.py).  The cases are tests/sim_edge_cases.py's; tests/test_sim_edge_cases_host.py
shows on the CPU that each sits on its edge and that the restatement flags no replication of any, so the
integer comparisons cover every replication."""
import numpy as np
import pytest

import ppc_ref as PR
from ppc_compare import against_restatement as _against_restatement
import sim_edge_cases as E
from bpl.base import _prng_key

pytestmark = pytest.mark.gpu

PPC = {c.name: c for c in E.ppc_cases()}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _check(c):
    kw = c.call
    try:
        # ok_share = 1: no replication may be set aside
        return _against_restatement(c.model, kw["data"], kw["num_replications"], kw["random_state"], kw["max_goals"],
                                    ok_share=1.0)
    finally:
        E.release(c.model)


@pytest.mark.parametrize("name", list(PPC))
def test_bit_exact_against_restatement(name):
    c = PPC[name]
    res, x, y, ok = _check(c)
    assert ok.all()
    xr, yr, _ = E.ppc_reference(c)
    np.testing.assert_array_equal(res["replications"]["home_goals"], xr)
    np.testing.assert_array_equal(res["replications"]["away_goals"], yr)


@pytest.mark.parametrize("G", [1, 15])
def test_cap_of_255_inside_the_tallies(G):
    c = PPC["ladder_G%d" % G]
    res, x, y, _ = _check(c)
    gx, gy = res["replications"]["home_goals"], res["replications"]["away_goals"]
    assert gx.dtype == np.uint8 and gx.max() == 255 and gy.max() == 255 and gx.min() == 0
    idx, hs, as_ = PR.slots(c.model, c.call["data"])
    raw = PR.raw_tallies(x, y, hs, as_, idx.size, G)
    np.testing.assert_array_equal(res["scoreline"]["replicated"], raw["score"])
    np.testing.assert_array_equal(res["team_goals_for"]["replicated"], raw["team"][..., 0])
    np.testing.assert_array_equal(res["team_goals_against"]["replicated"], raw["team"][..., 1])
    np.testing.assert_array_equal(res["home_goals"]["replicated"], raw["sums"][:, 0])
    # sum x^2, sum y^2 and sum x y with 255 in them, through the variances and the correlation's numerator
    n = x.shape[1]
    np.testing.assert_allclose(res["home_goals_var"]["replicated"], x.var(axis=1), rtol=1e-12)
    np.testing.assert_allclose(res["away_goals_var"]["replicated"], y.var(axis=1), rtol=1e-12)
    assert res["scoreline"]["replicated"].sum(axis=(1, 2)).tolist() == [n] * x.shape[0]
    assert res["scoreline"]["observed"][G, G] >= 2 and res["scoreline"]["replicated"][:, G, G].min() >= 4


@pytest.mark.parametrize("G", [0, 16])
def test_depths_outside_1_to_15_are_refused(G):
    # max_goals = 0 is no grid the kernel is ever launched with: the method and the library both refuse it
    c = PPC["depth_1"]
    kw = c.call
    with pytest.raises(ValueError):
        c.model.posterior_predictive_check(kw["data"], num_replications=2, random_state=1, max_goals=G)
    from bpl._ffi import BPLHIP_EINVAL, BplHipError

    h = np.array([0, 1], dtype=np.uint16)
    try:
        with pytest.raises(BplHipError) as e:
            c.model._device().ppc(h, h[::-1], h, h[::-1], 2, G, 2, (1, 2))
        assert e.value.code == BPLHIP_EINVAL
    finally:
        E.release(c.model)


def test_fixture_ids_are_the_counters():
    c = E.ppc_fixture_ids()
    kw, fid = c.call, c.facts["fixture_id"]
    x, y, flagged = E.ppc_reference(c)
    assert not flagged.any()
    m, d, G, R = c.model, kw["data"], kw["max_goals"], kw["num_replications"]
    (_, device, q), = m._loglik_groups(d)[0]
    idx, hs, as_ = PR.slots(m, d)
    try:
        raw = device().ppc(q["home_idx"], q["away_idx"], hs, as_, idx.size, G, R, _prng_key(kw["random_state"]),
                           fixture_id=fid, return_scores=True)
    finally:
        E.release(m)
    np.testing.assert_array_equal(raw["home_goals"], x)
    np.testing.assert_array_equal(raw["away_goals"], y)
    want = PR.raw_tallies(x, y, hs, as_, idx.size, G)
    for nm in ("score", "outcome", "sums", "team"):
        np.testing.assert_array_equal(raw[nm].astype(np.int64), want[nm], err_msg=nm)
