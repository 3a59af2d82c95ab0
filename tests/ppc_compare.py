"""The comparison tests/test_gpu_ppc.py and tests/test_gpu_ppc_edges.py share: posterior_predictive_check on
the device against the numpy restatement (tests/ppc_ref.py), scorelines and every statistic."""
import numpy as np

import ppc_ref as PR
from bpl.base import _prng_key
from bpl.ppc import STATISTICS

INTEGER_STATS = ("scoreline", "outcome", "home_goals", "away_goals", "team_goals_for", "team_goals_against",
                 "team_points")


def against_restatement(m, d, R, seed, G, ok_share=0.9):
    res = m.posterior_predictive_check(d, num_replications=R, random_state=seed, max_goals=G,
                                       return_replications=True)
    x, y, flagged = PR.replicate(m, d, R, _prng_key(seed))
    ok = ~flagged
    assert ok.mean() >= ok_share, ok.mean()
    np.testing.assert_array_equal(res["replications"]["home_goals"][ok], x[ok])
    np.testing.assert_array_equal(res["replications"]["away_goals"][ok], y[ok])
    idx, hs, as_ = PR.slots(m, d)
    assert list(res["teams"]) == list(np.asarray(m.teams)[idx])
    want = PR.stats(x, y, hs, as_, idx.size, G)
    obs = PR.stats(d["home_goals"], d["away_goals"], hs, as_, idx.size, G)
    for nm in STATISTICS:
        got = res[nm]["replicated"]
        assert got.shape == want[nm].shape, nm
        if nm in INTEGER_STATS:
            np.testing.assert_array_equal(got[ok], want[nm][ok])
            np.testing.assert_array_equal(res[nm]["observed"], obs[nm][0])
        else:
            np.testing.assert_allclose(got[ok], want[nm][ok], rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(res[nm]["observed"], obs[nm][0], rtol=1e-12, atol=1e-12)
    return res, x, y, ok
