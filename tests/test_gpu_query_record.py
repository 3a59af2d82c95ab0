"""Every posterior query of HipContext through the one fixtures record (bplhip_fixtures, bpl/_ffi.py:fixtures), on
the smallest posteriors that use every column of it: S = 10 draws, T = 2 teams, m = 2 fixtures; a plain posterior, a
venue posterior without confederations and one with C = 2.  Per query: (a) no posterior is ESTATE in either form,
(b) the other form's query is ESTATE, empty queries included where the entry takes m = 0, (c) confederations given or
missing against the posterior are EINVAL, (d) the well-formed call returns the documented shapes with finite
values.  Every bad call is rejected on the host, before any device call; the values themselves are the business of
the per-kernel tests."""
import numpy as np
import pytest

from bpl._ffi import BPLHIP_EINVAL, BPLHIP_ESTATE, BplHipError, HipContext

pytestmark = pytest.mark.gpu

S, T, M, G, R = 10, 2, 2, 3, 4
PLAIN, VENUE, WC = {}, {"neutral": [0, 1]}, {"neutral": [0, 1], "conf": ([0, 1], [1, 0])}
FIX = dict(h=[0, 1], a=[1, 0], x=[1, 0], y=[0, 2], b=[0, 1])
EMPTY = dict(h=[], a=[], x=[], y=[], b=[])
LW = np.full((2, S), -np.log(S))

# name -> (the call, {key of the result: (shape, dtype)}; "" for a bare array)
f64, u32 = np.float64, np.uint32
QUERIES = {
    "predict_score_proba": (lambda c, h, a, x, y, b, **kw: c.predict_score_proba(h, a, x, y, **kw), {"": ((M,), f64)}),
    "predict_score_grid": (lambda c, h, a, x, y, b, **kw: c.predict_score_grid(h, a, G, **kw),
                           {"": ((M, G + 1, G + 1), f64)}),
    "predict_score_grid_f32": (lambda c, h, a, x, y, b, **kw: c.predict_score_grid(h, a, G, dtype=np.float32, **kw),
                               {"": ((M, G + 1, G + 1), np.float32)}),
    "loglik_matrix": (lambda c, h, a, x, y, b, **kw: c.loglik_matrix(h, a, x, y, **kw), {"": ((S, M), f64)}),
    "loglik_summary": (lambda c, h, a, x, y, b, **kw: c.loglik_summary(h, a, x, y, **kw),
                       {**{k: ((M,), f64) for k in ("lppd", "mean", "var", "elpd_loo", "pareto_k")},
                        "tail_len": ((M,), np.int32)}),
    "outcome_scores": (lambda c, h, a, x, y, b, **kw: c.outcome_scores(h, a, x, y, G, **kw),
                       {"proba": ((M, 3), f64), "draw_sums": ((S, 3), f64)}),
    "block_loglik": (lambda c, h, a, x, y, b, **kw: c.block_loglik(h, a, x, y, b, 2, **kw), {"": ((2, S), f64)}),
    "weighted_scores": (lambda c, h, a, x, y, b, **kw: c.weighted_scores(h, a, x, y, b, LW, G, **kw),
                        {"elpd": ((M,), f64), "proba": ((M, 3), f64)}),
    "market_summary": (lambda c, h, a, x, y, b, **kw: c.market_summary(h, a, G, np.ones((1, G + 1, G + 1)), (0.5,), **kw),
                       {"mean": ((1, M), f64), "sd": ((1, M), f64), "quantile": ((1, 1, M), f64)}),
    "ppc": (lambda c, h, a, x, y, b, **kw: c.ppc(h, a, h, a, T, G, R, (0, 7), **kw),
            {"score": ((R, G + 1, G + 1), u32), "outcome": ((R, 3), u32), "sums": ((R, 5), np.int64),
             "team": ((R, T, 4), u32)}),
}
TAKES_EMPTY = ("predict_score_proba", "predict_score_grid", "predict_score_grid_f32", "loglik_matrix", "loglik_summary")


@pytest.fixture(scope="module")
def ctxs():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    rs = np.random.RandomState(3)
    tabs = [rs.normal(0.0, 0.2, (S, T)) for _ in range(6)]
    corr = rs.uniform(-0.05, 0.05, S)          # (no clipped tau: every log-likelihood is finite)
    c = {k: HipContext(0) for k in ("fresh", "plain", "venue", "wc")}
    c["plain"].predict_set_posterior(tabs[0], tabs[1], rs.normal(0.3, 0.05, S), corr)
    c["venue"].predict_set_posterior_venue(*tabs, corr)
    c["wc"].predict_set_posterior_venue(*tabs, corr, confederation_strength=rs.normal(0.0, 0.2, (S, 2)))
    yield c
    for x in c.values():
        x.close()


def _code(call, ctx, cols, kw):
    with pytest.raises(BplHipError) as e:
        call(ctx, **cols, **kw)
    return e.value.code


@pytest.mark.parametrize("name", list(QUERIES))
def test_query_through_the_record(ctxs, name):
    call, want = QUERIES[name]
    for kw in (PLAIN, VENUE, WC):                                                  # (a)
        assert _code(call, ctxs["fresh"], FIX, kw) == BPLHIP_ESTATE, kw
    wrong = [("plain", VENUE), ("plain", WC), ("venue", PLAIN), ("wc", PLAIN)]
    for which, kw in wrong:                                                        # (b)
        assert _code(call, ctxs[which], FIX, kw) == BPLHIP_ESTATE, (which, kw)
        if name in TAKES_EMPTY:
            kw0 = {k: ([], []) if k == "conf" else [] for k in kw}
            assert _code(call, ctxs[which], EMPTY, kw0) == BPLHIP_ESTATE, (which, kw0)
    assert _code(call, ctxs["venue"], FIX, WC) == BPLHIP_EINVAL                    # (c)
    assert _code(call, ctxs["wc"], FIX, VENUE) == BPLHIP_EINVAL
    for which, kw in (("plain", PLAIN), ("venue", VENUE), ("wc", WC)):             # (d)
        got = call(ctxs[which], **FIX, **kw)
        got = got if isinstance(got, dict) else {"": got}
        assert set(got) == set(want), (which, set(got))
        for k, (shape, dtype) in want.items():
            assert got[k].shape == shape and got[k].dtype == dtype, (which, k, got[k].shape, got[k].dtype)
            if (name, k) == ("loglik_summary", "pareto_k"):
                # S = 10 gives a PSIS tail of M = 2 draws; a tail of at most 4 is not smoothed and its k is
                # +inf by definition
                assert (got[k] == np.inf).all(), (which, got[k])
            else:
                assert np.isfinite(got[k]).all(), (which, k, got[k])
