"""The designed diagnostics series (tests/diagnostics_cases.py) through HipContext.mcmc_diagnostics against the numpy
restatement (tests/diagnostics_ref.py).  The gate is the one of tests/test_gpu_diagnostics.py: the same NaN pattern
and 1e-9 (1 + |restatement|) for all seven statistics.  What makes it meaningful -- that every case reaches the branch
it is built for, that the restatement agrees with 50-digit arithmetic and that each rule moves its case -- is shown
without a GPU in tests/test_diagnostics_cases_host.py."""
import functools

import numpy as np
import pytest

import bpl
import diagnostics_cases as DC
import diagnostics_ref as R

pytestmark = pytest.mark.gpu
GATE = 1e-9
RANK_STATS = ("rhat", "ess_bulk", "ess_tail")


def _errors(got, ref, label, j=0):
    """The error / (1 + |ref|) per statistic of column j of a device result against one restatement dict."""
    worst = {}
    for nm in R.STATS:
        g, r = float(np.asarray(got[nm]).ravel()[j]), float(ref[nm])
        assert np.isnan(g) == np.isnan(r), (label, nm, g, r)
        worst[nm] = 0.0 if np.isnan(r) else abs(g - r) / (1.0 + abs(r))
    print(f"{label}: error / (1 + |ref|): " + ", ".join(f"{nm} {e:.2e}" for nm, e in worst.items()))
    return worst


def _column(name):
    return DC.case(name).values.reshape(-1, 1)


def _one_quantity(S, NQ):
    return S * (16 if S <= DC.LDS_DRAWS else 28) + max(NQ, 1) * 8 + 8   # a single quantity (include/bplhip.h)


def _same_bits(a, b, label, cols_a=None, cols_b=None):
    for nm in R.STATS:
        x = a[nm] if cols_a is None else a[nm][cols_a]
        y = b[nm] if cols_b is None else b[nm][cols_b]
        assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), (label, nm)


@functools.lru_cache(maxsize=None)
def _alone(hip_ctx, name):
    c = DC.case(name)
    return hip_ctx.mcmc_diagnostics(_column(name), c.C, c.quantiles)


@pytest.mark.parametrize("name", DC.names())
def test_every_case_matches_the_restatement(hip_ctx, name):
    ref = DC.reference(name)
    assert ref["margin"] >= DC.MARGIN or name in DC.MARGIN_EXEMPT
    worst = _errors(_alone(hip_ctx, name), ref, name)
    for nm in (RANK_STATS if name in DC.RANK_ONLY else R.STATS):
        assert worst[nm] <= GATE, (name, nm, worst[nm])


@pytest.mark.parametrize("key", list(DC.stacks()), ids=lambda k: f"C{k[0]}-N{k[1]}-NQ{len(k[2])}")
def test_stacked_columns_are_the_single_calls_bit_for_bit(hip_ctx, key):
    C, N, quantiles = key
    names = DC.stacks()[key]
    v = np.concatenate([_column(n) for n in names], axis=1)
    a = hip_ctx.mcmc_diagnostics(v, C, quantiles)
    for j, n in enumerate(names):
        _same_bits(a, _alone(hip_ctx, n), n, cols_a=slice(j, j + 1))
    _same_bits(a, hip_ctx.mcmc_diagnostics(v, C, quantiles), "repeated")
    _same_bits(a, hip_ctx.mcmc_diagnostics(v[:, ::-1], C, quantiles), "reversed", cols_b=slice(None, None, -1))
    one = _one_quantity(2 * C * (N // 2), len(quantiles))
    _same_bits(a, hip_ctx.mcmc_diagnostics(v, C, quantiles, workspace_bytes=one), "one quantity per chunk")


@pytest.mark.parametrize("name", ["lds_edge", "ws_edge", "two_valued_workspace", "nq0", "nq16"])
def test_a_workspace_for_exactly_one_quantity(hip_ctx, name):
    c = DC.case(name)
    v = np.concatenate([_column(name), -_column(name)], axis=1)
    a = hip_ctx.mcmc_diagnostics(v, c.C, c.quantiles)
    b = hip_ctx.mcmc_diagnostics(v, c.C, c.quantiles, workspace_bytes=_one_quantity(2 * c.C * (c.N // 2), len(c.quantiles)))
    _same_bits(a, b, name)
    _same_bits(a, _alone(hip_ctx, name), name, cols_a=slice(0, 1))


def test_degenerate_columns_do_not_touch_their_neighbours(hip_ctx):
    """Columns in the manner of chains_constant (W = 0), of max_tie_tail_nan (one constant indicator), a constant
    quantity and one with a NaN, between continuous columns of the same shape."""
    C, N = 2, 128
    rs = np.random.RandomState(77)
    healthy = [DC.continuous(rs, C, N).reshape(-1, 1) for _ in range(4)]
    w0 = np.repeat(np.arange(2.0 * C), N // 2).reshape(-1, 1)
    assert (R.split_chains(w0[:, 0], C) == np.arange(2.0 * C)[:, None]).all()
    bad = healthy[1].copy()
    bad[200, 0] = np.nan
    odd = [w0, _column("max_tie_tail_nan"), np.full((C * N, 1), 0.1), bad]
    v = np.concatenate([healthy[0], odd[0], healthy[1], odd[1], odd[2], healthy[2], odd[3], healthy[3]], axis=1)
    got = hip_ctx.mcmc_diagnostics(v, C, DC.DEFAULT_Q)
    ref = R.diagnose(v, C, DC.DEFAULT_Q)
    nan = {j: sorted(nm for nm in R.STATS if np.isnan(ref[nm][j])) for j in range(v.shape[1])}
    assert nan[1] == ["ess_tail", "rhat"] and nan[3] == ["ess_tail"] and len(nan[4]) == 5 and len(nan[6]) == 7
    for j in range(v.shape[1]):
        worst = _errors(got, {nm: ref[nm][j] for nm in R.STATS}, f"column {j}", j)
        assert max(worst.values()) <= GATE, (j, worst)
    only = hip_ctx.mcmc_diagnostics(np.concatenate(healthy, axis=1), C, DC.DEFAULT_Q)
    _same_bits(got, only, "healthy columns", cols_a=[0, 2, 5, 7])
    _same_bits(got, _alone(hip_ctx, "max_tie_tail_nan"), "max_tie_tail_nan", cols_a=slice(3, 4))


def test_relabelling_the_chains_and_negating_the_draws(hip_ctx):
    C, N = 5, 101
    x = DC.continuous(np.random.RandomState(78), C, N)
    base, ref = hip_ctx.mcmc_diagnostics(x.reshape(-1, 1), C, DC.DEFAULT_Q), R.diagnose_one(x.ravel(), C)
    assert ref["margin"] >= DC.MARGIN
    assert max(_errors(base, ref, "relabelling: the base").values()) <= GATE
    for shift in (1, 3):
        got = hip_ctx.mcmc_diagnostics(np.roll(x, shift, axis=0).reshape(-1, 1), C, DC.DEFAULT_Q)
        worst = _errors(got, {nm: base[nm][0] for nm in R.STATS}, f"chains rolled by {shift}")
        assert max(worst.values()) <= GATE, worst
    neg = hip_ctx.mcmc_diagnostics(-x.reshape(-1, 1), C, DC.DEFAULT_Q)
    want = {nm: (-base[nm][0] if nm == "mean" else base[nm][0]) for nm in R.STATS}
    worst = _errors(neg, want, "negated")
    assert max(worst.values()) <= GATE, worst


def test_nq16_one_quantile_at_a_time(hip_ctx):
    """ess_tail is a minimum, which hides all but one quantile of a call: each of the sixteen on its own."""
    c = DC.case("nq16")
    tails = []
    for i, q in enumerate(c.quantiles):
        ref = R.diagnose_one(c.values, c.C, (q,))
        assert ref["margin"] >= DC.MARGIN
        got = hip_ctx.mcmc_diagnostics(_column("nq16"), c.C, (q,))
        worst = _errors(got, ref, f"nq16 quantile {i} (g = {DC.facts('nq16').quant[i]['g']:.6g})")
        assert max(worst.values()) <= GATE, (i, worst)
        tails.append(got["ess_tail"][0])
    assert min(tails) == _alone(hip_ctx, "nq16")["ess_tail"][0]


def test_no_quantiles_through_the_public_function(hip_ctx):
    c = DC.case("nq0")
    out = bpl.mcmc_diagnostics(c.values, c.C, quantiles=())
    alone = _alone(hip_ctx, "nq0")
    assert np.isnan(out["ess_tail"]) and out["ess_tail"].shape == ()
    for nm in R.STATS:
        assert np.asarray(out[nm]).tobytes() == alone[nm].tobytes(), nm
        assert nm == "ess_tail" or np.isfinite(out[nm])
