"""dcl::psis_tail (csrc/dc_loglik.hip.h) on rows the suite chooses: the designed cases of tests/psis_cases.py
through HipContext.psis_weights (psis_rows, one wave per row) against sequential_ref.psis_row, and through
loglik_summary (four waves per workgroup) on a model whose log-likelihood rows follow eight of the designs.
tests/test_psis_cases_host.py shows, without a GPU, that the restatement is accurate to 1e-11 on every case,
that no case is ill-conditioned, and that each edge changes the result.

Gates (DESIGN.md sections 12 and 17): tail_len exactly; pareto_k, ess and log_weights within 1e-9 (1 + |value|);
exact equality where the restatement is infinite; no NaN; every row's weights sum to one within 1e-9."""
import numpy as np
import pytest
from scipy.special import logsumexp

import loglik_ref as LR
import psis_cases as PC
import scores_ref as SR
import sequential_ref as QR

pytestmark = pytest.mark.gpu

GATE = 1e-9
WORST = {}     # (case, quantity) -> the largest error as a fraction of its gate
_SINGLE = {}   # case -> the device's result of the one-row call


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _gate(case, name, got, want, bound):
    """|got - want| <= bound elementwise where want is finite; exact where it is infinite; no NaN."""
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    assert got.shape == want.shape, (case, name, got.shape, want.shape)
    assert not np.isnan(got).any(), (case, name)
    fin = np.isfinite(want)
    np.testing.assert_array_equal(got[~fin], want[~fin], err_msg=f"{case} {name}")
    bound = np.broadcast_to(bound, want.shape)
    err = np.abs(got[fin] - want[fin])
    frac = float((err / bound[fin]).max()) if err.size else 0.0
    WORST[(case, name)] = max(WORST.get((case, name), 0.0), frac)
    print(f"{case} {name}: largest error {err.max() if err.size else 0.0:.3e}, {frac:.3e} of its gate")
    assert (err <= bound[fin]).all(), (case, name, float(err.max()), frac)


def _rel(v):
    return GATE * (1.0 + np.abs(np.where(np.isfinite(v), v, 0.0)))


def _single(ctx, name, row=None, r_eff=1.0):
    if name not in _SINGLE:
        if row is None:
            _, row, r_eff = PC.case(name)
        _SINGLE[name] = ctx.psis_weights(row[None, :], r_eff)
    return _SINGLE[name]


def _check_row(case, lw_got, k_got, ess_got, L_got, ref):
    lw, k, ess, L = ref
    assert int(L_got) == L, (case, int(L_got), L)
    _gate(case, "pareto_k", k_got, k, _rel(np.float64(k)))
    _gate(case, "ess", ess_got, ess, _rel(np.float64(ess)))
    _gate(case, "log_weights", lw_got, lw, _rel(lw))
    if np.isfinite(lw).any():
        total = float(logsumexp(lw_got))
        print(f"{case} logsumexp(log_weights) = {total:.3e}")
        assert abs(total) <= GATE, (case, total)


@pytest.mark.parametrize("name", PC.names())
def test_case_against_restatement(hip_ctx, name):
    out = _single(hip_ctx, name)
    assert out["log_weights"].shape == (1, PC.case(name)[1].size)
    _check_row(name, out["log_weights"][0], out["pareto_k"][0], out["ess"][0], out["tail_len"][0], PC.reference(name))


def test_stacked_call_is_the_single_rows_bit_for_bit(hip_ctx):
    names, R = PC.mixed_call()
    a, b = hip_ctx.psis_weights(R), hip_ctx.psis_weights(R)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key
    assert not np.isnan(a["log_weights"]).any() and not np.isnan(a["pareto_k"]).any() and not np.isnan(a["ess"]).any()
    for i, name in enumerate(names):
        one = _single(hip_ctx, name, R[i])
        for key in a:
            assert a[key][i].tobytes() == one[key][0].tobytes(), (name, key)
    i, j = names.index("constant"), names.index("dead")
    assert a["pareto_k"][i] == 0.0 and a["tail_len"][i] == 0 and abs(a["ess"][i] - PC.S0) <= GATE * (1 + PC.S0)
    np.testing.assert_allclose(a["log_weights"][i], -np.log(PC.S0), rtol=0, atol=1e-15)
    assert a["pareto_k"][j] == np.inf and a["tail_len"][j] == 0 and a["ess"][j] == 0.0
    assert (a["log_weights"][j] == -np.inf).all()
    assert len(set(a["tail_len"].tolist())) >= 6            # neighbouring blocks get unlike rows


def test_draw_permutations(hip_ctx):
    name = "pareto_0.7"                                      # no ties: the draw order decides nothing
    _, row, r_eff = PC.case(name)
    lw, k, ess, L = PC.reference(name)
    for seed in (1, 2, 3):
        perm = np.random.RandomState(seed).permutation(row.size)
        out = hip_ctx.psis_weights(row[perm][None, :], r_eff)
        _check_row(f"{name} permuted", out["log_weights"][0], out["pareto_k"][0], out["ess"][0], out["tail_len"][0],
                   (lw[perm], k, ess, L))


def test_shifted_rows_are_bit_identical(hip_ctx):
    # multiples of 2^-10 in (-8, 0]: adding 2^3 or 2^10 is exact, and so is x = r - max r
    rs = np.random.RandomState(7)
    row = -rs.permutation(8192)[:PC.S0] / 1024.0
    row[np.argmax(row)] = 0.0
    assert np.unique(row).size == PC.S0
    base = hip_ctx.psis_weights(row[None, :])
    assert np.isfinite(base["pareto_k"][0]) and base["tail_len"][0] == PC.M0
    _check_row("dyadic", base["log_weights"][0], base["pareto_k"][0], base["ess"][0], base["tail_len"][0],
               QR.psis_row(row))
    for p in (3, 10):
        shifted = row + 2.0 ** p
        assert ((shifted - 2.0 ** p) == row).all()
        out = hip_ctx.psis_weights(shifted[None, :])
        for key in base:
            assert out[key].tobytes() == base[key].tobytes(), (p, key)


def _close(name, got, ref, tol):
    _gate("two callers", name, got, ref, tol * (1.0 + np.abs(np.where(np.isfinite(ref), ref, 0.0))))


def test_the_two_callers_run_the_same_lines(hip_ctx):
    """loglik_summary (a workgroup of four waves, each with its own LDS slices) and psis_rows (one wave per
    workgroup) on the same eight rows of unlike tail lengths."""
    m, d = PC.two_caller_model()
    ll = m.log_likelihood(d)
    ref = LR.ll_matrix(m, d)
    _close("ll", ll, ref, 1e-12)
    got = m._loglik_summary(d, psis=True, r_eff=1.0)
    want = LR.summary(ref, 1.0)
    for key in ("lppd", "mean", "var"):
        _close(key, got[key], want[key], 1e-10)
    _close("elpd_loo", got["elpd_loo"], want["elpd_loo"], 1e-9)
    _close("pareto_k", got["pareto_k"], want["pareto_k"], 1e-9)
    np.testing.assert_array_equal(got["tail_len"], want["tail_len"])
    np.testing.assert_array_equal(got["tail_len"], LR.summary(ll, 1.0)["tail_len"])
    assert got["tail_len"].tolist() == [PC.reference(n)[3] for n in PC.TWO_CALLER_DESIGNS]
    assert len(set(got["tail_len"][:4].tolist())) > 1 and len(set(got["tail_len"][4:].tolist())) > 1
    # the stored-row kernel on the device's own matrix: (-v) - (-mn) and mn - v are the same IEEE operation
    w = hip_ctx.psis_weights(-ll.T)
    assert w["pareto_k"].tobytes() == got["pareto_k"].tobytes()
    assert w["tail_len"].tobytes() == got["tail_len"].tobytes()
    elpd = logsumexp(w["log_weights"] + ll.T, axis=1)
    _close("lse(lw + ll) against elpd_loo", elpd, got["elpd_loo"], 1e-9)


@pytest.mark.parametrize("kind", ["basic", "wc"])
def test_weights_with_minus_inf_downstream(hip_ctx, kind):
    """weighted_scores under log weights of which 30 % are -inf."""
    lw = _single(hip_ctx, "minus_inf_some")["log_weights"]
    assert np.isneginf(lw).sum() == 77
    m = QR.narrowed(LR.hand_model(kind, S=PC.S0, T=8, seed=3), 0.1)
    d = LR.hand_data(m, n=12, seed=4)
    index = np.zeros(12, dtype=np.int64)
    (positions, device, kw), = m._loglik_groups(d)[0]
    assert positions is None
    out = device().weighted_scores(**kw, block_idx=index.astype(np.int32), log_weights=lw, max_goals=15)
    lh, la = SR.rates(m, d)
    p = SR.draw_probs(lh, la, np.asarray(m.corr_coef, dtype=np.float64), 15)
    elpd, P = QR.weighted(LR.ll_matrix(m, d), p, lw, index)
    _gate(f"downstream {kind}", "elpd", out["elpd"], elpd, _rel(elpd))
    _gate(f"downstream {kind}", "proba", out["proba"], P, 1e-9)


def test_print_worst_errors():
    """The largest error of every gated quantity per case, as a fraction of its gate (profiles/psis/README.md)."""
    for (case, name), frac in sorted(WORST.items()):
        print(f"WORST {case:28s} {name:32s} {frac:.3e}")
    assert all(v <= 1.0 for v in WORST.values())
