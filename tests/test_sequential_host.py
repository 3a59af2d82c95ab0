"""sequential_scores without a GPU: every argument check (made on the host before a device context is
touched), the block relabelling, the running sum and the merge of the dynamic class's gameweek groups, and
the assembly of the result, through a stand-in context defined here that answers from the numpy restatement
(tests/sequential_ref.py); and the restatement against itself on identities that need no device."""
import numpy as np
import pytest
from scipy.special import logsumexp

import loglik_ref as LR
import scores_ref as SR
import sequential_ref as QR
from bpl import compare_scores
from bpl.sequential import SEQ_MAX_BLOCKS, log_ratios, relabel_blocks
from fake_ctx import FakePredictCtx


class FailCtx:
    """A device context that must never be touched."""

    def __getattr__(self, name):
        raise AssertionError(f"device call {name} before the host checks finished")


class SeqCtx(FakePredictCtx):
    """FakePredictCtx plus the three sequential entries, computed by the restatement from the uploaded
    posterior.  `calls` records (entry, fixtures)."""

    def __init__(self):
        self.calls = []

    def _parts(self, home_idx, away_idx, home_goals, away_goals, neutral, conf):
        h, a = np.asarray(home_idx, int), np.asarray(away_idx, int)
        eh, ea = self._log_rates(h, a, neutral, conf)
        lh, la = np.exp(eh), np.exp(ea)
        return lh, la, LR.ll_from_rates(lh, la, home_goals, away_goals, self.cc)

    def block_loglik(self, home_idx, away_idx, home_goals, away_goals, block_idx, n_blocks, neutral=None, conf=None):
        self.calls.append(("block_loglik", len(home_idx)))
        assert np.asarray(block_idx).dtype == np.int32
        _, _, ll = self._parts(home_idx, away_idx, home_goals, away_goals, neutral, conf)
        return QR.block_sums(ll, np.asarray(block_idx), n_blocks)

    def psis_weights(self, log_ratios, r_eff=1.0):
        self.calls.append(("psis_weights", np.shape(log_ratios)[0]))
        return QR.weights(np.asarray(log_ratios), r_eff)

    def weighted_scores(self, home_idx, away_idx, home_goals, away_goals, block_idx, log_weights, max_goals,
                        neutral=None, conf=None):
        self.calls.append(("weighted_scores", len(home_idx)))
        lh, la, ll = self._parts(home_idx, away_idx, home_goals, away_goals, neutral, conf)
        p = SR.draw_probs(lh, la, self.cc, max_goals)
        elpd, P = QR.weighted(ll, p, np.asarray(log_weights), np.asarray(block_idx))
        return {"elpd": elpd, "proba": P}


KEYS = {"kind", "n", "outcome", "outcome_proba", "elpd_i", "elpd", "block", "block_values", "n_block", "pareto_k",
        "ess", "tail_len", "reliable", "refit_from", "elpd_block"} | {
            f"{name}{suffix}" for name in ("log_score", "brier", "rps") for suffix in ("", "_i", "_se", "_block")}


@pytest.mark.parametrize("kind", LR.KINDS)
def test_result_assembly_against_the_restatement(kind):
    m = QR.narrowed(LR.hand_model(kind, S=65, T=6, seed=1), 0.1)
    d = LR.hand_data(m, n=30, seed=2)
    labels = np.array([40, -3, 7, 7000, 12])
    block = labels[np.random.RandomState(3).randint(0, 5, 30)]
    block[:5] = labels                                    # every label is used
    m._predict_ctx = ctx = SeqCtx()
    r = m.sequential_scores(d, block, max_goals=7, return_weights=True)
    groups = len(np.unique(d["gameweek"])) if kind == "dynamic" else 1
    assert [c[0] for c in ctx.calls] == ["block_loglik"] * groups + ["psis_weights"] + ["weighted_scores"] * groups
    assert sum(c[1] for c in ctx.calls if c[0] == "block_loglik") == 30
    assert set(r) == KEYS | {"log_weights"}
    assert set(m.sequential_scores(d, block, max_goals=7)) == KEYS
    assert r["kind"] == "scores" and r["n"] == 30
    assert r["outcome"].dtype == np.uint8 and r["block"].dtype == np.int64 and r["tail_len"].dtype == np.int32
    np.testing.assert_array_equal(r["block_values"], [-3, 7, 12, 40, 7000])
    np.testing.assert_array_equal(r["block_values"][r["block"]], block)
    assert r["log_weights"].shape == (5, 65) and r["outcome_proba"].shape == (30, 3)
    for k in ("pareto_k", "ess", "tail_len", "n_block", "reliable", "elpd_block", "rps_block"):
        assert r[k].shape == (5,), k
    assert r["n_block"].sum() == 30 and r["reliable"].dtype == np.bool_
    # the host side adds nothing to the restatement beyond rounding (the groups' sums are added in another order)
    ref = QR.scores(m, d, block, G=7)
    for k in KEYS - {"kind", "refit_from"}:
        np.testing.assert_allclose(r[k], ref[k], rtol=1e-9, atol=1e-12, err_msg=k)
    np.testing.assert_allclose(r["log_weights"], ref["log_weights"], rtol=1e-9, atol=1e-9)
    assert r["refit_from"] == ref["refit_from"]
    assert abs(r["elpd"] - r["elpd_i"].sum()) < 1e-12
    np.testing.assert_allclose(np.exp(r["log_weights"]).sum(axis=1), 1.0, rtol=0, atol=1e-12)
    # block 0 is the frozen forecast
    assert r["pareto_k"][0] == 0.0 and r["tail_len"][0] == 0 and abs(r["ess"][0] - 65) < 1e-9
    frozen = SR.scores(m, d, 7)
    first = r["block"] == 0
    np.testing.assert_allclose(r["outcome_proba"][first], frozen["outcome_proba"][first], rtol=0, atol=1e-12)
    out = compare_scores({"frozen": {k: v for k, v in frozen.items() if k != "p_draws"} | {"kind": "scores"},
                          "updated": r})
    assert set(out) == {"frozen", "updated"}


def test_refit_from_and_threshold():
    m = QR.narrowed(LR.hand_model("basic", S=129, T=6, seed=5), 0.1)
    d = LR.hand_data(m, n=48, seed=6)
    block = np.repeat(np.arange(8) * 10 + 3, 6)
    m._predict_ctx = SeqCtx()
    r = m.sequential_scores(d, block)
    k = r["pareto_k"]
    assert np.isfinite(k).all() and k[0] == 0.0 and k[1:].min() > 0.0
    low = m.sequential_scores(d, block, k_threshold=0.5 * float(k[1:].min()))   # block 0 (k = 0) stays reliable
    assert low["refit_from"] == 13 and low["reliable"].tolist() == [True] + [False] * 7
    high = m.sequential_scores(d, block, k_threshold=float(k.max()) + 0.5)
    assert high["refit_from"] is None and high["reliable"].all()
    mid = float(np.sort(k)[4])
    r = m.sequential_scores(d, block, k_threshold=mid)
    first = int(np.nonzero(k > mid)[0][0])
    assert r["refit_from"] == block[6 * first] and isinstance(r["refit_from"], int)
    np.testing.assert_array_equal(r["reliable"], k <= mid)


def test_relabel_blocks():
    values, index = relabel_blocks([5, 2, 9, 2, 5], 5)
    np.testing.assert_array_equal(values, [2, 5, 9])
    np.testing.assert_array_equal(index, [1, 0, 2, 0, 1])
    assert index.dtype == np.int64
    values, index = relabel_blocks(np.array([3.0, -1.0]), 2)            # integer-valued floats pass
    np.testing.assert_array_equal(values, [-1, 3])
    np.testing.assert_array_equal(index, [1, 0])
    for bad in ([1, 2], [1.5, 2, 3], [np.nan, 1, 2], ["a", "b", "c"], [True, False, True], [[1, 2, 3]], None):
        with pytest.raises((ValueError, TypeError)):
            relabel_blocks(bad, 3)
    with pytest.raises(ValueError):
        relabel_blocks(np.arange(SEQ_MAX_BLOCKS + 1), SEQ_MAX_BLOCKS + 1)
    assert relabel_blocks(np.arange(SEQ_MAX_BLOCKS), SEQ_MAX_BLOCKS)[0].size == SEQ_MAX_BLOCKS


def test_log_ratios_running_sum():
    A = np.array([[1.0, 2.0], [0.5, -np.inf], [3.0, 1.0], [9.0, 9.0]])
    R = log_ratios(A)
    np.testing.assert_array_equal(R, [[0.0, 0.0], [1.0, 2.0], [1.5, -np.inf], [4.5, -np.inf]])
    np.testing.assert_array_equal(log_ratios(A[:1]), [[0.0, 0.0]])
    np.testing.assert_array_equal(R, QR.log_ratios(A))
    assert not np.isnan(R).any()


def _raises(m, data, block, **kwargs):
    m._predict_ctx = FailCtx()
    with pytest.raises(ValueError):
        m.sequential_scores(data, block, **kwargs)


@pytest.mark.parametrize("kind", LR.KINDS)
def test_argument_checks_run_on_the_host(kind):
    m = LR.hand_model(kind, S=16)
    good = LR.hand_data(m, n=6)
    gw = [1, 1, 2, 2, 3, 3]
    _raises(m, {k: [] for k in good}, [])                   # no fixture
    for g in (-1, 64, 2.0, True, None, "15"):
        _raises(m, good, gw, max_goals=g)
    for r in (0.0, -1.0, np.inf, np.nan, "1", None, True):
        _raises(m, good, gw, r_eff=r)
    for t in (np.inf, -np.inf, np.nan, "0.7", None, True):
        _raises(m, good, gw, k_threshold=t)
    for b in (gw[:-1], gw + [4], [1.5] + gw[1:], ["a"] * 6, [np.nan] + gw[1:], [True] * 6):
        _raises(m, good, b)
    _raises(m, dict(good, home_team=["nope"] + list(good["home_team"][1:])), gw)
    _raises(m, dict(good, home_goals=[256] + list(good["home_goals"][1:])), gw)
    d = dict(good)
    d.pop("away_goals")
    _raises(m, d, gw)


def test_draw_and_block_limits_run_on_the_host():
    big = LR.hand_model("neutral", S=65537, T=2)
    _raises(big, LR.hand_data(big, n=2), [0, 1])
    m = LR.hand_model("basic", S=30000, T=2)
    _raises(m, LR.hand_data(m, n=2), [0, 1], r_eff=0.001)   # a PSIS tail beyond the device's limit
    m = LR.hand_model("basic", S=4, T=4)
    n = SEQ_MAX_BLOCKS + 1
    _raises(m, LR.hand_data(m, n=n), np.arange(n))


# ---- the restatement against itself
def test_ref_one_block_is_the_frozen_forecast():
    m = QR.narrowed(LR.hand_model("wc", S=50, T=6, seed=7), 0.1)
    d = LR.hand_data(m, n=12, seed=8)
    r = QR.scores(m, d, np.zeros(12, int), G=9)
    frozen = SR.scores(m, d, 9)
    np.testing.assert_allclose(r["outcome_proba"], frozen["outcome_proba"], rtol=0, atol=1e-14)
    np.testing.assert_allclose(r["elpd_i"], LR.summary(r["ll"], psis_on=False)["lppd"], rtol=0, atol=1e-12)
    assert r["pareto_k"].tolist() == [0.0] and abs(r["ess"][0] - 50) < 1e-10 and r["tail_len"].tolist() == [0]


def test_ref_second_block_weights_are_the_psis_of_the_first_fixture():
    m = QR.narrowed(LR.hand_model("basic", S=64, T=4, seed=9), 0.3)
    d = LR.hand_data(m, n=2, seed=10)
    r = QR.scores(m, d, [0, 1])
    _, k, L, lw = LR.psis(-r["ll"][:, 0], return_lw=True)
    np.testing.assert_array_equal(r["log_weights"][1], lw)
    assert r["pareto_k"][1] == k and r["tail_len"][1] == L
    assert abs(r["elpd_i"][1] - logsumexp(lw + r["ll"][:, 1])) < 1e-13


def test_ref_special_cases():
    lw, k, ess, L = QR.psis_row(np.full(7, -3.25))
    np.testing.assert_allclose(lw, -np.log(7), rtol=0, atol=1e-15)
    assert (k, L) == (0.0, 0) and abs(ess - 7) < 1e-12
    lw, k, ess, L = QR.psis_row(np.array([-1.0]))                        # one draw
    assert lw.tolist() == [0.0] and (k, ess, L) == (0.0, 1.0, 0)
    lw, k, ess, L = QR.psis_row(np.full(5, -np.inf))                     # a dead block
    assert (lw == -np.inf).all() and (k, ess, L) == (np.inf, 0.0, 0)
    r = np.random.RandomState(0).normal(0, 1, 40)
    r[3] = -np.inf                                                       # one draw ruled out: weight 0
    lw, k, ess, L = QR.psis_row(r)
    assert lw[3] == -np.inf and np.isfinite(np.delete(lw, 3)).all() and not np.isnan(k) and ess > 1
    assert abs(logsumexp(lw)) < 1e-12
