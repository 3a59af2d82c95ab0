"""sequential_scores on the device (csrc/dc_sequential.hip.h, bpl/sequential.py) against the numpy
restatement (tests/sequential_ref.py: the full log-likelihood matrix, a full sort, the full scoreline grids)
for the five predictor classes; the refit flag; identities against forecast_scores and loo; shape edges; a
clipped tau and a dead block; the dynamic class's groups; determinism and the library's own errors.

Gates (DESIGN.md sections 12, 15 and 17): block sums within 1e-12 sum_n (1 + |ll|) per (block, draw); tail_len
exactly; lw, k, ess and elpd_i within 1e-9 (1 + |value|); outcome_proba within 1e-9 absolute (the weights carry
the 1e-9); Brier and RPS within 1e-8; a log score within 1e-9 / p + 1e-9.  The posteriors are hand models
narrowed about their mean (sequential_ref.narrowed): prior-wide ones collapse onto one draw at the first update."""
import numpy as np
import pytest

import loglik_ref as LR
import sequential_ref as QR
from bpl import _ffi, compare_scores
from bpl._ffi import BPLHIP_EINVAL, BPLHIP_ESTATE, BplHipError, HipContext

pytestmark = pytest.mark.gpu

WORST = {}   # the largest error of each gated quantity, as a fraction of its gate (printed by every check)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _gate(name, got, want, bound):
    """|got - want| <= bound elementwise where want is finite; exact where it is infinite."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert not np.isnan(got).any(), name
    fin = np.isfinite(want)
    np.testing.assert_array_equal(got[~fin], want[~fin], err_msg=name)
    bound = np.broadcast_to(bound, want.shape)
    err = np.abs(got[fin] - want[fin])
    frac = float((err / bound[fin]).max()) if err.size else 0.0
    WORST[name] = max(WORST.get(name, 0.0), frac)
    print(f"{name}: largest error {err.max() if err.size else 0.0:.3e}, {frac:.3e} of its gate")
    assert (err <= bound[fin]).all(), (name, float(err.max()), frac)


def _check(m, d, block, G=15, r_eff=1.0, **kwargs):
    """sequential_scores against the restatement, every gate; returns (result, restatement)."""
    got = m.sequential_scores(d, block, r_eff=r_eff, max_goals=G, return_weights=True, **kwargs)
    ref = QR.scores(m, d, block, r_eff=r_eff, G=G, **kwargs)
    for k, v in got.items():
        if k not in ("kind", "refit_from"):
            assert not np.isnan(np.asarray(v, dtype=np.float64)).any(), k
    assert got["n"] == ref["n"] and got["kind"] == "scores"
    for k in ("outcome", "block", "block_values", "n_block"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    np.testing.assert_array_equal(got["tail_len"], ref["tail_len"])
    rel = lambda v: 1e-9 * (1.0 + np.abs(np.where(np.isfinite(v), v, 0.0)))
    for k in ("pareto_k", "ess", "elpd_i", "elpd_block"):
        _gate(k, got[k], ref[k], rel(ref[k]))
    _gate("log_weights", got["log_weights"], ref["log_weights"], rel(ref["log_weights"]))
    _gate("outcome_proba", got["outcome_proba"], ref["outcome_proba"], 1e-9)
    for name in ("brier", "rps"):
        _gate(name + "_i", got[name + "_i"], ref[name + "_i"], 1e-8)
        _gate(name + "_block", got[name + "_block"], ref[name + "_block"], 1e-8)
        assert abs(got[name] - ref[name]) <= 1e-8 and abs(got[name + "_se"] - ref[name + "_se"]) <= 1e-8
    o = ref["outcome"].astype(np.int64)
    P_o = ref["outcome_proba"][np.arange(o.size), o]
    with np.errstate(divide="ignore"):
        _gate("log_score_i", got["log_score_i"], ref["log_score_i"], 1e-9 / P_o + 1e-9)
    if np.isfinite(ref["elpd"]):
        assert abs(got["elpd"] - ref["elpd"]) <= 1e-9 * (1.0 + np.abs(ref["elpd_i"])).sum()
    else:
        assert got["elpd"] == ref["elpd"]
    np.testing.assert_array_equal(got["reliable"], ref["reliable"])
    assert got["refit_from"] == ref["refit_from"]
    return got, ref


def _block_sums(m, d, index, B):
    groups, n = m._loglik_groups(d)
    S = m._loglik_draws()
    A = np.zeros((B, S))
    for positions, device, kw in groups:
        at = slice(None) if positions is None else positions
        A += device().block_loglik(**kw, block_idx=index[at].astype(np.int32), n_blocks=B)
    return A


def _first_shape(kind):
    m = QR.narrowed(LR.hand_model(kind, S=257, T=8, seed=3), 0.1)
    d = LR.hand_data(m, n=40, seed=4)
    return m, d, np.repeat(np.arange(10), 4)


@pytest.mark.parametrize("G", [1, 15])
@pytest.mark.parametrize("kind", LR.KINDS)
def test_all_classes_against_restatement(kind, G):
    m, d, block = _first_shape(kind)
    got, ref = _check(m, d, block, G)
    # the comparison is not one of degenerate weights
    k, ess, L = ref["pareto_k"][1:], ref["ess"][1:], ref["tail_len"][1:]
    assert np.isfinite(k).all() and (ess >= 10).all(), (k, ess)
    assert 2 * np.count_nonzero(L > 0) >= L.size
    if G == 15:
        A = _block_sums(m, d, ref["block"], 10)
        bound = 1e-12 * np.stack([(1.0 + np.abs(ref["ll"][:, ref["block"] == b])).sum(axis=1) for b in range(10)])
        _gate("block_sums", A, ref["block_sums"], bound)
    print("worst so far, as fractions of the gates:", {k: f"{v:.2e}" for k, v in WORST.items()})


def _second_shape(kind):
    m = QR.narrowed(LR.hand_model(kind, S=513, T=8, seed=3), 0.1)
    d = LR.hand_data(m, n=60, seed=4)
    labels = np.array([3, 4, 9, 10, 17, 30, 31, 44, 58, 59, 80, 1000])   # non-contiguous
    perm = np.random.RandomState(5).permutation(60)                      # the fixtures are shuffled
    d = {k: [v[i] for i in perm] for k, v in d.items()}
    return m, d, labels[np.repeat(np.arange(12), 5)[perm]]


@pytest.mark.parametrize("kind", LR.KINDS)
def test_refit_flag(kind):
    m, d, block = _second_shape(kind)
    got, ref = _check(m, d, block)
    k, labels = ref["pareto_k"], ref["block_values"]
    stale = np.nonzero(k > 0.7)[0]
    assert got["refit_from"] == (int(labels[stale[0]]) if stale.size else None)
    assert (got["refit_from"] is None) == (kind == "dynamic")
    np.testing.assert_array_equal(got["reliable"], k <= 0.7)
    assert k[1:].min() > 0.0
    low = m.sequential_scores(d, block, k_threshold=0.5 * float(k[1:].min()))
    assert low["refit_from"] == int(labels[1]) and low["reliable"][0] and not low["reliable"][1:].any()
    high = m.sequential_scores(d, block, k_threshold=float(k.max()) + 1.0)
    assert high["refit_from"] is None and high["reliable"].all()
    # the fixtures in another order: the same per-fixture values within the gates
    again = np.random.RandomState(6).permutation(60)
    d2 = {key: [v[i] for i in again] for key, v in d.items()}
    other = m.sequential_scores(d2, block[again])
    _gate("reordered elpd_i", other["elpd_i"], ref["elpd_i"][again], 1e-9 * (1 + np.abs(ref["elpd_i"][again])))
    _gate("reordered outcome_proba", other["outcome_proba"], ref["outcome_proba"][again], 1e-9)
    _gate("reordered pareto_k", other["pareto_k"], k, 1e-9 * (1 + np.abs(k)))
    np.testing.assert_array_equal(other["block"], ref["block"][again])


@pytest.mark.parametrize("kind", LR.KINDS)
def test_one_block_is_forecast_scores_and_lppd(kind):
    m = QR.narrowed(LR.hand_model(kind, S=300, T=8, seed=7), 0.2)
    d = LR.hand_data(m, n=70, seed=8)
    got = m.sequential_scores(d, np.full(70, 5))
    frozen = m.forecast_scores(d)
    err = np.abs(got["outcome_proba"] - frozen["outcome_proba"]).max()
    print(f"{kind}: one block against forecast_scores {err:.3e}")
    assert err <= 1e-12
    lppd = m.loo(d)["lppd_i"]
    fin = np.isfinite(lppd)
    np.testing.assert_array_equal(got["elpd_i"][~fin], lppd[~fin])
    err = np.abs(got["elpd_i"][fin] - lppd[fin]).max()
    print(f"{kind}: one block against loo's lppd_i {err:.3e}")
    assert err <= 1e-10
    assert got["pareto_k"].tolist() == [0.0] and got["tail_len"].tolist() == [0]
    assert abs(got["ess"][0] - 300) <= 1e-9 * 301 and got["refit_from"] is None
    np.testing.assert_array_equal(got["block_values"], [5])


def test_two_blocks_of_one_fixture():
    m = QR.narrowed(LR.hand_model("basic", S=64, T=4, seed=9), 0.3)
    d = LR.hand_data(m, n=2, seed=10)
    got = m.sequential_scores(d, [0, 1], return_weights=True)
    ll = LR.ll_matrix(m, d)
    _, k, L, lw = LR.psis(-ll[:, 0], return_lw=True)     # PSIS of r = ll[:, 0]: loglik_ref.psis takes ll = -r
    assert np.isfinite(k) and L > 4                      # the smoothing ran
    _gate("second fixture's lw", got["log_weights"][1], lw, 1e-9 * (1 + np.abs(lw)))
    assert got["tail_len"][1] == L and abs(got["pareto_k"][1] - k) <= 1e-9 * (1 + abs(k))
    assert got["pareto_k"][0] == 0.0 and (got["log_weights"][0] == -np.log(64.0)).all()


@pytest.mark.parametrize("S", [1, 2, 5, 63, 64, 65, 257])
@pytest.mark.parametrize("kind", ["basic", "wc"])
def test_draw_count_edges(kind, S):
    # S - 1 < M, L <= 4, a partial and a second lane round, a second draw tile and strip
    m = QR.narrowed(LR.hand_model(kind, S=S, T=6, seed=S), 0.1)
    d = LR.hand_data(m, n=12, seed=S + 1)
    got, _ = _check(m, d, np.repeat([2, 4, 6], 4))
    if S == 1:
        assert got["pareto_k"].tolist() == [0.0] * 3 and got["ess"].tolist() == [1.0] * 3
        assert (got["log_weights"] == 0.0).all()


@pytest.mark.parametrize("sizes", [(1, 1), (63, 2), (64, 64), (65, 1), (1, 129), (128, 3)])
@pytest.mark.parametrize("kind", ["basic", "wc"])
def test_block_size_edges(kind, sizes):
    # block sizes on either side of the chunk size of 64 fixtures (1, 63, 64, 65, 128, 129: one, two, three chunks)
    m = QR.narrowed(LR.hand_model(kind, S=70, T=6, seed=31), 0.05)
    n = sum(sizes)
    d = LR.hand_data(m, n=n, seed=32)
    block = np.repeat(np.arange(len(sizes)), sizes)
    got, ref = _check(m, d, block[np.random.RandomState(33).permutation(n)])
    index = ref["block"]
    A = _block_sums(m, d, index, len(sizes))
    bound = 1e-12 * np.stack([(1.0 + np.abs(ref["ll"][:, index == b])).sum(axis=1) for b in range(len(sizes))])
    _gate("block_sums", A, ref["block_sums"], bound)


@pytest.mark.parametrize("B", [1, 2, 65])
@pytest.mark.parametrize("kind", ["basic", "wc"])
def test_block_count_edges(kind, B):
    m = QR.narrowed(LR.hand_model(kind, S=130, T=6, seed=41), 0.03)
    d = LR.hand_data(m, n=2 * B, seed=42)
    _check(m, d, np.repeat(np.arange(B) * 7 - 20, 2))


@pytest.mark.parametrize("G", [0, 63])
@pytest.mark.parametrize("kind", ["basic", "wc"])
def test_max_goals_edges(kind, G):
    m = QR.narrowed(LR.hand_model(kind, S=65, T=6, seed=51), 0.1)
    d = LR.hand_data(m, n=9, seed=52)
    got, _ = _check(m, d, np.repeat([0, 1, 2], 3), G)
    if G == 0:
        assert (got["outcome_proba"][:, [0, 2]] == 0.0).all() and (got["outcome_proba"][:, 1] > 0.0).all()


def _clipped_model(all_draws):
    m = QR.narrowed(LR.hand_model("basic", S=64, T=4, seed=2), 0.1)
    m.corr_coef = np.full(64, 5.0) if all_draws else np.where(np.arange(64) == 7, 5.0, 0.01)   # 1 - rho < 0: no 1-1
    d = {"home_team": ["t00", "t01", "t02", "t03", "t00", "t02"], "away_team": ["t01", "t02", "t03", "t00", "t02", "t01"],
         "home_goals": [2, 1, 3, 0, 2, 1], "away_goals": [0, 1, 1, 2, 2, 0]}
    return m, d, [0, 1, 2, 2, 3, 3]


def test_clipped_tau_draw_gets_weight_zero():
    m, d, block = _clipped_model(False)
    got, ref = _check(m, d, block)
    lw = got["log_weights"]
    assert np.isfinite(lw[:2]).all()                      # the 1-1 is in block 1: blocks 0 and 1 do not see it
    assert (lw[2:, 7] == -np.inf).all()                   # afterwards draw 7 has weight exactly 0
    assert np.isfinite(np.delete(lw[2:], 7, axis=1)).all() and np.isfinite(got["pareto_k"]).sum() >= 2
    assert (got["ess"][2:] > 0).all() and np.isfinite(got["elpd_i"][2:]).all()
    assert got["elpd_i"][1] > -np.inf                     # the 1-1 itself is scored by the 63 other draws


def test_dead_block():
    m, d, block = _clipped_model(True)
    got, _ = _check(m, d, block)
    dead = np.array([False, False, True, True])
    assert (got["log_weights"][dead] == -np.inf).all() and np.isfinite(got["log_weights"][~dead]).all()
    assert (got["pareto_k"][dead] == np.inf).all() and (got["ess"][dead] == 0.0).all()
    assert (got["tail_len"][dead] == 0).all()
    late = np.asarray(block) >= 2
    assert (got["elpd_i"][late] == -np.inf).all() and (got["outcome_proba"][late] == 0.0).all()
    assert got["elpd_i"][1] == -np.inf and got["elpd"] == -np.inf   # the 1-1 has no mass under any draw
    assert got["refit_from"] == 2 and not got["reliable"][2:].any()
    assert got["log_score"] == -np.inf and got["log_score_se"] == np.inf


def test_dynamic_groups_and_blocks_cross():
    # several gameweek groups feed one block, and one gameweek is split over two blocks
    m = QR.narrowed(LR.hand_model("dynamic", S=200, T=8, seed=15, G=4), 0.1)
    d = LR.hand_data(m, n=48, seed=16)
    gw = np.asarray(d["gameweek"])
    block = np.where(gw <= 1, 10, np.where(gw == 2, 20, 30))
    three = np.nonzero(gw == 3)[0]
    block[three[: three.size // 2]] = 20                 # gameweek 3 is split over blocks 20 and 30
    assert len(set(gw[block == 10])) == 2 and set(block[gw == 3]) == {20, 30}
    _check(m, d, block)


def test_two_calls_are_bit_identical():
    m = QR.narrowed(LR.hand_model("wc", S=1000, T=12, seed=13), 0.1)
    d = LR.hand_data(m, n=300, seed=14)
    block = np.random.RandomState(15).randint(0, 9, 300)
    a = m.sequential_scores(d, block, return_weights=True)
    b = m.sequential_scores(d, block, return_weights=True)
    for k in a:
        if k not in ("kind", "n", "refit_from"):
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    assert a["refit_from"] == b["refit_from"]


class _FailCtx:
    def __getattr__(self, name):
        raise AssertionError(f"device call {name} before the host checks finished")


def test_host_errors_come_before_any_device_call():
    m = LR.hand_model("basic", S=16)
    d = LR.hand_data(m, n=6)
    m._predict_ctx = _FailCtx()
    for kwargs in ({"max_goals": 64}, {"r_eff": 0.0}, {"k_threshold": np.nan}):
        with pytest.raises(ValueError):
            m.sequential_scores(d, [0, 0, 1, 1, 2, 2], **kwargs)
    with pytest.raises(ValueError):
        m.sequential_scores(d, [0, 0, 1, 1, 2])
    with pytest.raises(ValueError):
        m.sequential_scores(d, [0.5, 0, 1, 1, 2, 2])


def test_library_errors_and_symbols():
    lib = _ffi.load_library()
    for sym in ("bplhip_block_loglik", "bplhip_psis_weights", "bplhip_weighted_scores"):
        assert sym in _ffi.ABI_SYMBOLS and getattr(lib, sym) is not None
    h = np.array([0, 1], dtype=np.uint16)
    blk = np.array([0, 1], dtype=np.int32)
    lw = np.full((2, 10), -np.log(10.0))
    ctx = HipContext(0)
    with pytest.raises(BplHipError) as e:
        ctx.block_loglik(h, h[::-1], h, h, blk, 2)           # no posterior
    assert e.value.code == BPLHIP_ESTATE
    with pytest.raises(BplHipError) as e:
        ctx.weighted_scores(h, h[::-1], h, h, blk, lw, 15)
    assert e.value.code == BPLHIP_ESTATE
    w = ctx.psis_weights(np.zeros((3, 10)))                  # needs no posterior
    assert (w["pareto_k"] == 0.0).all() and (w["tail_len"] == 0).all()
    np.testing.assert_allclose(w["log_weights"], -np.log(10.0), rtol=0, atol=1e-15)
    for bad in (np.full((1, 4), np.nan), np.full((1, 4), np.inf)):
        with pytest.raises(BplHipError) as e:
            ctx.psis_weights(bad)
        assert e.value.code == BPLHIP_EINVAL
    for r in (0.0, np.inf, -1.0):
        with pytest.raises(BplHipError) as e:
            ctx.psis_weights(np.zeros((1, 4)), r_eff=r)
        assert e.value.code == BPLHIP_EINVAL
    rs = np.random.RandomState(0)
    ctx.predict_set_posterior(rs.normal(0, 0.2, (10, 2)), rs.normal(0, 0.2, (10, 2)), rs.normal(0, 0.1, 10),
                              rs.uniform(-0.05, 0.05, 10))
    for bad in ([0, 2], [-1, 0]):                            # a block index out of range
        with pytest.raises(BplHipError) as e:
            ctx.block_loglik(h, h[::-1], h, h, np.array(bad, dtype=np.int32), 2)
        assert e.value.code == BPLHIP_EINVAL
        with pytest.raises(BplHipError) as e:
            ctx.weighted_scores(h, h[::-1], h, h, np.array(bad, dtype=np.int32), lw, 15)
        assert e.value.code == BPLHIP_EINVAL
    for B in (0, 4097):
        with pytest.raises(BplHipError) as e:
            ctx.block_loglik(h, h[::-1], h, h, blk, B)
        assert e.value.code == BPLHIP_EINVAL
    for G in (64, -1):
        with pytest.raises(BplHipError) as e:
            ctx.weighted_scores(h, h[::-1], h, h, blk, lw, G)
        assert e.value.code == BPLHIP_EINVAL
    with pytest.raises(BplHipError) as e:
        ctx.block_loglik(h[:0], h[:0], h[:0], h[:0], blk[:0], 2)   # no fixture
    assert e.value.code == BPLHIP_EINVAL
    with pytest.raises(BplHipError) as e:
        ctx.block_loglik(h, h[::-1], h, h, blk, 2, neutral=[0, 1])   # the other form's entry point
    assert e.value.code == BPLHIP_ESTATE
    A = ctx.block_loglik(h, h[::-1], h, h, np.array([2, 0], dtype=np.int32), 3)
    assert A.shape == (3, 10) and (A[1] == 0.0).all() and (A[[0, 2]] < 0.0).all()   # block 1 has no fixtures
    out = ctx.weighted_scores(h, h[::-1], h, h, blk, lw, 63)
    assert out["elpd"].shape == (2,) and out["proba"].shape == (2, 3)
    ctx.close()


@pytest.mark.parametrize("kind", ["basic", "dynamic"])
def test_compare_scores_takes_the_result(kind):
    m, d, block = _first_shape(kind)
    frozen, updated = m.forecast_scores(d), m.sequential_scores(d, block)
    for rule in ("rps", "brier", "log_score"):
        out = compare_scores({"frozen": frozen, "updated": updated}, rule=rule)
        assert set(out) == {"frozen", "updated"} and {v["rank"] for v in out.values()} == {0, 1}
        assert all(np.isfinite(v["score"]) and np.isfinite(v["se_diff"]) for v in out.values())
