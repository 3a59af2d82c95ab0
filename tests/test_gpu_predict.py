"""The predict kernels (csrc/dc_predict.hip.h) against the float64 restatement (tests/fake_ctx.py:
FakePredictCtx) on hand-built posteriors (tests/loglik_ref.py:hand_model, nothing is fitted): the shape edges
of `predict_score_grid` -- draws around the blocks of 64 and the float64 fold at 256, depths around the 16 x 16
tiles, fixture counts around the 4 waves of a workgroup, team indices up to T - 1 and T > 256 --, all five
rate forms, clipped tau terms, a context whose posterior is replaced, and the pointwise kernel.

Gates.  A grid cell: err <= 3e-6 * want + 1e-12, the gate of tests/test_gpu_fit.py; the float32 method by itself
stays under half of it on these inputs (tests/test_predict_emu_host.py).  Where every draw's tau is clipped the
restatement's cell is an exact 0 and so is the kernel's (the tau cells are sums of terms >= 0), and no cell is
negative.  The pointwise kernel is float64 throughout: 1e-12 absolute, the project's figure, and 1e-12
relative where want >= 1e-280: the exponent's argument stays below 745 in magnitude, its rounding gives at
most ~2e-13, exp and lgamma add a few ulp, the mean over draws nothing of that order.
Every test prints its largest err / bound."""
import numpy as np
import pytest

import predict_emu as PE
from bpl._ffi import BPLHIP_EINVAL, BplHipError, HipContext
from fake_ctx import FakePredictCtx
from loglik_ref import KINDS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def ctx():
    c = HipContext(0)
    yield c
    c.close()


def _both(ctx, venue, args):
    """The posterior on the device context and on a fresh float64 restatement."""
    ref = FakePredictCtx()
    PE.set_posterior(ctx, venue, args)
    PE.set_posterior(ref, venue, args)
    return ref


def _check_grid(ctx, ref, h, a, G, kw, label, gate=True):
    """Every cell of the float64 grids against the restatement, the shape, the float32 output; returns (got, want)."""
    got = ctx.predict_score_grid(h, a, G, **kw)
    want = ref.predict_score_grid(h, a, G, kw.get("neutral"), kw.get("conf"))
    assert got.shape == want.shape == (len(h), G + 1, G + 1) and got.dtype == np.float64
    assert not np.isnan(got).any()
    assert (got >= 0.0).all(), got.min()
    g32 = ctx.predict_score_grid(h, a, G, dtype=np.float32, **kw)
    assert g32.dtype == np.float32 and g32.shape == got.shape
    np.testing.assert_array_equal(g32, got.astype(np.float32))   # the float64 cells rounded once
    if gate:
        ratio = np.abs(got - want) / PE.grid_bound(want)
        print(f"{label}: largest err / bound {ratio.max():.3f}")
        assert (ratio <= 1.0).all(), (label, ratio.max(), np.unravel_index(ratio.argmax(), ratio.shape))
    return got, want


# ---- the grid: shapes
@pytest.mark.parametrize("G", [0, 15, 16, 63])
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 127, 128, 255, 256, 257, 320, 321])
def test_grid_draw_counts_and_depths(ctx, S, G):
    venue, args, h, a, kw = PE.case("basic", S, 6, 5)
    ref = _both(ctx, venue, args)
    _check_grid(ctx, ref, h, a, G, kw, f"S={S} max_goals={G}")


@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 7, 9])
def test_grid_fixture_counts(ctx, M):
    venue, args, h, a, kw = PE.case("basic", 65, 6, M)
    ref = _both(ctx, venue, args)
    _check_grid(ctx, ref, h, a, 17, kw, f"M={M}")


@pytest.mark.parametrize("G", [1, 17, 31, 32, 47, 48])
def test_grid_tile_edges(ctx, G):
    venue, args, h, a, kw = PE.case("basic", 130, 6, 3)
    ref = _both(ctx, venue, args)
    _check_grid(ctx, ref, h, a, G, kw, f"max_goals={G}")


# ---- the grid: the five rate forms
@pytest.mark.parametrize("kind", KINDS)
def test_grid_all_kinds(ctx, kind):
    T = 8
    venue, args, h, a, kw = PE.case(kind, 257, T, 7)
    ref = _both(ctx, venue, args)
    assert h[-1] == T - 1
    if venue:
        assert set(kw["neutral"]) == {0, 1}
    if kind == "wc":
        assert kw["conf"][0][0] == kw["conf"][1][0] and kw["conf"][0][1] != kw["conf"][1][1]
    _check_grid(ctx, ref, h, a, 31, kw, kind)


@pytest.mark.parametrize("kind", ["extended", "wc"])
def test_grid_three_hundred_teams(ctx, kind):
    T = 300
    venue, args, h, a, kw = PE.case(kind, 65, T, 7)
    ref = _both(ctx, venue, args)
    assert h[-1] == T - 1 and a[0] == T - 1 and max(h.max(), a.max()) > 256
    _check_grid(ctx, ref, h, a, 17, kw, f"{kind} T={T}")


# ---- the grid: clipped tau
@pytest.mark.parametrize("G", [0, 1, 15])
@pytest.mark.parametrize("S", [64, 257])
@pytest.mark.parametrize("pattern", PE.CLIP_PATTERNS)
def test_grid_clipped_tau(ctx, pattern, S, G):
    """corr_coef = 5.0: 1 - rho < 0 and 1 - rho lh la < 0 (rates about 1), -5.0: 1 + rho lh < 0 and 1 + rho la < 0."""
    venue, args, h, a, kw = PE.case("basic", S, 6, 5, pattern=pattern)
    ref = _both(ctx, venue, args)
    got, want = _check_grid(ctx, ref, h, a, G, kw, f"{pattern} S={S} max_goals={G}")   # no NaN, >= 0, the gate
    zero = want == 0.0
    print(f"{pattern} S={S} max_goals={G}: {int(zero.sum())} cells are exactly 0 in the restatement; "
          f"least cell {got.min():.3e}")
    if pattern == "all" and G >= 1:
        assert zero[:, 1, 1].all()   # 1 - rho < 0 on every draw
    assert (got[zero] == 0.0).all(), np.abs(got[zero]).max()
    g32 = ctx.predict_score_grid(h, a, G, dtype=np.float32, **kw)
    assert (g32[zero] == 0.0).all() and (g32 >= 0.0).all()


@pytest.mark.parametrize("S", [64, 257])
def test_grid_tau_on_the_clip_boundary(ctx, S):
    """Draws with tau exactly at the clip: rho = 1 (1 - rho = 0), rho = -1 / lh, rho = -1 / la and rho = 1 / (lh la) of
    the first fixture.  The float32 and the float64 route may land on different sides of the clip, so only: no
    NaN, no negative cell (and the float32 output is the float64 one rounded once)."""
    venue, args, h, a, kw = PE.case("basic", S, 6, 5)
    att, dfn, ha, cc = (np.array(v) for v in args)
    lh = np.exp(att[:, h[0]] - dfn[:, a[0]] + ha)
    la = np.exp(att[:, a[0]] - dfn[:, h[0]])
    cc[3], cc[4], cc[5], cc[6] = 1.0, -1.0 / lh[4], -1.0 / la[5], 1.0 / (lh[6] * la[6])
    cc[S - 1] = 1.0
    ref = _both(ctx, venue, [att, dfn, ha, cc])
    for G in (0, 1, 15):
        got, _ = _check_grid(ctx, ref, h, a, G, kw, "boundary", gate=False)
        print(f"clip boundary S={S} max_goals={G}: least cell {got.min():.3e}")


# ---- a context whose posterior is replaced
def test_posterior_replaced_on_a_live_context():
    """Smaller, other-form and again plain posteriors on one context: the device buffers only grow, so a stale
    float32 copy or a stale shape would show in the grid (float32 team-major copies) or the pointwise query
    (float64 tables)."""
    c = HipContext(0)
    steps = [("basic", 257, 8), ("basic", 5, 3), ("wc", 65, 6), ("extended", 64, 5)]
    worst = 0.0
    for n, (kind, S, T) in enumerate(steps):
        venue, args, h, a, kw = PE.case(kind, S, T, 5)
        ref = _both(c, venue, args)
        _check_grid(c, ref, h, a, 17, kw, f"step {n + 1} ({kind} S={S} T={T})")
        x, y = np.array([0, 1, 1, 3, 20]), np.array([0, 0, 1, 2, 1])
        got = c.predict_score_proba(h, a, x, y, **kw)
        want = ref.predict_score_proba(h, a, x, y, kw.get("neutral"), kw.get("conf"))
        worst = max(worst, np.abs(got - want).max())
        assert np.abs(got - want).max() <= 1e-12
    print(f"pointwise after each replacement: largest error {worst:.3e} (gate 1e-12)")
    c.close()


# ---- the pointwise kernel
GOALS = np.array([0, 1, 64, 70, 170, 255, 2, 3, 5, 16])


@pytest.mark.parametrize("S", [1, 65])
@pytest.mark.parametrize("M", [1, 255, 256, 257])
@pytest.mark.parametrize("kind", KINDS)
def test_pointwise(ctx, kind, M, S):
    T = 8
    venue, args = PE.posterior(kind, S, T, seed=71)
    ref = _both(ctx, venue, args)
    h, a, kw = PE.fixtures(kind, M, T, seed=M)
    # every pair of the goal counts comes up within 100 queries; the first four queries are the tau scorelines
    q = np.arange(M)
    x, y = GOALS[q % 10], GOALS[(q // 10) % 10]
    x[:4], y[:4] = np.array([0, 0, 1, 1])[:M], np.array([0, 1, 0, 1])[:M]
    got = ctx.predict_score_proba(h, a, x, y, **kw)
    want = ref.predict_score_proba(h, a, x, y, kw.get("neutral"), kw.get("conf"))
    assert got.shape == (M,) and not np.isnan(got).any() and (got >= 0.0).all()
    err = np.abs(got - want)
    big = want >= 1e-280
    rel = (err[big] / want[big]).max()
    print(f"{kind} M={M} S={S}: largest absolute error {err.max():.3e}, largest relative error {rel:.3e} "
          f"over {int(big.sum())} queries (gates 1e-12)")
    assert err.max() <= 1e-12, err.max()
    assert rel <= 1e-12, (rel, x[big][(err[big] / want[big]).argmax()], y[big][(err[big] / want[big]).argmax()])


# ---- cross-checks
@pytest.mark.parametrize("kind", ["basic", "wc"])
def test_grid_cells_are_the_pointwise_results(ctx, kind):
    T, G = 8, 17
    venue, args = PE.posterior(kind, 130, T, seed=81)
    PE.set_posterior(ctx, venue, args)
    h, a, kw = PE.fixtures(kind, 5, T, seed=82)
    grid = ctx.predict_score_grid(h, a, G, **kw)
    xs, ys = np.meshgrid(np.arange(G + 1), np.arange(G + 1), indexing="ij")
    n = xs.size
    rep = {k: (np.repeat(v[0], n), np.repeat(v[1], n)) if k == "conf" else np.repeat(v, n) for k, v in kw.items()}
    point = ctx.predict_score_proba(np.repeat(h, n), np.repeat(a, n), np.tile(xs.ravel(), 5), np.tile(ys.ravel(), 5),
                                    **rep).reshape(grid.shape)
    ratio = np.abs(grid - point) / PE.grid_bound(point)
    print(f"{kind}: grid against pointwise, largest err / bound {ratio.max():.3f}")
    assert (ratio <= 1.0).all(), ratio.max()


def test_two_grid_calls_are_byte_identical(ctx):
    venue, args = PE.posterior("neutral", 321, 8, seed=91)
    PE.set_posterior(ctx, venue, args)
    h, a, kw = PE.fixtures("neutral", 9, 8, seed=92)
    for dtype in (np.float64, np.float32):
        one, two = (ctx.predict_score_grid(h, a, 20, dtype=dtype, **kw) for _ in range(2))
        assert one.tobytes() == two.tobytes()


def test_depth_out_of_range_is_an_error(ctx):
    venue, args = PE.posterior("basic", 10, 4, seed=93)
    PE.set_posterior(ctx, venue, args)
    for G in (-1, 64):
        for dtype in (np.float64, np.float32):
            with pytest.raises(BplHipError) as e:
                ctx.predict_score_grid([0, 1], [1, 2], G, dtype=dtype)
            assert e.value.code == BPLHIP_EINVAL
    assert ctx.predict_score_grid([0, 1], [1, 2], 63).shape == (2, 64, 64)
