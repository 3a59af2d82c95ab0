"""predict_slate on the device (csrc/dc_slate.hip.h, bpl/slate.py) against the numpy restatement
(tests/slate_ref.py: the full scoreline grid of every draw and fixture, np.bincount by leg value, np.convolve in
list order, markets_ref.summarise) for the five predictor classes, against an enumeration of all value
combinations, against what the project already computes, and on shape edges, the shared-posterior effect,
determinism and the library's own errors.

Gates.  A leg's value law is a market with 0/1 weights: each value within
tests/test_gpu_markets.py's g = 1e-12.  A draw's pmf is a product structure of N such laws whose other factors
and partial sums stay <= 1, so the legs' errors add up to N g; the convolution itself adds at most N (m_max + 1)
roundings per entry and at_least another P + 1:
    G_s = N 1e-12 + (N (m_max + 1) + P + 1) 2^-52          N, m_max the slate's; P the call's largest total
for pmf and at_least per draw; expected = sum_t t pmf[t] within P G_s.  Over the draws, as in the markets test: the
mean within the per-draw gate, sd within 10 x, a quantile within the gate plus one rounding.  (The float64
convolution in the kernel's order was checked on the CPU against long double at N = 127 with m = 1, N = 18 with
m = 7 and N = 42 with m = 3: below 0.5 % of the N (m + 1) 2^-52 term, so the reference sits far inside the gate.)"""
import numpy as np
import pytest

import loglik_ref as LR
import slate_ref as SLR
from bpl import markets as MK
from bpl import slate as SL
from bpl._ffi import BPLHIP_EINVAL, BPLHIP_ESTATE, BplHipError, HipContext

pytestmark = pytest.mark.gpu

g = 1e-12   # tests/test_gpu_markets.py, |W| <= 1
EPS = 2.0 ** -52
QS = (0.0, 0.05, 0.5, 0.95, 1.0)
EXACT = ("slates", "size", "max_total", "totals", "quantiles")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _without_goals(m, n, seed):
    d = LR.hand_data(m, n=n, seed=seed)
    for k in ("home_goals", "away_goals"):
        d.pop(k)
    return d


def _mixed_legs(n, G):
    kinds = [SL.pick("home"), MK.btts(), MK.total_over(2.5), SL.capped(MK.total_goals(), 3),
             SL.prediction_points(2, 1, exact=3, goal_difference=2, result=1), SL.pick("away"),
             SL.prediction_points(1, 1), SL.pick("draw")]
    return [kinds[i % len(kinds)] for i in range(n)]


def _gates(legs, slate, G, n):
    """G_s [J] of the call (and P)."""
    legs = [legs] * n if isinstance(legs, MK.Market) or (isinstance(legs, np.ndarray) and legs.ndim == 2) else legs
    tops = np.array([SLR.table_of(leg, G).max() for leg in legs])
    index = np.zeros(n, dtype=int) if slate is None else np.unique(np.asarray(slate), return_inverse=True)[1].reshape(n)
    J = index.max() + 1
    N = np.bincount(index, minlength=J)
    m_max = np.array([tops[index == j].max() for j in range(J)])
    P = int(np.bincount(index, weights=tops, minlength=J).max())
    return N * g + (N * (m_max + 1) + P + 1) * EPS, P


def _compare(got, ref, Gs, P, tag):
    """Every array of `got` against the restatement `ref` within the gates; prints the measured maxima over the gate."""
    assert got["kind"] == "slate" and got["n"] == ref["n"]
    for key in EXACT[:4]:
        np.testing.assert_array_equal(got[key], ref[key], err_msg=key)
    J = Gs.size
    one = EPS
    checks = {"leg_proba": g, "pmf_draws": Gs[None, :, None], "pmf": Gs[:, None], "pmf_sd": 10 * Gs[:, None],
              "pmf_quantile": (Gs + one)[:, None, None], "at_least": Gs[:, None], "at_least_sd": 10 * Gs[:, None],
              "at_least_quantile": (Gs + one)[:, None, None], "mass": Gs, "top_proba": Gs,
              "independent_pmf": Gs[:, None], "independent_at_least": Gs[:, None]}
    if P > 0:   # (P = 0: expected is an exact 0 on both sides, compared below)
        big = np.maximum(1.0, ref["expected"])
        checks.update({"expected": P * Gs, "expected_sd": 10 * P * Gs,
                       "expected_quantile": (P * Gs + one * big)[:, None]})
    else:
        for key in ("expected", "expected_sd", "expected_quantile"):
            assert (got[key] == 0.0).all(), key
    worst = {}
    for key, gate in checks.items():
        if key not in got and key == "pmf_draws":
            continue
        assert got[key].shape == ref[key].shape, (key, got[key].shape, ref[key].shape)
        assert not np.isnan(got[key]).any(), key
        worst[key] = (np.abs(got[key] - ref[key]) / gate).max()
    print(f"{tag}: error / gate " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for key, w in worst.items():
        assert w <= 1.0, (key, w)
    for j in range(J):
        top = ref["max_total"][j]
        for key in ("pmf", "pmf_sd", "at_least", "at_least_sd", "independent_pmf", "independent_at_least"):
            assert (got[key][j, top + 1:] == 0.0).all(), key   # beyond a slate's own total: an exact 0
        assert (got["pmf_quantile"][j, :, top + 1:] == 0.0).all()
        if "pmf_draws" in got:
            assert (got["pmf_draws"][:, j, top + 1:] == 0.0).all()
        assert got["top_proba"][j] == got["pmf"][j, top]


def _check(m, d, legs, slate, G, quantiles=QS, tag=""):
    got = m.predict_slate(d, legs, slate=slate, max_goals=G, quantiles=quantiles, return_draws=True)
    ref = SLR.predict_slate(m, d, legs, slate, G, quantiles)
    np.testing.assert_array_equal(got["quantiles"], np.asarray(quantiles, dtype=np.float64))
    Gs, P = _gates(legs, slate, G, ref["n"])
    _compare(got, ref, Gs, P, tag)
    return got, ref


def _interleaved(sizes, labels, seed):
    lab = np.repeat(labels, sizes)
    return lab[np.random.RandomState(seed).permutation(lab.size)]


# 1
@pytest.mark.parametrize("G", [1, 15])
@pytest.mark.parametrize("kind", LR.KINDS)
def test_all_classes_against_restatement(kind, G):
    m = LR.hand_model(kind, S=257, T=8, seed=3)
    d = _without_goals(m, 24, 4)
    slate = _interleaved([1, 2, 7, 14], [10, 3, -5, 8], 5)
    if kind == "dynamic":
        d["gameweek"] = np.where((slate == 3) | (slate == 8), 2, 0)   # the slates lie in two gameweeks
    got, _ = _check(m, d, _mixed_legs(24, G), slate, G, tag=f"{kind} G={G}")
    assert got["slates"].tolist() == [-5, 3, 8, 10] and got["size"].tolist() == [7, 2, 14, 1]


# 2
def test_against_enumeration():
    m = LR.hand_model("neutral", S=65, T=8, seed=21)
    sizes = [1, 2, 3, 4, 5, 6]
    n, G = sum(sizes), 4
    d = _without_goals(m, n, 22)
    slate = _interleaved(sizes, [0, 1, 2, 3, 4, 5], 23)
    rs = np.random.RandomState(24)
    legs = [rs.randint(0, 3, (G + 1, G + 1)) for _ in range(n)]
    for leg in legs:
        leg[0, 0], leg[G, G] = 0, 2   # every leg has the values 0..2
    got = m.predict_slate(d, legs, slate=slate, max_goals=G, return_draws=True)
    ref = SLR.predict_slate(m, d, legs, slate, G, QS)
    Gs, P = _gates(legs, slate, G, n)
    assert P == 12
    for j, N in enumerate(sizes):
        at = np.nonzero(slate == j)[0]
        want = SLR.enumerate_pmf(ref["leg_draws"][:, at], np.full(N, 2), P + 1)
        err = np.abs(got["pmf_draws"][:, j] - want).max()
        print(f"enumeration, {N} legs: error / gate {err / Gs[j]:.2e}")
        assert err <= Gs[j]
        assert np.abs(want - ref["pmf_draws"][:, j]).max() <= Gs[j]   # the two reference routes agree


# 3
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65])
def test_draw_and_slate_size_edges(S):
    m = LR.hand_model("basic", S=S, T=6, seed=S)
    sizes = [1, 63, 64, 65, 127]   # 0/1 legs: at 127 legs P + 1 = 128, the limit
    n, G = sum(sizes), 2
    d = _without_goals(m, n, 31)
    slate = _interleaved(sizes, [4, 3, 2, 1, 0], 32)
    legs = [(SL.pick("home"), SL.pick("draw"), MK.btts())[i % 3] for i in range(n)]
    got, _ = _check(m, d, legs, slate, G, tag=f"S={S}")
    assert got["max_total"].tolist() == sizes[::-1] and got["totals"].size == 128
    if S == 1:
        for name in ("pmf", "at_least", "expected"):
            assert (got[f"{name}_sd"] == 0.0).all()
            assert (got[f"{name}_quantile"] == np.expand_dims(got[name], 1)).all()   # every quantile is the single value
            assert got["pmf"].tobytes() == got["pmf_draws"][0].tobytes()


def test_eighteen_legs_worth_seven():
    m = LR.hand_model("wc", S=65, T=8, seed=41)
    d = _without_goals(m, 18, 42)
    got, _ = _check(m, d, SL.capped(MK.total_goals(), 7), None, 7, tag="18 x 7")
    assert got["max_total"].tolist() == [126] and got["pmf"][0, 126] > 0.0


@pytest.mark.parametrize("G", [0, 63])
def test_grid_depth_edges(G):
    m = LR.hand_model("extended", S=65, T=6, seed=43)
    d = _without_goals(m, 9, 44)
    legs = _mixed_legs(9, G)
    slate = [0, 1, 0, 1, 0, 1, 0, 1, 2]
    got, _ = _check(m, d, legs, slate, G, tag=f"G={G}")
    if G == 0:
        # only 0-0 is on the grid: a leg is worth 0 or, for the draw picks and prediction_points(1, 1), its value at 0-0
        assert got["max_total"].tolist() == [1, 1, 0]
        assert (got["pmf_draws"][:, 2, 0] > 0.0).all()


def test_all_zero_legs():
    m = LR.hand_model("basic", S=65, T=6, seed=45)
    d = _without_goals(m, 5, 46)
    G = 15
    zero = np.zeros((G + 1, G + 1), dtype=int)
    got, _ = _check(m, d, [zero, SL.pick("home"), zero, zero, SL.pick("home")], [0, 1, 0, 0, 1], G, tag="zeros")
    assert got["max_total"].tolist() == [0, 2]
    assert got["pmf"][0, 0].tobytes() == got["mass"][0].tobytes() and (got["pmf"][0, 1:] == 0.0).all()
    assert (got["pmf_draws"][:, 0, 1:] == 0.0).all() and (got["expected"][0] == 0.0)


# 4
@pytest.mark.parametrize("kind", ["basic", "dynamic"])
def test_ties_to_predict_markets(kind):
    m = LR.hand_model(kind, S=130, T=8, seed=51)
    n, G = 10, 15
    d = _without_goals(m, n, 52)
    got = m.predict_slate(d, SL.pick("home"), slate=np.arange(n)[::-1], max_goals=G, return_draws=True)
    mk = m.predict_markets(d, {"home_win": MK.home_win()}, max_goals=G, return_draws=True)
    err = np.abs(got["pmf_draws"][:, ::-1, 1] - mk["draws"][:, 0, :]).max()   # slate n - 1 - i is fixture i
    print(f"{kind}: pmf[1] of one-leg slates against predict_markets' home_win draws, error / g {err / g:.2e}")
    assert err <= g
    assert got["at_least"][:, 0].tobytes() == got["mass"].tobytes()
    assert got["pmf"].shape == (n, 2) and got["max_total"].tolist() == [1] * n
    np.testing.assert_array_equal(got["top_proba"], got["pmf"][np.arange(n), got["max_total"]])
    err = np.abs(got["leg_proba"][:, 1] - mk["mean"][0]).max()
    assert err <= g and (got["leg_proba"][:, 2:] == 0.0).all()


# 5
def test_shared_posterior_lifts_the_accumulator():
    S = 64
    m = LR.hand_model("basic", S=S, T=4, seed=61)
    m.attack[:, 0] = np.where(np.arange(S) < S // 2, 0.8, -0.8)   # team 0 strong in one half of the draws, weak in the other
    d = {"home_team": ["t00", "t00"], "away_team": ["t01", "t02"]}
    legs = SL.pick("home")
    got, ref = _check(m, d, legs, None, 15, tag="two halves")
    Gs, _ = _gates(legs, None, 15, 2)
    margin = ref["pmf"][0, 2] - ref["independent_pmf"][0, 2]   # Cov_draw(p_1, p_2), about Var_draw(p)
    p = ref["leg_draws"][:, :, 1]
    assert margin > 0.01 and abs(margin - np.cov(p[:, 0], p[:, 1], ddof=0)[0, 1]) < 1e-12
    print(f"accumulator {got['pmf'][0, 2]:.6f}, from posterior means {got['independent_pmf'][0, 2]:.6f}, margin {margin:.6f}")
    assert got["pmf"][0, 2] - got["independent_pmf"][0, 2] >= margin - 2 * Gs[0]   # fails if anything averages first
    # one draw: nothing is shared, the two agree
    one = LR.hand_model("basic", S=1, T=4, seed=62)
    r = one.predict_slate(d, legs, max_goals=15)
    assert np.abs(r["pmf"] - r["independent_pmf"]).max() <= Gs[0]
    assert np.abs(r["at_least"] - r["independent_at_least"]).max() <= Gs[0]


# 6
ARRAYS = ("pmf", "pmf_sd", "pmf_quantile", "at_least", "at_least_sd", "at_least_quantile", "expected", "expected_sd",
          "expected_quantile", "mass", "top_proba", "pmf_draws")


def _direct(m, d, legs, slate, G):
    """(context, keyword arguments) of the one HipContext.slate_summary call predict_slate makes."""
    (_, device, kw), = m._fixture_groups(d, with_goals=False)[0]
    n = len(d["home_team"])
    tables, leg_table = SL.leg_tables(legs, n, G)
    _, index = SL.slate_index(slate, n)
    order = np.argsort(index, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(index))]).astype(np.int32)
    return device(), dict(SL._rows(kw, order), max_goals=G, tables=tables, leg_table=leg_table[order], start=start)


@pytest.mark.parametrize("kind", ["extended", "wc"])
def test_runs_chunks_and_reorderings_are_bit_identical(kind):
    S = 257
    m = LR.hand_model(kind, S=S, T=8, seed=71)
    sizes = [3, 9, 1, 6, 5]
    n, G = sum(sizes), 15
    d = _without_goals(m, n, 72)
    slate = _interleaved(sizes, [0, 1, 2, 3, 4], 73)
    legs = _mixed_legs(n, G)
    a = m.predict_slate(d, legs, slate=slate, max_goals=G, quantiles=QS, return_draws=True)
    b = m.predict_slate(d, legs, slate=slate, max_goals=G, quantiles=QS, return_draws=True)
    for key in ARRAYS + ("leg_proba", "independent_pmf", "independent_at_least"):
        assert a[key].tobytes() == b[key].tobytes(), key
    # any chunking of the slates
    ctx, kw = _direct(m, d, legs, slate, G)
    whole = ctx.slate_summary(**kw, quantiles=QS, return_draws=True)
    K = whole["mean"].shape[0]
    largest = (K + 8 * max(sizes)) * S * 8
    for ws in (largest, largest + 8 * S * 8, 2 * largest + 5, 3 * largest):   # 5 chunks (one slate each) down to 2
        part = ctx.slate_summary(**kw, quantiles=QS, return_draws=True, workspace_bytes=ws)
        for key in ("mean", "sd", "quantile", "leg_proba", "draws"):
            assert whole[key].tobytes() == part[key].tobytes(), (key, ws)
    # any reordering that keeps each slate's own order: the slates one after the other, and reversed blocks
    for perm in (np.argsort(slate, kind="stable"), np.argsort(-slate, kind="stable")):
        p = m.predict_slate({k: [v[i] for i in perm] for k, v in d.items()}, [legs[i] for i in perm], slate=slate[perm],
                            max_goals=G, quantiles=QS, return_draws=True)
        for key in ARRAYS:
            assert a[key].tobytes() == p[key].tobytes(), key
        assert a["leg_proba"][perm].tobytes() == p["leg_proba"].tobytes()
    # a slate's own order reversed: another summation order, within the gate
    rev = np.arange(n)[::-1]
    r = m.predict_slate({k: [v[i] for i in rev] for k, v in d.items()}, [legs[i] for i in rev], slate=slate[rev],
                        max_goals=G, quantiles=QS, return_draws=True)
    Gs, _ = _gates(legs, slate, G, n)
    err = np.abs(r["pmf_draws"] - a["pmf_draws"]).max(axis=(0, 2))
    print(f"{kind}: reversed slates, error / gate {(err / Gs).max():.2e}")
    assert (err <= Gs).all()


# 7
def test_library_errors():
    h = np.array([0, 1, 0], dtype=np.uint16)
    a = np.array([1, 0, 1], dtype=np.uint16)
    ones = np.ones((1, 16, 16), dtype=np.uint8)
    ctx = HipContext(0)

    def fails(code, *args, **kwargs):
        with pytest.raises(BplHipError) as e:
            ctx.slate_summary(*args, **kwargs)
        assert e.value.code == code, (e.value.code, kwargs)

    ok = dict(tables=ones, leg_table=[0, 0, 0], start=[0, 2, 3])
    fails(BPLHIP_ESTATE, h, a, 15, **ok)                                       # no posterior
    rs = np.random.RandomState(0)
    S = 10
    ctx.predict_set_posterior(rs.normal(0, 0.2, (S, 2)), rs.normal(0, 0.2, (S, 2)), rs.normal(0, 0.1, S),
                              rs.uniform(-0.05, 0.05, S))
    fails(BPLHIP_ESTATE, h, a, 15, neutral=[0, 1, 0], **ok)                    # the other form's entry point
    fails(BPLHIP_EINVAL, h, a, 64, tables=np.ones((1, 65, 65), dtype=np.uint8), leg_table=[0, 0, 0], start=[0, 3])
    bad = ones.copy()
    bad[0, 3, 4] = 8
    fails(BPLHIP_EINVAL, h, a, 15, **dict(ok, tables=bad))                     # a leg value of 8
    fails(BPLHIP_EINVAL, h, a, 15, **dict(ok, leg_table=[0, 1, 0]))            # no such table
    fails(BPLHIP_EINVAL, h, a, 15, **dict(ok, start=[0, 2]))                   # start does not cover the fixtures
    fails(BPLHIP_EINVAL, h, a, 15, **dict(ok, start=[1, 2, 3]))
    fails(BPLHIP_EINVAL, h, a, 15, **dict(ok, start=[0, 4]))
    fails(BPLHIP_EINVAL, h, a, 15, **dict(ok, start=[0, 2, 2, 3]))             # an empty slate
    fails(BPLHIP_EINVAL, h, a, 15, quantiles=[0.5, 1.5], **ok)
    fails(BPLHIP_EINVAL, h, a, 15, quantiles=np.linspace(0, 1, 17), **ok)
    many = np.arange(128) % 2
    seven = np.full((1, 16, 16), 7, dtype=np.uint8)
    fails(BPLHIP_EINVAL, many.astype(np.uint16), (1 - many).astype(np.uint16), 15, tables=ones,
          leg_table=np.zeros(128, dtype=np.int32), start=[0, 128])             # sum m_i = 128
    fails(BPLHIP_EINVAL, many[:19].astype(np.uint16), (1 - many[:19]).astype(np.uint16), 15, tables=seven,
          leg_table=np.zeros(19, dtype=np.int32), start=[0, 19])               # 19 x 7 = 133
    K = 2 * (2 + 1) + 2
    largest = (K + 8 * 2) * S * 8
    fails(BPLHIP_EINVAL, h, a, 15, workspace_bytes=-1, **ok)
    fails(BPLHIP_EINVAL, h, a, 15, workspace_bytes=largest - 1, **ok)          # holds no slate
    out = ctx.slate_summary(h, a, 15, workspace_bytes=largest, quantiles=[0.1, 0.9], return_draws=True, **ok)
    assert out["mean"].shape == (K, 2) and out["sd"].shape == (K, 2) and out["quantile"].shape == (K, 2, 2)
    assert out["leg_proba"].shape == (3, 8) and out["draws"].shape == (S, 2, 3) and np.isfinite(out["draws"]).all()
    full = ctx.slate_summary(many[:127].astype(np.uint16), (1 - many[:127]).astype(np.uint16), 63,
                             tables=np.ones((1, 64, 64), dtype=np.uint8), leg_table=np.zeros(127, dtype=np.int32),
                             start=[0, 127])                                   # the limits themselves
    assert full["mean"].shape == (258, 1) and full["quantile"].shape == (258, 0, 1) and "draws" not in full
    assert (full["mean"][:127, 0] == 0.0).all() and full["mean"][127, 0] > 0.0   # every leg scores 1: the total is 127
    ctx.close()
