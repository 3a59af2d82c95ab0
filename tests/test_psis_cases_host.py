"""The designed PSIS rows (tests/psis_cases.py) without a GPU: the conditions that make the gates of
tests/test_gpu_psis.py meaningful.

* The restatement (sequential_ref.psis_row, i.e. loglik_ref.psis) against the same algorithm in 50-digit mpmath
  on the same float64 inputs: tail_len equal, |dk| <= 1e-11 (1 + |k|).
* Conditioning: with every exp / log / log1p / expm1 result of the restatement moved one ulp up or down at
  random, tail_len does not change and k, log_weights and ess move by at most 1e-11 (1 + |value|): 1 % of the
  device gate of 1e-9, the margin being for a device libm that is not correctly rounded.
* Every edge is live: the restatement with one rule altered differs on the case built for that rule.
* The selection depth of the depth cases, by a radix walk over the device's key.
No case is exempt from the first two."""
import numpy as np
import pytest

import loglik_ref as LR
import psis_cases as PC
import sequential_ref as QR
from bpl.elpd import tail_size

REF_BOUND = 1e-11        # restatement against mpmath, and under jitter: times (1 + |value|)
GATE = 1e-9              # the device gate (DESIGN.md sections 12 and 17)
TABLE = {}               # name -> the printed figures


# ---- the same algorithm in mpmath
def _mp_psis(row, r_eff):
    """(k, L) of loglik_ref.psis with every transcendental and every sum in 50 digits.  x = r - max r is the
    float64 subtraction (one IEEE operation, the same on every machine); NaN and the "nothing smoothed" rule
    follow numpy's."""
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    mp.dps = 50
    nan, inf = mp.nan, mp.inf

    def log(v):
        if mpmath.isnan(v) or v < 0:
            return nan
        return -inf if v == 0 else mp.log(v)

    def log1p(v):
        if mpmath.isnan(v) or v < -1:
            return nan
        return -inf if v == -1 else mp.log1p(v)

    def div(a, b):
        if b == 0:
            return nan if (a == 0 or mpmath.isnan(a)) else (inf if a > 0 else -inf)
        return a / b

    S = row.size
    M = tail_size(S, r_eff)
    x = (row - row.max()) + 0.0
    cutoff = max(np.sort(x, kind="stable")[S - M - 1], LR.LOG_DBL_MIN)
    tail = np.sort(x[x > cutoff], kind="stable")
    L = tail.size
    if L <= 4:
        return np.inf, L
    ecut = mp.exp(mp.mpf(float(cutoff)))
    z = [mp.exp(mp.mpf(float(v))) - ecut for v in tail]
    n = L
    m = 30 + int(n ** 0.5)
    b = [div(1 - mp.sqrt(mp.mpf(m) / (mp.mpf(j) - mp.mpf("0.5"))), 3 * z[int(n / 4 + 0.5) - 1]) + div(mp.mpf(1), z[-1])
         for j in range(1, m + 1)]
    kj = [sum(log1p(-bj * zi) for zi in z) / n for bj in b]
    lj = [n * (log(-div(bj, k)) - k - 1) for bj, k in zip(b, kj)]
    w = [div(mp.mpf(1), sum(mp.exp(li - lo) for li in lj)) for lo in lj]
    kept = [(wj, bj) for wj, bj in zip(w, b) if wj >= 10 * LR.EPS]
    wsum = sum(wj for wj, _ in kept)
    bh = sum(bj * (wj / wsum) for wj, bj in kept) if kept else mp.mpf(0)
    kh = sum(log1p(-bh * zi) for zi in z) / n
    sigma = div(-kh, bh)
    k = (n * kh + 5) / (n + 10)
    if mpmath.isnan(k) or mpmath.isinf(k) or mpmath.isnan(sigma) or mpmath.isinf(sigma) or not sigma > 0:
        return np.inf, L
    return float(k), L


# ---- one-ulp jitter of the restatement's transcendentals
class _JitterNumpy:
    """numpy, except that every finite non-zero result of exp, log, log1p and expm1 is moved one ulp up or down
    at random.  Swapped in for loglik_ref's `np`."""

    def __init__(self, seed):
        self._rs = np.random.RandomState(seed)

    def __getattr__(self, name):
        return getattr(np, name)

    def _moved(self, v):
        v = np.asarray(v, dtype=np.float64)
        up = self._rs.randint(0, 2, v.shape).astype(bool)
        with np.errstate(all="ignore"):
            moved = np.where(up, np.nextafter(v, np.inf), np.nextafter(v, -np.inf))
        out = np.where(np.isfinite(v) & (v != 0.0), moved, v)
        return out if out.ndim else float(out)

    def exp(self, v):
        return self._moved(np.exp(v))

    def log(self, v):
        return self._moved(np.log(v))

    def log1p(self, v):
        return self._moved(np.log1p(v))

    def expm1(self, v):
        return self._moved(np.expm1(v))


def _rel(got, want):
    """max |got - want| / (1 + |want|) over the finite entries of want; the others must be equal."""
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    fin = np.isfinite(want)
    np.testing.assert_array_equal(got[~fin], want[~fin])
    assert not np.isnan(got).any()
    return float((np.abs(got[fin] - want[fin]) / (1.0 + np.abs(want[fin]))).max()) if fin.any() else 0.0


def _line(name):
    _, row, r_eff = PC.case(name)
    t = TABLE.setdefault(name, {})
    lw, k, ess, L = PC.reference(name)
    mpk = f"{t['mp']:.1e}" if "mp" in t else "-"
    jit = " ".join(f"{t[q]:.1e}" if q in t else "-" for q in ("jk", "jlw", "jess"))
    return (f"{name:22s} S={row.size:6d} M={tail_size(row.size, r_eff):5d} L={L:5d} k={k:9.4f} ess={ess:10.3f}  "
            f"mp dk {mpk}  jitter k/lw/ess {jit}")


@pytest.mark.parametrize("name", [n for n, row, _ in PC.cases() if row.size <= 1000 and np.isfinite(row).all()])
def test_restatement_against_mpmath(name):
    _, row, r_eff = PC.case(name)
    _, k, _, L = PC.reference(name)
    mk, mL = _mp_psis(row, r_eff)
    assert mL == L
    TABLE.setdefault(name, {})["mp"] = err = _rel(k, mk)
    print(_line(name))
    assert err <= REF_BOUND, (name, k, mk)


@pytest.mark.parametrize("name", PC.names())
def test_one_ulp_jitter_moves_nothing(name, monkeypatch):
    _, row, r_eff = PC.case(name)
    lw, k, ess, L = PC.reference(name)
    worst = {"jk": 0.0, "jlw": 0.0, "jess": 0.0}
    for seed in range(8):
        monkeypatch.setattr(LR, "np", _JitterNumpy(1000 + seed))
        jlw, jk, jess, jL = QR.psis_row(row, r_eff)
        monkeypatch.undo()
        assert jL == L, (name, seed)
        for key, got, want in (("jk", jk, k), ("jlw", jlw, lw), ("jess", jess, ess)):
            worst[key] = max(worst[key], _rel(got, want))
    TABLE.setdefault(name, {}).update(worst)
    print(_line(name))
    assert max(worst.values()) <= REF_BOUND, (name, worst)


def test_jitter_proxy_moves_results():
    # the proxy is in effect: a jittered run differs from the plain one in the last bits, and only there
    _, row, r_eff = PC.case("pareto_0.7")
    lw, k, _, _ = PC.reference("pareto_0.7")
    old = LR.np
    try:
        LR.np = _JitterNumpy(1)
        jlw, jk, _, _ = QR.psis_row(row, r_eff)
    finally:
        LR.np = old
    assert jk != k and (jlw != lw).any() and abs(jk - k) < 1e-12


@pytest.mark.parametrize("name", [n for n, row, _ in PC.cases() if np.max(row) > -np.inf])
def test_variant_with_no_rule_altered_is_the_restatement(name):
    _, row, r_eff = PC.case(name)
    lw, k, ess, L = PC.reference(name)
    v = PC.psis_variant(row, r_eff)
    assert v[0].tobytes() == lw.tobytes() and v[1:] == (k, ess, L)


@pytest.mark.parametrize("name,rule", [("floor", {"floor": False}), ("straddle", {"strict": False}),
                                       ("tail_ties", {"tie_reverse": True}), ("pareto_2.5", {"clamp": False}),
                                       ("minus_inf_cutoff", {"drop_inf": True}), ("M64", {"m_offset": 1}),
                                       ("M64", {"m_offset": -1})])
def test_every_edge_is_live(name, rule):
    """The restatement with one rule altered differs on the case built for it: in tail_len, or by more than 100
    device gates in k or log_weights."""
    _, row, r_eff = PC.case(name)
    lw, k, _, L = PC.reference(name)
    mlw, mk, _, mL = PC.psis_variant(row, r_eff, **rule)
    fin = np.isfinite(lw) & np.isfinite(mlw)
    dk = abs(mk - k) / (1.0 + abs(k)) if np.isfinite(k) and np.isfinite(mk) else (0.0 if mk == k else np.inf)
    dlw = float((np.abs(mlw[fin] - lw[fin]) / (1.0 + np.abs(lw[fin]))).max())
    if (np.isfinite(lw) != np.isfinite(mlw)).any():
        dlw = np.inf
    print(f"{name} with {rule}: tail_len {L} -> {mL}, k {k:.6f} -> {mk:.6f} ({dk / GATE:.2e} gates), "
          f"log_weights {dlw / GATE:.2e} gates")
    assert mL != L or dk > 100 * GATE or dlw > 100 * GATE


@pytest.mark.parametrize("d", range(1, 9))
def test_depth_cases_resolve_exactly_d_digits(d):
    _, row, r_eff = PC.case(f"depth{d}")
    x = (row - row.max()) + 0.0
    assert PC.radix_walk(x, PC.M0) == (d, 1)
    # the cutoff is the top of the cluster and the tail is far from it
    assert np.sort(x)[PC.S0 - PC.M0 - 1] == -3.0 and x[x > -3.0].min() > -2.0 and x.max() == 0.0


def test_tie_cases_end_at_the_last_digit_with_a_full_bucket():
    for name, count in (("straddle", PC.S0 - PC.M0 + 10), ("tail_ties", 2), ("one_spike", PC.S0 - 1),
                        ("minus_inf_cutoff", 950), ("top_tied", PC.M0 + 11)):
        _, row, r_eff = PC.case(name)
        assert PC.radix_walk((row - row.max()) + 0.0, tail_size(row.size, r_eff)) == (8, count), name


def test_mixed_call_and_two_caller_designs():
    names, R = PC.mixed_call()
    assert R.shape == (len(names), PC.S0) and len(names) >= 25 and {"constant", "dead"} <= set(names)
    assert not np.isnan(R).any() and not (R == np.inf).any()
    L = [QR.psis_row(r)[3] for r in R]
    assert len(set(L)) >= 6                                  # the rows of one call do not look alike
    m, d = PC.two_caller_model()
    ll = LR.ll_matrix(m, d)
    assert ll.shape == (PC.S0, len(PC.TWO_CALLER_DESIGNS)) and np.isfinite(ll).all()
    want = [PC.reference(n)[3] for n in PC.TWO_CALLER_DESIGNS]
    got = LR.summary(ll)["tail_len"].tolist()
    assert got == want                                       # the ll rows follow their designs
    assert len(set(got[:4])) > 1 and len(set(got[4:])) > 1   # unequal tails within each workgroup of four waves
    x = ll.min(axis=0) - ll
    assert x[:, 0].min() < -800.0                            # the floor design is 800 wide in ll
