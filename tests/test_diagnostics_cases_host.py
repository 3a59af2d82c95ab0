"""The designed diagnostics series (tests/diagnostics_cases.py) without a GPU: the conditions that make the gates of
tests/test_gpu_diagnostics_cases.py meaningful.

* Reach: every case asserts the facts it claims (skipped sort passes, tie runs against a wave's quarter of the
  array, where and why the walk stopped, monotone replacements, tau's floor, the NaN pattern, each quantile's
  fraction g and its two order statistics), and its decision margin.
* The restatement (diagnostics_ref.diagnose_one) against the same algorithm in 50-digit mpmath on the same float64
  inputs: ranks exact, Phi^-1 from mpmath's inverse error function, every sum and the walk in mp.mpf.
* Every rule is live: the restatement with one rule altered moves a statistic of the case built for that rule by
  more than 1e-6 (1 + |value|), or changes its NaN pattern."""
import functools
import math

import numpy as np
import pytest

import diagnostics_cases as DC
import diagnostics_ref as R

REF_BOUND = 1e-11        # restatement against mpmath: times (1 + |value|)
LIVE = 1e-6              # a rule altered must move a statistic by more than this, times (1 + |value|)
MP_MAX_S = 4096
# one_byte_low: 1 + j 2^-52 has a spread of 255 ulps, so float64 moments of it depend on how the mean rounds; the
# measured errors of its sd, ess_mean and mcse_mean are in DESIGN.md section 20a and only its rank statistics
# are held to the bound (here and on the device)
RANK_STATS = ("rhat", "ess_bulk", "ess_tail")


# ---- reach
CLAIMS = [(c.name, i) for c in DC.cases() for i in range(len(c.claims))]


@pytest.mark.parametrize("name, i", CLAIMS, ids=[f"{n}-{i}" for n, i in CLAIMS])
def test_every_case_reaches_what_it_claims(name, i):
    text, holds = DC.case(name).claims[i]
    assert holds(DC.facts(name)), (name, text)


@pytest.mark.parametrize("name", DC.names())
def test_margins(name):
    m = DC.reference(name)["margin"]
    if name in DC.MARGIN_EXEMPT:
        assert m == 0.0      # by design: see the case's docstring (exact arithmetic on both sides)
    else:
        assert m >= DC.MARGIN, (name, m)


def test_the_helpers_on_hand_made_values():
    v = np.array([1.0, 1.0, 2.0, 2.0, 2.0, 3.0, 1.0, 5.0])
    assert DC.tie_runs(v, 1) == [(0, 3), (3, 6), (6, 7), (7, 8)]
    sx, sf = DC.skipped_passes(v, 1)
    assert sx == frozenset(range(6)) and sf == frozenset(range(6))    # small integers: six zero mantissa bytes
    assert DC.skipped_passes(np.array([1.0, 1.0 + 2.0 ** -52] * 4), 1)[0] == frozenset(range(1, 8))
    f = DC.walk_facts(R.split_chains(R.ar1(np.random.RandomState(5), 2, 100, 0.7)[:, 0], 2))
    assert f["stop_reason"] == "pair" and 3 <= f["stop_lag"] < 47 and not f["floor"] and len(f["rho"]) == f["stop_lag"] + 1
    f = DC.walk_facts(np.random.RandomState(1).normal(size=(2, 4)))
    assert f["stop_reason"] == "bound" and f["stop_lag"] == 1 and f["floor"] and f["replacements"] == 0
    t = DC.quantile_facts(np.arange(8.0), 1, 0.5)
    assert (t["lo"], t["g"], t["a"], t["b"], t["value"]) == (3, 0.5, 3.0, 4.0, 3.5)


def test_the_branches_the_issue_lists_each_have_a_case():
    F = {n: DC.facts(n) for n in DC.names()}
    per = lambda f: f.per
    # a run spanning a wave's quarter; one from index 0; one up to S - 1; all but one; one in the workspace
    assert any(b - a > per(f) for f in F.values() for a, b in f.runs_x)
    assert any(f.runs_x[0][1] > 1 for f in F.values()) and any(f.runs_x[-1][1] - f.runs_x[-1][0] > 1 for f in F.values())
    assert any(max(b - a for a, b in f.runs_x) == f.S - 1 for f in F.values())
    assert any(f.S > DC.LDS_DRAWS and len(f.runs_x) == 2 for f in F.values())
    # stop lags 61, 63 and 65 by the bound and 63, 65 by a pair; the floor after a walk; three replacements
    stops = {(w["stop_lag"], w["stop_reason"]) for f in F.values() for w in f.walk.values()}
    assert {(61, "bound"), (63, "bound"), (65, "bound"), (63, "pair"), (65, "pair")} <= stops
    assert any(w["floor"] and w["stop_lag"] >= 3 for f in F.values() for w in f.walk.values())
    assert any(w["replacements"] >= 3 for w in F["monotone"].walk.values())
    # NQ of 0, 1, 2, 3, 5 and 16; S on both sides of the storage switch
    assert {len(DC.case(n).quantiles) for n in F} >= {0, 1, 2, 3, 5, 16}
    assert {DC.LDS_DRAWS, DC.LDS_DRAWS + 2} <= {f.S for f in F.values()}
    assert max(f.M for f in F.values()) == 512


# ---- the same algorithm in mpmath
@functools.lru_cache(maxsize=None)
def _mp_inv_phi(r2, S):
    """Phi^-1((r - 3/8) / (S + 1/4)) for the rank r = r2 / 2."""
    import mpmath
    mp = mpmath.mp
    p = (mp.mpf(r2) / 2 - mp.mpf(3) / 8) / (mp.mpf(S) + mp.mpf(1) / 4)
    return mp.sqrt(2) * mp.erfinv(2 * p - 1)


def _mp_diagnose(x, C, quantiles):
    """diagnose_one with every sum, Phi^-1 and the walk in 50 digits.  What is float64 by definition stays so: the
    fold |x - median| and the quantile values (single IEEE operations the device repeats), hence the indicators."""
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    mp.dps = 50
    f = mp.mpf
    x = np.asarray(x, dtype=np.float64).ravel()
    out = {}
    X = [f(float(v)) for v in x]
    mean = sum(X) / len(X)
    out["mean"] = mean
    out["sd"] = mp.sqrt(sum((v - mean) ** 2 for v in X) / (len(X) - 1))
    s = R.split_chains(x, C)
    M, n = s.shape
    S = M * n

    def z_of(m):
        v = m.ravel() + 0.0
        srt = np.sort(v)
        r2 = np.searchsorted(srt, v, side="left") + np.searchsorted(srt, v, side="right") + 1   # twice the average rank
        return [[_mp_inv_phi(int(r2[c * n + i]), S) for i in range(n)] for c in range(M)]

    def moments(m):
        mu = [sum(row) / n for row in m]
        var = [sum((v - a) ** 2 for v in row) / (n - 1) for row, a in zip(m, mu)]
        gm = sum(mu) / M
        between = sum((a - gm) ** 2 for a in mu) / (M - 1)
        return mu, var, between

    def rhat(m):
        mu, var, between = moments(m)
        W = sum(var) / M
        return mp.nan if W == 0 else mp.sqrt((f(n - 1) / n * W + between) / W)

    def ess(m):
        mu, var, between = moments(m)
        d = [[v - a for v in row] for row, a in zip(m, mu)]
        acov = lambda t: sum(sum(row[i] * row[i + t] for i in range(n - t)) / n for row in d) / M
        mean_var = acov(0) * n / (n - 1)
        var_plus = mean_var * (n - 1) / n + between
        if var_plus == 0:
            return mp.nan
        rho = [f(0)] * (n + 2)
        rho_of = lambda t: 1 - (mean_var - acov(t)) / var_plus
        even, odd = f(1), rho_of(1)
        rho[0], rho[1] = even, odd
        t = 1
        while t < n - 3:
            if not even + odd > 0:
                break
            even, odd = rho_of(t + 1), rho_of(t + 2)
            if even + odd >= 0:
                rho[t + 1], rho[t + 2] = even, odd
            t += 2
        max_t = t - 2
        if even > 0:
            rho[max_t + 1] = even
        t = 1
        while t <= max_t - 2:
            if rho[t + 1] + rho[t + 2] > rho[t - 1] + rho[t]:
                rho[t + 1] = (rho[t - 1] + rho[t]) / 2
                rho[t + 2] = rho[t + 1]
            t += 2
        tau = -1 + 2 * sum(rho[:max_t + 1]) + rho[max_t + 1]
        floor = 1 / mp.log10(S)
        return S / max(tau, floor)

    as_mp = lambda m: [[f(float(v)) for v in row] for row in m]
    zb, zf = z_of(s), z_of(np.abs(s - np.median(s)))
    rb, rf = rhat(zb), rhat(zf)
    out["rhat"] = mp.nan if (mpmath.isnan(rb) or mpmath.isnan(rf)) else max(rb, rf)
    out["ess_bulk"], out["ess_mean"] = ess(zb), ess(as_mp(s))
    tails = [ess(as_mp((s <= np.quantile(s, q)).astype(np.float64))) for q in quantiles]
    out["ess_tail"] = mp.nan if (not tails or any(mpmath.isnan(t) for t in tails)) else min(tails)
    out["mcse_mean"] = out["sd"] / mp.sqrt(out["ess_mean"])
    return {k: float(v) for k, v in out.items()}


MP_BOUNDS = {}           # name -> a bound other than REF_BOUND, from the case's own conditioning (none needed)


@pytest.mark.parametrize("name", [c.name for c in DC.cases() if 2 * c.C * (c.N // 2) <= MP_MAX_S])
def test_restatement_against_mpmath(name):
    c = DC.case(name)
    ref = DC.reference(name)
    want = _mp_diagnose(c.values, c.C, c.quantiles)
    worst = {}
    for nm in R.STATS:
        assert math.isnan(ref[nm]) == math.isnan(want[nm]), (name, nm)
        worst[nm] = 0.0 if math.isnan(want[nm]) else abs(ref[nm] - want[nm]) / (1.0 + abs(want[nm]))
    print(f"{name:22s} restatement against mpmath, error / (1 + |value|): "
          + " ".join(f"{nm} {e:.1e}" for nm, e in worst.items()))
    bound = MP_BOUNDS.get(name, REF_BOUND)
    for nm in (RANK_STATS if name in DC.RANK_ONLY else R.STATS):
        assert worst[nm] <= bound, (name, nm, worst[nm])
    if name in DC.RANK_ONLY:     # the exemption is needed: a moment of the case is beyond the bound in float64
        assert max(worst[nm] for nm in R.STATS if nm not in RANK_STATS) > 1e3 * REF_BOUND


# ---- the restatement with one rule altered
@pytest.mark.parametrize("name", DC.names())
def test_variant_with_no_rule_altered_is_the_restatement(name):
    c = DC.case(name)
    ref, v = DC.reference(name), DC.diagnose_variant(c.values, c.C, c.quantiles)
    assert np.array([v[nm] for nm in R.STATS]).tobytes() == np.array([ref[nm] for nm in R.STATS]).tobytes()


RULES = [("small_ints", {"rank": "first"}), ("two_valued_low", {"tail_strict": True}), ("run_at_both_ends", {"tail_strict": True}),
         ("monotone", {"monotone": False}), ("antithetic", {"floor": False}), ("never_truncates@128", {"stop": 2}),
         ("never_truncates@132", {"stop": 2}), ("never_truncates@136", {"stop": 2}), ("symmetric_fold", {"fold": "mean"}),
         ("wide_range", {"keep_middle": True})]


@pytest.mark.parametrize("name, rule", RULES, ids=[f"{n}-{next(iter(r))}" for n, r in RULES])
def test_each_rule_matters_on_its_case(name, rule):
    c = DC.case(name)
    ref, v = DC.reference(name), DC.diagnose_variant(c.values, c.C, c.quantiles, **rule)
    moved = {}
    for nm in R.STATS:
        if math.isnan(ref[nm]) != math.isnan(v[nm]):
            moved[nm] = math.inf
        elif not math.isnan(ref[nm]):
            moved[nm] = abs(v[nm] - ref[nm]) / (1.0 + abs(ref[nm]))
    print(f"{name} with {rule}: " + " ".join(f"{nm} {e:.1e}" for nm, e in moved.items() if e > 0))
    assert max(moved.values()) > LIVE, (name, rule, moved)


def test_two_valued_cannot_show_the_tail_comparison():
    """With 0.95 among the quantiles of 0/1 draws that are 30 % ones, that quantile is 1, the maximum: `<=` makes its
    indicator constant, `<` makes the indicators of 0.05 and 0.5 (both 0, the minimum) constant, and ess_tail is NaN
    either way.  `two_valued_low` (the same draws without the 0.95 quantile) and `run_at_both_ends` carry the rule."""
    c = DC.case("two_valued")
    assert math.isnan(DC.reference("two_valued")["ess_tail"])
    assert math.isnan(DC.diagnose_variant(c.values, c.C, c.quantiles, tail_strict=True)["ess_tail"])


def test_lower_for_linear_matters_on_the_quantiles_of_nq16_built_for_it():
    """ess_tail is a minimum over the quantiles, so the rule is shown one quantile at a time (the GPU test runs them
    one at a time too): where g > 1/2 meets order statistics one ulp apart, "linear" rounds to the upper one and
    "lower" leaves out its draw; everywhere else the two indicators are the same."""
    c = DC.case("nq16")
    moved = []
    for q in c.quantiles:
        a = DC.diagnose_variant(c.values, c.C, (q,))["ess_tail"]
        b = DC.diagnose_variant(c.values, c.C, (q,), method="lower")["ess_tail"]
        moved.append(abs(a - b) / (1.0 + abs(a)))
    print("nq16, lower for linear, per quantile: " + " ".join(f"{m:.1e}" for m in moved))
    assert all(moved[i] > LIVE for i in (4, 6, 9)) and all(m == 0.0 for i, m in enumerate(moved) if i not in (4, 6, 9))
