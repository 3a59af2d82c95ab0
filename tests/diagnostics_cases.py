"""Designed series for the MCMC diagnostics kernels (diag_rank and diag_ess in csrc/dc_diagnostics.hip.h, reached
through HipContext.mcmc_diagnostics): pure numpy, seeded, no GPU.  Each case is (name, group, C, N, values[C N],
quantiles, claims) and exists for one branch of the sort, the tie search, the quantile read-off, the R-hat or
Geyer's walk that continuous Student-t draws never reach.  `claims` are the reach facts
of the case: (text, predicate of `facts(name)`) pairs computed from the values on the host, so that a test can
assert that the case enters its branch.

Also here, because the host and the GPU tests share them: the facts themselves (`skipped_passes`, `tie_runs`,
`walk_facts`, `quantile_facts`), the restatement's result per case (computed once), and the restatement with one
rule altered at a time (`diagnose_variant`, for the mutation check)."""
import functools
import math
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

import diagnostics_ref as R
from psis_cases import key_of

Case = namedtuple("Case", "name group C N values quantiles claims")
MARGIN = 1e-6                 # the least decision margin of the restatement (tests/test_gpu_diagnostics.py)
DEFAULT_Q = (0.05, 0.95)
LDS_DRAWS = 12288             # csrc/dc_diagnostics.hip.h DIAG_LDS_DRAWS
WAVES = 4                     # DIAG_WAVES: each wave sorts ceil(S / 4) entries


# ---- the facts
def split_keys(values, C):
    """(keys of the split x, keys of |x - median|), each uint64 [S], as diag_rank builds them."""
    s = R.split_chains(values, C).ravel() + 0.0
    return key_of(s), key_of(np.abs(s - np.median(s)) + 0.0)


def _skipped(keys):
    return frozenset(b for b in range(8) if np.unique((keys >> np.uint64(8 * b)) & np.uint64(255)).size == 1)


def skipped_passes(values, C):
    """The byte positions (0 = the least significant, the first pass) at which every key has the same digit, so
    that radix_sort skips the pass: (for x, for |x - median|)."""
    kx, kf = split_keys(values, C)
    return _skipped(kx), _skipped(kf)


def _runs(keys):
    s = np.sort(keys)
    edges = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1], [True]]))
    return [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]


def tie_runs(values, C, fold=False):
    """The runs of equal values in the sorted split draws (of |x - median| with fold) as (first, past)."""
    return _runs(split_keys(values, C)[1 if fold else 0])


def walk_facts(m):
    """What Geyer's walk does on the M x n matrix m: diagnostics_ref.ess_of's `facts`, plus "ess" and "margin"."""
    f = {}
    ess, margin = R.ess_of(np.asarray(m, dtype=np.float64), facts=f)
    f.update(ess=ess, margin=margin)
    return f


def quantile_facts(values, C, q):
    """numpy's "linear" read-off as diag_rank does it: the virtual index h = S q + (1 - q) - 1 in float64, lo = its
    floor, g = h - lo, a and b the order statistics lo and lo + 1 of the split draws, and the value."""
    s = np.sort(R.split_chains(values, C).ravel() + 0.0)
    S = s.size
    q = float(q)
    h = (S * q + (1.0 + q * -1.0)) - 1.0
    lo = min(max(int(math.floor(h)), 0), S - 1)
    g = max(h - math.floor(h), 0.0)
    a, b = float(s[lo]), float(s[min(lo + 1, S - 1)])
    return dict(q=q, h=h, lo=lo, g=g, a=a, b=b, value=float(np.quantile(s, q)))


def series_of(values, C, quantiles):
    """{"bulk": z, "mean": split x, "tail0", "tail1", ...: the indicators}, the matrices diag_ess walks."""
    s = R.split_chains(values, C)
    out = {"bulk": R.z_scale(s), "mean": s}
    for i, q in enumerate(quantiles):
        out[f"tail{i}"] = (s <= np.quantile(s, q)).astype(np.float64)
    return out


# ---- the restatement with one rule altered (the mutation check, and the identity with none altered)
def _ess_variant(m, monotone=True, floor=True, stop=3):
    """diagnostics_ref.ess_of once more, with a switch for the monotone step, for tau's floor and for the walk's
    bound t < n - stop."""
    M, n = m.shape
    S = M * n
    d = m - m.mean(axis=1, keepdims=True)
    acov = lambda t: float(np.mean(np.sum(d[:, :n - t] * d[:, t:], axis=1) / n))
    mean_var = acov(0) * n / (n - 1.0)
    var_plus = mean_var * (n - 1.0) / n
    if M > 1:
        var_plus += float(np.var(m.mean(axis=1), ddof=1))
    if var_plus == 0.0:
        return math.nan
    rho = np.zeros(n + 3)
    rho_of = lambda t: 1.0 - (mean_var - acov(t)) / var_plus
    even, odd = 1.0, rho_of(1)
    rho[0], rho[1] = even, odd
    t = 1
    while t < n - stop:
        if not even + odd > 0.0:
            break
        even, odd = rho_of(t + 1), rho_of(t + 2)
        if even + odd >= 0.0:
            rho[t + 1], rho[t + 2] = even, odd
        t += 2
    max_t = t - 2
    if even > 0.0:
        rho[max_t + 1] = even
    t = 1
    while monotone and t <= max_t - 2:
        if rho[t + 1] + rho[t + 2] > rho[t - 1] + rho[t]:
            rho[t + 1] = (rho[t - 1] + rho[t]) / 2.0
            rho[t + 2] = rho[t + 1]
        t += 2
    tau = -1.0 + 2.0 * float(np.sum(rho[:max_t + 1])) + rho[max_t + 1]
    return S / (max(tau, 1.0 / math.log10(S)) if floor else tau)


def _first_ranks(v):
    """1-based ranks; tied values all take the first rank of their run."""
    v = np.asarray(v, dtype=np.float64).ravel() + 0.0
    return np.searchsorted(np.sort(v), v, side="left") + 1.0


def diagnose_variant(x, num_chains, quantiles=DEFAULT_Q, rank="average", tail_strict=False, monotone=True, floor=True,
                     stop=3, fold="median", method="linear", keep_middle=False):
    """diagnostics_ref.diagnose_one written out once more with a switch per rule: the rank of a tie run (its
    average or its first), `<` for `<=` in the tail indicator, the monotone step, tau's floor, the walk's bound,
    the centre of the fold (median or mean), numpy's quantile method, and a split whose second half starts at
    draw n (keeping the middle draw of an odd N and dropping the last).  With every switch at its default it
    returns diagnose_one's statistics bit for bit."""
    x = np.asarray(x, dtype=np.float64).ravel()
    out = {nm: math.nan for nm in R.STATS}
    with np.errstate(all="ignore"):
        out["mean"] = float(np.mean(x))
        out["sd"] = float(np.std(x, ddof=1))
    if not np.all(np.isfinite(x)):
        return out
    s = R.split_chains(x, num_chains)
    if keep_middle:
        c = x.reshape(num_chains, -1)
        n = c.shape[1] // 2
        s = np.stack([c[:, :n], c[:, n:2 * n]], axis=1).reshape(2 * num_chains, n)
    if s.min() == s.max():
        return out
    ranks = R.average_ranks if rank == "average" else _first_ranks
    z_of = lambda m: np.array([R._INV((ri - 0.375) / (m.size + 0.25)) for ri in ranks(m)]).reshape(m.shape)
    ess = lambda m: _ess_variant(m, monotone, floor, stop)
    zb = z_of(s)
    zf = z_of(np.abs(s - (np.median(s) if fold == "median" else np.mean(s))))
    out["rhat"] = float(np.maximum(R.rhat_of(zb), R.rhat_of(zf)))
    out["ess_bulk"], out["ess_mean"] = ess(zb), ess(s)
    tails = []
    for q in quantiles:
        qv = np.quantile(s, q, method=method)
        tails.append(ess((s < qv if tail_strict else s <= qv).astype(np.float64)))
    out["ess_tail"] = float(np.min(tails)) if tails else math.nan
    with np.errstate(invalid="ignore"):   # (without the floor tau, and so the ess, can be negative)
        out["mcse_mean"] = float(out["sd"] / np.sqrt(out["ess_mean"]))
    return out


# ---- the generators
def _rs(name, seed=0):
    return np.random.RandomState((sum(ord(c) * (i + 1) for i, c in enumerate(name)) + 7919 * seed) % (2 ** 31))


def continuous(rs, C, N):
    """[C, N] chains of different location and scale with a heavy tail: no ties (tests/test_gpu_diagnostics.py)."""
    return rs.standard_t(5, size=(C, N)) * rs.uniform(0.5, 2.0, (C, 1)) + rs.normal(0, 0.3, (C, 1))


def ar1(rs, C, N, phi):
    return R.ar1(rs, C, N, phi)[:, 0].reshape(C, N)


def _one_byte():
    """1 + j 2^-12: the 512 keys differ in byte 5 only (bits 40..47 hold j), every other pass is skipped."""
    rs = _rs("one_byte")
    j = np.concatenate([rs.permutation(256), rs.permutation(256)])
    return 1.0 + j * 2.0 ** -12


def _one_byte_low():
    """1 + j 2^-52: the keys differ in the least significant byte only.  The spread is 255 ulps of the values, so
    the moments (sd, ess_mean, mcse_mean) are decided by how the mean happens to round: only the rank statistics
    of this case are compared."""
    rs = _rs("one_byte")
    j = np.concatenate([rs.permutation(256), rs.permutation(256)])
    return 1.0 + j * 2.0 ** -52


def _exponent_only(positive):
    """2 x 64 signed powers of two, 64 of each sign, every magnitude 2^e with e in -60..60 and 2^-60 present with
    both signs as the two middle order statistics, so the median is exactly 0 and |x - median| is a power of two."""
    rs = _rs("exponent_only", 3)
    e_neg = np.concatenate([[-60], rs.randint(-59, 61, 63)])
    e_pos = np.concatenate([[-60], rs.randint(-59, 61, 63)])
    v = np.concatenate([-(2.0 ** e_neg), 2.0 ** e_pos])[rs.permutation(128)]
    return np.abs(v) if positive else v


def _small_ints():
    return _rs("small_ints", 1).poisson(3.0, size=(4, 128)).astype(np.float64)


def _wide_range():
    """2 x 65: signed magnitudes 10^u, u uniform in (-140, 140), with three subnormals, +0 and -0 among them and
    1e140 as the middle draw of chain 0, which the split drops."""
    rs = _rs("wide_range", 0)
    v = rs.choice([-1.0, 1.0], size=(2, 65)) * 10.0 ** rs.uniform(-140.0, 140.0, (2, 65))
    v[0, 5], v[1, 40], v[1, 60] = 4.9e-324, -3.0e-310, 1.1e-315
    v[0, 50], v[1, 3] = 0.0, -0.0
    v[0, 32] = 1e140
    return v


def _two_valued(name, C, N, p, seed=0):
    return (_rs(name, seed).uniform(size=(C, N)) < p).astype(np.float64)


def _all_but_one(larger):
    v = np.full((1, 64), 2.5)
    v[0, 41] = 4.0 if larger else 1.0
    return v


def _run_at_both_ends():
    """3 x 129: 38 of the 384 split draws tied at the minimum, 15 at the maximum (3.9 %: below the 5 % at which the
    0.95 indicator would be constant); the middle draws, which the split drops, hold the maximum too."""
    rs = _rs("run_at_both_ends", 0)
    v = continuous(rs, 3, 129)
    lo, hi = math.floor(v.min()) - 1.0, math.ceil(v.max()) + 1.0
    keep = np.flatnonzero((np.arange(3 * 129) % 129) != 64)
    slots = keep[rs.permutation(keep.size)]
    v = v.reshape(-1)
    v[slots[:38]] = lo
    v[slots[38:53]] = hi
    v[64::129] = hi
    return v.reshape(3, 129)


def _max_tie_tail_nan():
    """2 x 128: 31 of the 256 draws (12 %) tied at the maximum: the 0.95 quantile is the maximum and its indicator
    is all ones."""
    rs = _rs("max_tie_tail_nan", 0)
    v = continuous(rs, 2, 128).reshape(-1)
    v[rs.permutation(256)[:31]] = math.ceil(v.max()) + 1.0
    return v.reshape(2, 128)


def _symmetric_fold():
    """2 x 64 around the median 0.75: 57 pairs 0.75 +- a_j, two more magnitudes twice each on the upper side (so
    that the mean is not the median) and ten draws equal to the median; a_j = k / 32, the small k in chain 0 and the
    large in chain 1, so that the folded R-hat is the larger one.  Every |x - median| is exact and occurs at least
    twice."""
    rs = _rs("symmetric_fold", 0)
    k = rs.permutation(np.arange(1, 60))
    small, large = np.sort(k)[:29], np.sort(k)[29:]
    c0 = np.concatenate([0.75 + small / 32.0, 0.75 - small / 32.0, np.full(6, 0.75)])                       # 64
    c1 = np.concatenate([0.75 + large[:28] / 32.0, 0.75 - large[:28] / 32.0,
                         np.repeat(0.75 + large[28:] / 32.0, 2), np.full(4, 0.75)])                          # 64
    assert c0.size == 64 and c1.size == 64 and large[28:].size == 2
    return np.stack([c0[rs.permutation(64)], c1[rs.permutation(64)]])


def _chains_constant():
    """Split chain m holds the integer m (4 chains of 16: chain c is eight draws of 2 c, then eight of 2 c + 1).
    W = 0, so rhat is NaN; the chains differ, so var_plus > 0 and every ess is finite.  Every autocorrelation is
    exactly 1, so the monotone comparisons are between equal numbers and the restatement's margin is exactly 0.
    The case is admitted all the same because every quantity compared is exact in float64 on both sides: the
    values are small integers (and, rank-normalised, one z per chain, summed eight at a time, which only doubles
    it), so the chain means are exact, every deviation is exactly 0, every autocovariance is 0, var_plus is the
    variance of the chain means alone and rho = 1 - 0 / var_plus = 1 whatever var_plus rounds to; tau is a sum of
    ones."""
    return np.repeat(np.arange(8.0), 8).reshape(4, 16)


def _c256(shift):
    rs = _rs("c256", 0)
    v = continuous(rs, 256, 8)
    if shift:
        v[100] += 3.0 * v.std()
    return v


NQ16_K0 = (13, 64, 100)       # q = k / 127 whose virtual index comes out as the integer k in float64


def nq16_quantiles():
    near = lambda lo, g: (lo + g) / 127.0
    q = [k / 127.0 for k in NQ16_K0]
    q += [near(20, 0.5 - 5e-4), near(20, 0.5 + 5e-4), near(90, 0.5 - 5e-4), near(90, 0.5 + 5e-4), near(50, 0.5)]
    q += [near(30, 1e-3), near(70, 0.999)]
    q += [0.004, 0.996, 1e-9, 1.0 - 1e-9, 0.05, 0.95]
    assert len(q) == 16
    return tuple(q)


NQ16_ADJACENT = (20, 90, 50, 70)   # order statistics lo, lo + 1 one ulp apart: a lerp with g >= 1/2 rounds to the upper


def _nq(name, seed=0, adjacent=()):
    rs = _rs(name, seed)
    v = continuous(rs, 2, 64).reshape(-1)
    order = np.argsort(v)
    for lo in adjacent:
        v[order[lo + 1]] = np.nextafter(v[order[lo]], np.inf)
    assert (np.argsort(v) == order).all() and np.unique(v).size == v.size
    return v.reshape(2, 64)


def _edge(C, N):
    """Student-t draws, the chains alike (so that every walk ends inside the first block of lags)."""
    return _rs("store_edge", 0).standard_t(5, size=(C, N))


# seeds searched on the CPU (how: DESIGN.md section 20a): the walk cases need a stop lag, a
# stop reason or a number of monotone replacements, and every case needs a margin of at least 1e-6
WALK = {"antithetic": (-0.9, 3), "stop_at_63": (0.95, 30), "stop_at_65": (0.95, 0), "monotone": (0.8, 4),
        "never_truncates@128": (0.999, 3), "never_truncates@130": (0.999, 1), "never_truncates@132": (0.999, 0),
        "never_truncates@134": (0.999, 0), "never_truncates@136": (0.999, 0)}


def _walk(name, C, N):
    phi, seed = WALK[name]
    return ar1(_rs(name, seed), C, N, phi)


# ---- the claims (predicates of facts(name))
def _long_runs(F, fold=False):
    return [b - a for a, b in (F.runs_fold if fold else F.runs_x) if b - a > F.per]


def _nan_is(*names):
    return (f"NaN exactly in {sorted(names)}", lambda F: F.nan == frozenset(names))


_FINITE = _nan_is()
_LOW6 = frozenset(range(6))


def _build():
    out = []

    def add(name, group, v, quantiles=DEFAULT_Q, claims=()):
        v = np.ascontiguousarray(v, dtype=np.float64)
        C, N = v.shape
        out.append(Case(name, group, C, N, v.reshape(-1), tuple(quantiles), tuple(claims)))

    # -- sort
    add("one_byte", "sort", _one_byte().reshape(1, 512), claims=[
        ("seven of the eight passes are skipped for x, all but byte 5", lambda F: F.skipped_x == frozenset(range(8)) - {5}),
        ("every value occurs twice", lambda F: len(F.runs_x) == 256 and all(b - a == 2 for a, b in F.runs_x)), _FINITE])
    add("one_byte_low", "sort", _one_byte_low().reshape(1, 512), claims=[
        ("seven of the eight passes are skipped for x, all but byte 0", lambda F: F.skipped_x == frozenset(range(1, 8))),
        ("every value occurs twice", lambda F: len(F.runs_x) == 256 and all(b - a == 2 for a, b in F.runs_x))])
    add("exponent_only", "sort", _exponent_only(False).reshape(2, 64), claims=[
        ("both signs, 64 each", lambda F: np.count_nonzero(F.split < 0) == 64 and np.count_nonzero(F.split > 0) == 64),
        ("the median is exactly 0", lambda F: F.median == 0.0),
        ("x: the low six bytes take the two digits 0x00 and 0xff, one per sign; no pass is skipped",
         lambda F: F.skipped_x == frozenset() and all(F.digits_x[b] == 2 for b in range(6))),
        ("|x - median|: the low six bytes are skipped", lambda F: F.skipped_fold == _LOW6), _FINITE])
    add("exponent_only_pos", "sort", _exponent_only(True).reshape(2, 64), claims=[
        ("x: the low six bytes are skipped, the two exponent bytes are not", lambda F: F.skipped_x == _LOW6), _FINITE])
    add("small_ints", "sort", _small_ints(), np.linspace(0.05, 0.95, 5), claims=[
        ("the low six bytes are skipped for x and for the fold",
         lambda F: F.skipped_x >= _LOW6 and F.skipped_fold >= _LOW6),
        ("at most 16 distinct values: runs of 20 and more", lambda F: len(F.runs_x) <= 16 and max(b - a for a, b in F.runs_x) >= 100),
        ("every quantile lies inside a tie run", lambda F: all(t["a"] == t["b"] for t in F.quant)),
        ("no quantile is the maximum", lambda F: all(t["value"] < F.split.max() for t in F.quant)), _FINITE])
    add("wide_range", "sort", _wide_range(), claims=[
        ("N is odd and the dropped middle draw is the largest", lambda F: F.N % 2 == 1 and F.values.max() > F.split.max()),
        ("no pass is skipped", lambda F: F.skipped_x == frozenset() and F.skipped_fold == frozenset()),
        ("both signs, subnormals, +0 and -0",
         lambda F: (F.split < 0).any() and (F.split > 0).any()
         and np.count_nonzero((F.split != 0) & (np.abs(F.split) < 2.3e-308)) == 3
         and sorted(np.signbit(F.raw_split[F.raw_split == 0]).tolist()) == [False, True]),
        ("magnitudes from below 1e-130 to above 1e130, squares finite",
         lambda F: np.abs(F.split[F.split != 0]).min() < 1e-300 and np.abs(F.split).max() > 1e130
         and np.isfinite(np.sum(F.values ** 2))), _FINITE])
    # -- ties
    add("two_valued", "ties", _two_valued("two_valued", 2, 256, 0.3), (0.05, 0.5, 0.95), claims=[
        ("two runs, each longer than a quarter of S", lambda F: len(F.runs_x) == 2 and len(_long_runs(F)) == 2),
        ("every quantile lies inside a run", lambda F: [t["a"] == t["b"] for t in F.quant] == [True] * 3),
        ("the 0.95 quantile is the maximum, so its indicator is constant and ess_tail is NaN",
         lambda F: F.quant[2]["value"] == 1.0 and F.walk["tail2"]["stop_reason"] == "constant"),
        _nan_is("ess_tail")])
    add("two_valued_low", "ties", _two_valued("two_valued", 2, 256, 0.3), (0.05, 0.5), claims=[
        ("two runs, each longer than a quarter of S", lambda F: len(F.runs_x) == 2 and len(_long_runs(F)) == 2),
        ("both quantiles lie inside the run of zeros", lambda F: all(t["a"] == t["b"] == 0.0 for t in F.quant)), _FINITE])
    for larger in (True, False):
        add("all_but_one_" + ("larger" if larger else "smaller"), "ties", _all_but_one(larger), claims=[
            ("one run of 63 and one single value",
             lambda F, larger=larger: F.runs_x == ([(0, 63), (63, 64)] if larger else [(0, 1), (1, 64)])),
            ("the fold has 63 zeros", lambda F: F.runs_fold == [(0, 63), (63, 64)]),
            _FINITE if larger else _nan_is("ess_tail")])
    add("run_at_both_ends", "ties", _run_at_both_ends(), claims=[
        ("a run of 38 from sorted index 0 and a run of 15 up to S - 1",
         lambda F: F.runs_x[0] == (0, 38) and F.runs_x[-1] == (F.S - 15, F.S)),
        ("the run at the maximum is below 5 % of S and the 0.95 quantile is below the maximum",
         lambda F: 15 < 0.05 * F.S and F.quant[1]["b"] < F.split.max()),
        ("the 0.05 quantile lies inside the run at the minimum", lambda F: F.quant[0]["a"] == F.quant[0]["b"] == F.split.min()),
        _FINITE])
    add("max_tie_tail_nan", "ties", _max_tie_tail_nan(), claims=[
        ("31 of 256 tied at the maximum", lambda F: F.runs_x[-1] == (225, 256)),
        ("the 0.95 indicator is constant, the 0.05 one is not",
         lambda F: F.walk["tail1"]["stop_reason"] == "constant" and F.walk["tail0"]["stop_reason"] != "constant"),
        _nan_is("ess_tail")])
    add("symmetric_fold", "ties", _symmetric_fold(), claims=[
        ("every folded value occurs at least twice", lambda F: min(b - a for a, b in F.runs_fold) >= 2),
        ("ten folded zeros from sorted index 0", lambda F: F.runs_fold[0] == (0, 10) and F.median == 0.75),
        ("the mean is not the median", lambda F: abs(F.split.mean() - F.median) > 1e-3),
        ("the folded R-hat is the one reported", lambda F: F.ref["rhat"] == F.ref["rhat_folded"] > F.ref["rhat_bulk"]),
        _FINITE])
    add("two_valued_workspace", "ties", _two_valued("two_valued_workspace", 64, 1000, 0.5), (0.05, 0.45), claims=[
        ("S = 64000 is sorted in the workspace", lambda F: F.S == 64000 > LDS_DRAWS),
        ("two runs of about 32000", lambda F: len(F.runs_x) == 2 and min(b - a for a, b in F.runs_x) > 31000),
        ("every walk stops inside the first block of lags", lambda F: all(w["stop_lag"] < 63 for w in F.walk.values())),
        _FINITE])
    # -- rhat
    add("chains_constant", "rhat", _chains_constant(), (0.05, 0.8), claims=[
        ("split chain m is the integer m", lambda F: (R.split_chains(F.values, 4) == np.arange(8.0)[:, None]).all()),
        ("every autocorrelation the walks compute is exactly 1.0",
         lambda F: all(w["rho"] and all(r == 1.0 for r in w["rho"]) for w in F.walk.values())),
        ("the margin is exactly 0", lambda F: F.ref["margin"] == 0.0),
        _nan_is("rhat")])
    add("c256", "rhat", _c256(False), claims=[("M = 512, n = 4: the walk never starts",
                                                lambda F: F.M == 512 and F.walk["mean"]["stop_lag"] == 1), _FINITE])
    add("c256_shift", "rhat", _c256(True), claims=[("one chain moved: rhat above 1.01 and above c256's",
                                                    lambda F: F.ref["rhat"] > 1.01 and F.ref["rhat"] > facts("c256").ref["rhat"]),
                                                   _FINITE])
    # -- walk
    add("antithetic", "walk", _walk("antithetic", 4, 200), (0.4, 0.6), claims=[
        ("every series walks at least one pair and takes the floor",
         lambda F: all(w["floor"] and w["stop_lag"] >= 3 for w in F.walk.values())),
        ("every ess is S log10 S", lambda F: all(F.ref[k] == F.S * math.log10(F.S) for k in ("ess_bulk", "ess_mean", "ess_tail"))),
        _FINITE])
    for lag in (63, 65):
        add(f"stop_at_{lag}", "walk", _walk(f"stop_at_{lag}", 2, 600), claims=[
            (f"the mean series stops at lag {lag} by a non-positive pair",
             lambda F, lag=lag: F.walk["mean"]["stop_lag"] == lag and F.walk["mean"]["stop_reason"] == "pair"), _FINITE])
    for N in (128, 130, 132, 134, 136):
        n = N // 2
        stop = n - 3 if (n - 3) % 2 else n - 2
        add(f"never_truncates@{N}", "walk", _walk(f"never_truncates@{N}", 1, N), claims=[
            (f"the mean and bulk series end by t < n - 3 at lag {stop}",
             lambda F, stop=stop: all(F.walk[k]["stop_reason"] == "bound" and F.walk[k]["stop_lag"] == stop
                                      for k in ("mean", "bulk"))), _FINITE])
    add("monotone", "walk", _walk("monotone", 2, 400), claims=[
        ("the mean series makes at least 3 monotone replacements, the bulk series at least 1",
         lambda F: F.walk["mean"]["replacements"] >= 3 and F.walk["bulk"]["replacements"] >= 1), _FINITE])
    # -- quantiles
    add("nq0", "quant", _nq("nq"), (), claims=[_nan_is("ess_tail")])
    add("nq1", "quant", _nq("nq"), (0.3,), claims=[_FINITE])
    add("nq16", "quant", _nq("nq", adjacent=NQ16_ADJACENT), nq16_quantiles(), claims=[
        ("three virtual indices are integers: g == 0", lambda F: [F.quant[i]["g"] for i in range(3)] == [0.0] * 3
         and [F.quant[i]["lo"] for i in range(3)] == list(NQ16_K0)),
        ("g within 1e-3 below and above 1/2, twice each",
         lambda F: all(0.499 < F.quant[i]["g"] < 0.5 for i in (3, 5)) and all(0.5 < F.quant[i]["g"] < 0.501 for i in (4, 6))),
        ("g near 0 and near 1", lambda F: 0 < F.quant[8]["g"] < 2e-3 and 0.998 < F.quant[9]["g"] < 1
         and 0 < F.quant[12]["g"] < 1e-6 and F.quant[12]["lo"] == 0 and F.quant[13]["g"] > 1 - 1e-6 and F.quant[13]["lo"] == 126),
        ("where g > 1/2 meets order statistics one ulp apart the quantile is the upper one",
         lambda F: all(F.quant[i]["b"] == np.nextafter(F.quant[i]["a"], np.inf) and F.quant[i]["value"] == F.quant[i]["b"]
                       for i in (4, 6, 9))),
        ("one g is exactly 1/2, between order statistics one ulp apart",
         lambda F: F.quant[7]["g"] == 0.5 and F.quant[7]["b"] == np.nextafter(F.quant[7]["a"], np.inf)),
        ("where g < 1/2 meets them it is the lower one",
         lambda F: all(F.quant[i]["b"] == np.nextafter(F.quant[i]["a"], np.inf) and F.quant[i]["value"] == F.quant[i]["a"]
                       for i in (3, 5))),
        _FINITE])
    # -- storage
    add("lds_edge", "store", _edge(3, 4096), claims=[("S = 12288, the last size sorted in LDS", lambda F: F.S == LDS_DRAWS), _FINITE])
    add("ws_edge", "store", _edge(1, 12290), claims=[("S = 12290, the first even size sorted in the workspace",
                                                      lambda F: F.S == LDS_DRAWS + 2), _FINITE])
    for c in out:
        c.values.setflags(write=False)
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


RANK_ONLY = ("one_byte_low",)   # compared in rhat, ess_bulk and ess_tail only (see _one_byte_low)
MARGIN_EXEMPT = ("chains_constant",)


@functools.lru_cache(maxsize=None)
def cases():
    return _build()


def case(name):
    return next(c for c in cases() if c.name == name)


def names():
    return [c.name for c in cases()]


@functools.lru_cache(maxsize=None)
def reference(name):
    """diagnostics_ref.diagnose_one of a case, computed once."""
    c = case(name)
    return R.diagnose_one(c.values, c.C, c.quantiles)


@functools.lru_cache(maxsize=None)
def facts(name):
    """Everything the claims of a case are predicates of."""
    c = case(name)
    raw = R.split_chains(c.values, c.C)
    s = raw.ravel() + 0.0
    kx, kf = split_keys(c.values, c.C)
    n = c.N // 2
    F = SimpleNamespace(name=name, C=c.C, N=c.N, n=n, M=2 * c.C, S=2 * c.C * n, values=c.values, split=s,
                        raw_split=raw.ravel(), median=float(np.median(s)))
    F.per = -(-F.S // WAVES)
    F.skipped_x, F.skipped_fold = _skipped(kx), _skipped(kf)
    F.digits_x = [int(np.unique((kx >> np.uint64(8 * b)) & np.uint64(255)).size) for b in range(8)]
    F.runs_x, F.runs_fold = _runs(kx), _runs(kf)
    F.quant = [quantile_facts(c.values, c.C, q) for q in c.quantiles]
    F.ref = reference(name)
    F.nan = frozenset(nm for nm in R.STATS if math.isnan(F.ref[nm]))
    F.walk = {k: walk_facts(m) for k, m in series_of(c.values, c.C, c.quantiles).items()}
    return F


def stacks():
    """The cases of equal (C, N, quantiles), two or more: {(C, N, quantiles): [names]}."""
    groups = {}
    for c in cases():
        groups.setdefault((c.C, c.N, c.quantiles), []).append(c.name)
    return {k: v for k, v in groups.items() if len(v) > 1}
