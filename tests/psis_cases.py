"""Designed log-ratio rows for the PSIS tail (dcl::psis_tail in csrc/dc_loglik.hip.h, reached through
HipContext.psis_weights and through loglik_summary): pure numpy, seeded, no GPU.  Each case is
(name, row float64[S], r_eff) and exists for one branch of the selection, the gather, the sort, the fit or
the smoothing that continuous posteriors never reach ("The PSIS tail on designed rows").
S is 257 (M = 49 at r_eff = 1) unless the edge needs another size.

Also here, because the host and the GPU tests share them: the restatement's result per case (computed once),
a restatement with one rule altered at a time (`psis_variant`, for the mutation check), the order-preserving
key of the device (`key_of`) with a radix walk over it, and the eight-fixture model of the two-callers test."""
import functools

import numpy as np
from scipy.special import logsumexp

import loglik_ref as LR
import sequential_ref as QR
from bpl import DixonColesMatchPredictor
from bpl.elpd import LOGLIK_MAX_TAIL, tail_size

S0 = 257
M0 = tail_size(S0, 1.0)
assert M0 == 49
LOG_DBL_MIN = LR.LOG_DBL_MIN


def _rs(name):
    return np.random.RandomState(sum(ord(c) * (i + 1) for i, c in enumerate(name)) % (2 ** 31))


def _spread(rs, n, lo=-2.0):
    """n distinct values in (lo, 0], the largest exactly 0."""
    v = lo * rs.uniform(0.0, 1.0, n)
    v[np.argmax(v)] = 0.0
    assert np.unique(v).size == n and v.min() > lo
    return v


def _r_eff_for(S, M):
    """An r_eff with tail_size(S, r_eff) = M: 3 sqrt(S / r_eff) = M - 1/2."""
    r = 9.0 * S / (M - 0.5) ** 2
    assert tail_size(S, r) == M, (S, M, tail_size(S, r))
    return r


# ---- the device's key and a radix walk over it
def key_of(x):
    """The order-preserving 64-bit key of float64 x (csrc/dc_loglik.hip.h key_of); x is never -0."""
    u = np.asarray(x, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))


def radix_walk(x, M):
    """The digits the 8-bit selection of the (M+1)-th largest key needs: (digits resolved, count of the last
    digit's bucket).  It stops when the bucket holding the rank has one draw, or after the eighth digit."""
    keys = [int(k) for k in key_of(x)]
    r, prefix, digits = M + 1, 0, 0
    for shift in range(56, -1, -8):
        cand = [k for k in keys if (k >> (shift + 8)) == prefix] if shift < 56 else keys
        hist = np.bincount([(k >> shift) & 255 for k in cand], minlength=256)
        acc = 0
        for b in range(255, -1, -1):
            if acc + hist[b] >= r:
                break
            acc += hist[b]
        prefix, r, digits = (prefix << 8) | b, r - acc, digits + 1
        if hist[b] == 1 or shift == 0:
            return digits, int(hist[b])
    raise AssertionError("unreachable")


# ---- the rows
def _depth(d):
    """The top M spread over (-2, 0]; the other S - M a cluster whose top is -3 and whose other members differ
    from -3 first in byte d of the key (d = 1: in the exponent), so the cutoff -3 is alone in its bucket at
    digit d and shares it with the whole cluster before."""
    rs = _rs(f"depth{d}")
    shift = 8 * (8 - d)
    u0 = int(np.float64(-3.0).view(np.uint64))
    jmax = {1: 16, 2: 15}.get(d, 255)           # no carry into the byte above
    j = rs.randint(1, jmax + 1, S0 - M0 - 1)
    low = [int(rs.randint(0, 2 ** 31)) << 32 | int(rs.randint(0, 2 ** 31)) for _ in j]
    u = [u0 + (int(a) << shift) + (b & ((1 << shift) - 1)) for a, b in zip(j, low)]
    cluster = np.array([u0] + u, dtype=np.uint64).view(np.float64)
    assert np.isfinite(cluster).all() and cluster.max() == -3.0 and np.count_nonzero(cluster == -3.0) == 1
    row = np.concatenate([_spread(rs, M0), cluster])
    return row[rs.permutation(S0)]


def _straddle():
    rs = _rs("straddle")
    row = np.concatenate([np.full(S0 - M0 + 10, -3.0), _spread(rs, M0 - 10)])
    return row[rs.permutation(S0)]


def _all_tied_tail():
    rs = _rs("all_tied_tail")
    row = np.concatenate([np.zeros(M0), rs.uniform(-5.0, -3.0, S0 - M0)])
    return row[rs.permutation(S0)]


def _tail_ties():
    """25 values twice each on top (the lowest pair is the cutoff: 24 pairs in the tail), the two draws of a
    pair 20 or more apart."""
    rs = _rs("tail_ties")
    pairs = _spread(rs, 25)
    row = rs.uniform(-5.0, -3.0, S0)
    row[rs.permutation(100)[:25]] = pairs
    row[120 + rs.permutation(130)[:25]] = pairs
    assert np.count_nonzero(row > -2.5) == 50
    return row


def _levels(name, fractions, values):
    rs = _rs(name)
    counts = [int(round(f * S0)) for f in fractions[:-1]]
    counts.append(S0 - sum(counts))
    row = np.concatenate([np.full(c, v) for c, v in zip(counts, values)])
    return row[rs.permutation(S0)]


def _floor():
    rs = _rs("floor")
    n = 26
    row = np.concatenate([_spread(rs, n, -5.0), rs.uniform(-5.0, 0.0, S0 - n) - 800.0])
    assert row[row > -100].min() > LOG_DBL_MIN + 1.0 and row[row < -100].max() < LOG_DBL_MIN - 1.0
    return row[rs.permutation(S0)]


def _wide():
    rs = _rs("wide_1500")
    row = -1500.0 * rs.uniform(0.0, 1.0, S0)
    row[np.argmax(row)] = 0.0
    return row


def _minus_inf(name, S, fraction):
    rs = _rs(name)
    row = rs.normal(0.0, 1.0, S)
    row[rs.permutation(S)[:int(round(fraction * S))]] = -np.inf
    return row


def _pareto(k):
    """k Exponential(1): one set of exponential draws for the four cases, from a seed at which the largest two
    smoothed values of the 2.5 case exceed 0 (most seeds clamp one)."""
    return k * np.random.RandomState(35).exponential(1.0, S0)


def _bounded():
    return np.log(_rs("bounded").uniform(0.5, 1.0, S0))


def _one_spike():
    row = np.zeros(S0)
    row[131] = 50.0
    return row


def _top_tied():
    """More than M draws tie at the maximum: the cutoff is 0, nothing is above it, nothing is gathered."""
    rs = _rs("top_tied")
    row = np.concatenate([np.zeros(M0 + 11), _spread(rs, S0 - M0 - 11, -4.0) - 1.0])
    return row[rs.permutation(S0)]


def _last_draw_largest():
    rs = _rs("S65536")
    row = rs.normal(0.0, 1.0, 65536)
    row[65535] = row.max() + 0.5
    return row


PLACEMENT_S, PLACEMENT_R_EFF = 1000, 40.0      # M = 15: the 16 draws = 5 (mod 64) hold the whole tail


def _placements():
    """One spread row, its M largest moved to: the draws = 5 (mod 64); the last S mod 64 draws and the round
    of 64 before them; the draws 0..M-1."""
    S, M = PLACEMENT_S, tail_size(PLACEMENT_S, PLACEMENT_R_EFF)
    assert M == 15 and S % 64 == 40
    rs = _rs("placement")
    v = np.sort(rs.normal(0.0, 1.5, S))[::-1]                # descending: the first M are the tail
    out = []
    for name, slots in (("lane5", np.arange(5, S, 64)[:M]), ("last_rounds", S - 1 - rs.permutation(S % 64 + 64)[:M]),
                        ("first_draws", np.arange(M))):
        assert slots.size == M and np.unique(slots).size == M
        rest = np.setdiff1d(np.arange(S), slots)
        row = np.empty(S)
        row[slots[rs.permutation(M)]] = v[:M]
        row[rest[rs.permutation(S - M)]] = v[M:]
        out.append((f"placement_{name}", row, PLACEMENT_R_EFF))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, row, r_eff)]; the rows are read-only."""
    out = [(f"depth{d}", _depth(d), 1.0) for d in range(1, 9)]
    out += [("straddle", _straddle(), 1.0), ("all_tied_tail", _all_tied_tail(), 1.0), ("tail_ties", _tail_ties(), 1.0),
            ("two_levels", _levels("two_levels", (0.1, 0.9), (0.0, -1.0)), 1.0),
            ("three_levels", _levels("three_levels", (0.1, 0.3, 0.6), (0.0, -1.0, -2.0)), 1.0),
            ("floor", _floor(), 1.0), ("wide_1500", _wide(), 1.0),
            ("minus_inf_some", _minus_inf("minus_inf_some", S0, 0.3), 1.0),
            ("minus_inf_cutoff", _minus_inf("minus_inf_cutoff", 1000, 0.95), 1.0)]
    out += [(f"pareto_{k}", _pareto(k), 1.0) for k in (0.3, 0.7, 1.2, 2.5)]
    out += [("bounded", _bounded(), 1.0), ("one_spike", _one_spike(), 1.0), ("top_tied", _top_tied(), 1.0),
            ("S6", _rs("S6").normal(0.0, 1.0, 6), 1.0)]
    # 0.2 S caps M at 64 for S = 320, so M = 65 takes the next S whose cap is above it
    out += [(f"M{M}", _rs(f"M{M}").normal(0.0, 1.0, S), _r_eff_for(S, M))
            for S, M in ((320, 63), (320, 64), (330, 65), (5120, 513))]
    out += [("M1024", _rs("M1024").normal(0.0, 1.0, 5120), 0.04), ("S65536", _last_draw_largest(), 1.0)]
    out += _placements()
    for _, row, _ in out:
        row.flags.writeable = False
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    _check_design(dict((c[0], c) for c in out))
    return tuple(out)


def case(name):
    return next(c for c in cases() if c[0] == name)


def names():
    return [c[0] for c in cases()]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's (lw, k, ess, L) of a case, computed once (lw read-only)."""
    _, row, r_eff = case(name)
    lw, k, ess, L = QR.psis_row(row, r_eff)
    lw.flags.writeable = False
    return lw, k, ess, L


def _check_design(by_name):
    """What the cases claim about themselves, on the restatement."""
    def ref(name):
        _, row, r_eff = by_name[name]
        return QR.psis_row(row, r_eff)

    sizes = {"M63": 63, "M64": 64, "M65": 65, "M1024": 1024, "M513": 513, "S65536": 768, "S6": 2}
    for name, M in sizes.items():
        _, row, r_eff = by_name[name]
        assert tail_size(row.size, r_eff) == M and ref(name)[3] == M, name
    assert LOGLIK_MAX_TAIL == 1024 and int(np.argmax(by_name["S65536"][1])) == 65535
    assert ref("straddle")[3] == M0 - 10 and ref("tail_ties")[3] == 48 and ref("floor")[3] == 26
    assert ref("top_tied")[3] == 0 and ref("one_spike")[1] == np.inf and ref("one_spike")[3] == 1
    assert ref("minus_inf_cutoff")[3] == 50 and ref("minus_inf_some")[3] == M0
    k = {name: ref(name)[1] for name in by_name if name.startswith("pareto_")}
    assert all(np.isfinite(v) for v in k.values())
    assert min(k.values()) < 0.7 < max(k.values()) and min(k.values()) < 1.0 < max(k.values()), k
    assert sorted(k, key=k.get) == ["pareto_0.3", "pareto_0.7", "pareto_1.2", "pareto_2.5"], k
    lw = ref("pareto_2.5")[0]
    assert np.count_nonzero(lw == lw.max()) >= 2             # the clamp at 0 is hit by several draws
    assert ref("bounded")[1] < 0.0
    assert ref("two_levels")[3] == 26 and ref("three_levels")[3] == 26 and ref("all_tied_tail")[3] == M0


def mixed_call():
    """(names, R [B, 257]): every S = 257 case in one call, a constant row and an all -inf row among them."""
    rows = [(n, r) for n, r, e in cases() if r.size == S0 and e == 1.0]
    rows.insert(3, ("constant", np.full(S0, -3.25)))
    rows.insert(11, ("dead", np.full(S0, -np.inf)))
    return [n for n, _ in rows], np.stack([r for _, r in rows])


# ---- the restatement with one rule altered (the mutation check, and the identity with none altered)
def psis_variant(r, r_eff=1.0, floor=True, strict=True, tie_reverse=False, clamp=True, drop_inf=False, m_offset=0):
    """sequential_ref.psis_row written out once more with a switch per rule: the floor of the cutoff, the
    strict comparison at it, the order of tied tail draws, the clamp of smoothed values at 0, -inf draws taking
    part in the ranking, and M.  With every switch at its default it returns psis_row's values bit for bit."""
    r = np.asarray(r, dtype=np.float64)
    keep = r > -np.inf if drop_inf else np.ones(r.size, dtype=bool)
    full = r
    r = r[keep]
    S = r.size
    M = tail_size(S, r_eff) + m_offset
    with np.errstate(all="ignore"):
        x = (r - r.max()) + 0.0
        order = np.argsort(x, kind="stable")
        cutoff = x[order[S - M - 1]]
        if floor:
            cutoff = max(cutoff, LOG_DBL_MIN)
        tail = np.nonzero(x > cutoff if strict else x >= cutoff)[0]
        L = tail.size
        k = np.inf
        if L > 4:
            ti = tail[np.argsort(x[tail], kind="stable")]
            if tie_reverse:
                ti = tail[np.lexsort((-tail, x[tail]))]
            z = np.exp(x[ti]) - np.exp(cutoff)
            k, sigma = LR.gpdfit(z)
            if not (np.isfinite(k) and sigma > 0 and np.isfinite(sigma)):
                k = np.inf
            else:
                p = np.arange(0.5, L) / L
                q = -np.log1p(-p) if abs(k) < LR.EPS else np.expm1(-k * np.log1p(-p)) / k
                x = x.copy()
                x[ti] = np.log(q * sigma + np.exp(cutoff))
                if clamp:
                    x[x > 0] = 0
        lw = np.full(full.size, -np.inf)
        lw[keep] = x - logsumexp(x)
        return lw, float(k), float(np.exp(-logsumexp(2 * lw))), int(L)


# ---- the two-callers model: eight fixtures whose ll rows follow eight designs
TWO_CALLER_DESIGNS = ("floor", "pareto_2.5", "straddle", "pareto_0.3",
                      "depth3", "tail_ties", "bounded", "all_tied_tail")


def two_caller_model():
    """(model, data): a basic model of 8 disjoint pairs of teams, fixture i = team 2i at home to team 2i+1,
    scored 2-2 (no tau term), defence 0 and the away side's attack 0, so ll_s = 2 e_s - exp(e_s) + const with
    e_s = attack_s + home_advantage_s of the home side.  e is solved per draw so that min ll - ll, the x of
    loo's PSIS, follows design i (on the branch e <= 0; the floor design takes e down to -400).  Equal design
    values get equal e, so the ties of a design are exact ties of ll.  One pair has one e row per call, hence
    eight pairs, not one."""
    n = len(TWO_CALLER_DESIGNS)
    m = DixonColesMatchPredictor()
    names = [f"t{i:02d}" for i in range(2 * n)]
    m.teams = np.array(names)
    m._teams_dict = {t: i for i, t in enumerate(names)}
    m.attack, m.defence = np.zeros((S0, 2 * n)), np.zeros((S0, 2 * n))
    m.home_advantage = np.full(S0, 0.25)
    m.corr_coef = np.zeros(S0)
    for i, name in enumerate(TWO_CALLER_DESIGNS):
        row = case(name)[1]
        assert row.size == S0 and np.isfinite(row).all()
        t = -(row - row.max())                              # ll - min ll >= 0
        target = -1.0 - (t.max() - t)                       # f(e) = 2 e - exp(e), f(0) = -1 at the largest ll
        e = np.minimum(target / 2.0, 0.0)
        for _ in range(60):                                 # Newton on the increasing branch e < log 2
            e = e - (2.0 * e - np.exp(e) - target) / (2.0 - np.exp(e))
        assert np.abs(2.0 * e - np.exp(e) - target).max() <= 1e-12 * (1.0 + np.abs(target).max()) and e.max() <= 1e-12
        m.attack[:, 2 * i] = e - 0.25
    d = {"home_team": names[0::2], "away_team": names[1::2], "home_goals": [2] * n, "away_goals": [2] * n}
    return m, d
