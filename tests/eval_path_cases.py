"""Deterministic inputs that pin each form of the neutral-venue and dynamic evaluation kernels
(tests/test_gpu_eval_paths.py runs them, tests/test_eval_path_cases_host.py checks on the CPU that every
case still sits on the edge it was built for).

The host picks the form from the data (bpl-next_amd/csrc/bplhip.hip, launch_eval_neutral /
launch_eval_dynamic).  This module restates those rules in numpy -- the sort, the slice arithmetic, the
run count per wave, the incidence lists -- with every constant read out of the headers, and each builder
returns a Case: the fixtures, the options, the form it was built for and the facts that put it there.

Assumed: 256 CUs (the option dyn_big_wgs = 0 means one workgroup per CU); every case that sets dyn_big_wgs
asks for at most 7 workgroups and does not depend on the CU count while that many are resident at once.
"""
import os
import re
from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np

import dc_dynamic_oracle as DO
import dc_neutral_oracle as NO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bpl-next_amd", "csrc")
N_CU = 256


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(text, name):
    """`NAME = <integer expression>` of a constexpr / enum declaration."""
    m = re.search(r"\b%s\s*=\s*([^,;}]+?)\s*[,;}]" % name, text)
    assert m, name
    expr = m.group(1)
    assert re.fullmatch(r"[\d\s<*+()-]+", expr), (name, expr)
    return int(eval(expr))  # pylint: disable=eval-used  (digits, shifts, products only: checked above)


_NEU, _DYN, _HOST = _read("dc_neutral.hip.h"), _read("dc_dynamic.hip.h"), _read("bplhip.hip")
NEU_RUNS_MAX = _const(_NEU, "NEU_RUNS_MAX")
NEU_RUN_W = _const(_NEU, "NEU_RUN_W")
NEU_BIG_BLOCK = _const(_NEU, "NEU_BIG_BLOCK")
NEU_SUMS = _const(_NEU, "NEU_SUMS")
FUSED_MAX_N = _const(_NEU, "FUSED_MAX_N")
P_N, A_N, SC_N = _const(_DYN, "P_N"), _const(_DYN, "A_N"), _const(_DYN, "SC_N")
GATHER_MAX_INCIDENT = _const(_DYN, "GATHER_MAX_INCIDENT")
FUSED_DYN_BLOCK = _const(_DYN, "FUSED_DYN_BLOCK")
FUSED_DYN_MAX_G, FUSED_DYN_MAX_T = _const(_DYN, "FUSED_DYN_MAX_G"), _const(_DYN, "FUSED_DYN_MAX_T")
BACK_BLOCK = _const(_DYN, "BACK_BLOCK")
LDS_LIMIT = _const(_HOST, "LDS_LIMIT")
NEU_STATIC_LDS = 2 * 1024      # launch_eval_neutral's allowance for neu_big's static arrays
WAVES = NEU_BIG_BLOCK // 64


@dataclass
class Case:
    name: str
    fx: object
    path: str                       # the form the case was built for (bpl._ffi.PATH_<path>)
    wgs: int = 0                    # option dyn_big_wgs
    facts: dict = field(default_factory=dict)
    fix_z: Optional[Callable] = None   # (z, scale) -> None: pins sites of a test point


# ------------------------------------------------------------------------------------ neutral
def neutral_sorted(fx):
    """The device order of the fixtures -- stable sort by (venue, home, away, !(x <= 1 && y <= 1)) -- and the
    run key (home, away, venue, hc, ac) of each sorted fixture."""
    low = (fx.home_goals <= 1) & (fx.away_goals <= 1)
    skey = (fx.neutral << 33) | (fx.home_idx << 17) | (fx.away_idx << 1) | (~low).astype(np.int64)
    order = np.argsort(skey, kind="stable")
    hc = fx.home_conf if fx.n_conf else np.zeros(fx.n, np.int64)
    ac = fx.away_conf if fx.n_conf else np.zeros(fx.n, np.int64)
    rkey = (fx.home_idx << 33) | (fx.away_idx << 17) | ((fx.neutral != 0).astype(np.int64) << 16) | (hc << 8) | ac
    return order, rkey[order]


def neutral_facts(fx, wgs, neu_runs=1, fused_small=1):
    """The host's dispatch for neutral fixtures `fx` under dyn_big_wgs = wgs, and what decided it."""
    n, T, C, K = fx.n, fx.n_teams, fx.n_conf, fx.k
    _, rkey = neutral_sorted(fx)
    want = wgs if wgs > 0 else N_CU
    nbig = max(1, min(want, -(-n // NEU_BIG_BLOCK)))
    cap = -(-n // nbig)
    lds = (T * (2 * P_N + 2 * A_N) + 2 * C + SC_N + 4 * cap + NEU_SUMS + 2 * K + 2) * 8
    table_fits = WAVES * NEU_RUNS_MAX * NEU_RUN_W <= 2 * cap
    runs = np.zeros((nbig, WAVES), np.int64)       # runs (key changes + 1) of every wave's part
    heads = 0                                      # most run heads in one 64-fixture step of a wave
    heads_seen = set()                             # ... and every count that occurs
    n_mine = np.zeros(nbig, np.int64)
    for b in range(nbig):
        i_lo = min(b * cap, n)
        i_hi = min(i_lo + cap, n)
        n_mine[b] = i_hi - i_lo
        per_wave = -(-(i_hi - i_lo) // WAVES)
        for w in range(WAVES):
            w0 = min(w * per_wave, i_hi - i_lo)
            w1 = min(w0 + per_wave, i_hi - i_lo)
            part = rkey[i_lo + w0:i_lo + w1]
            if part.size == 0:
                continue
            runs[b, w] = 1 + np.count_nonzero(part[1:] != part[:-1])
            for s0 in range(0, part.size, 64):
                step = part[s0:s0 + 64]
                heads_seen.add(1 + int(np.count_nonzero(step[1:] != step[:-1])))
                heads = max(heads_seen)
    accepted = bool(table_fits and (2 * runs + 1 <= NEU_RUNS_MAX).all())
    lds_fits = lds + NEU_STATIC_LDS <= LDS_LIMIT
    if fused_small and n <= FUSED_MAX_N:
        path = "NEU_FUSED"   # (team / confederation counts and its own LDS bound are not restated: N decides here)
    elif fused_small and lds_fits:
        path = "NEU_BIG_RUNS" if accepted and neu_runs else "NEU_BIG_FIXTURE"
    else:
        path = "NEU_MULTI"
    return {"path": path, "nbig": nbig, "cap": cap, "n_mine": n_mine, "runs": runs, "max_runs": int(runs.max()),
            "table_fits": table_fits, "accepted": accepted, "lds_fits": lds_fits, "max_heads": heads, "heads_seen": heads_seen,
            "total_runs": 1 + int(np.count_nonzero(rkey[1:] != rkey[:-1]))}


def _neutral_case(name, fx, wgs, path, fix_z=None, **extra):
    facts = neutral_facts(fx, wgs)
    facts.update(extra)
    return Case(name, fx, path, wgs, facts, fix_z)


def _sorted_keys(T):
    """(venue, home, away) of every ordered pair at both venues, in the device's sort order."""
    return [(nv, h, a) for nv in (0, 1) for h in range(T) for a in range(T) if h != a]


def _from_counts(T, keys, counts, seed, n_conf=0, conf_of=None):
    """Fixtures with counts[j] copies of keys[j], goals and weights drawn at random, input order shuffled."""
    rs = np.random.RandomState(seed)
    nv = np.repeat([k[0] for k in keys], counts)
    h = np.repeat([k[1] for k in keys], counts)
    a = np.repeat([k[2] for k in keys], counts)
    n = h.size
    x, y, w = rs.poisson(1.4, n), rs.poisson(1.1, n), rs.uniform(0.2, 3.0, n)
    p = rs.permutation(n)
    h, a, nv, x, y, w = h[p], a[p], nv[p], x[p], y[p], w[p]
    if conf_of is None:
        conf_of = rs.randint(0, max(n_conf, 1), T)
    return NO.NeutralFixtures(h, a, x, y, nv, w, T, home_conf=conf_of[h] if n_conf else None,
                              away_conf=conf_of[a] if n_conf else None, n_conf=n_conf)


def runs_random():
    for T, n, wgs in ((4, 9000, 3), (5, 9000, 5), (6, 12000, 7), (5, 8193, 3), (3, 8200, 6)):
        yield _neutral_case(f"runs_random_T{T}_n{n}_w{wgs}", NO.synthetic_neutral(n, T, k=2, n_conf=3), wgs,
                            "NEU_BIG_RUNS")


def _capacity(m):
    T, n, per = 6, 10240, 20
    keys = _sorted_keys(T)
    rest = n - m * per
    counts = [per] * m + [rest // (len(keys) - m) + (j < rest % (len(keys) - m)) for j in range(len(keys) - m)]
    assert sum(counts) == n
    return _from_counts(T, keys, counts, seed=20 + m)


def runs_at_capacity():
    return _neutral_case("runs_at_capacity", _capacity(14), 4, "NEU_BIG_RUNS")


def runs_overflow():
    return _neutral_case("runs_overflow", _capacity(15), 4, "NEU_BIG_FIXTURE")


def heads_8_and_9():
    """Per-fixture form at the threshold of its straddling steps: wave 0's first step holds exactly 8 run
    heads (one set of adjoint atomics per run), its second exactly 9 (every lane for itself)."""
    T, n = 6, 10240
    keys = _sorted_keys(T)
    small = [8] * 8 + [7] * 8 + [8]
    rest, others = n - sum(small), len(keys) - len(small)
    counts = small + [rest // others + (j < rest % others) for j in range(others)]
    return _neutral_case("heads_8_and_9", _from_counts(T, keys, counts, seed=45), 4, "NEU_BIG_FIXTURE")


def runs_split_by_conf():
    """Per-fixture confederations: inside each (venue, home, away, low-flag) group, in input order, the first
    half has one (hc, ac) and the second half another, so every (venue, home, away) yields four runs."""
    fx = NO.synthetic_neutral(8400, 3, seed=31, n_conf=2)
    low = ((fx.home_goals <= 1) & (fx.away_goals <= 1)).astype(np.int64)
    grp = ((fx.neutral * 3 + fx.home_idx) * 3 + fx.away_idx) * 2 + low
    hc, ac = np.zeros(fx.n, np.int64), np.zeros(fx.n, np.int64)
    for g in np.unique(grp):
        idx = np.nonzero(grp == g)[0]            # input order
        first, second = idx[:idx.size // 2], idx[idx.size // 2:]
        if g & 1:                                # low scorelines (sorted first): (0,1) then (1,0)
            hc[first], ac[first], hc[second], ac[second] = 0, 1, 1, 0
        else:                                    # the others: (0,0) then (1,1)
            hc[first], ac[first], hc[second], ac[second] = 0, 0, 1, 1
    fx.home_conf, fx.away_conf = hc, ac
    return _neutral_case("runs_split_by_conf", fx, 3, "NEU_BIG_RUNS")


def conf_random_per_fixture():
    fx = NO.synthetic_neutral(8400, 3, seed=32, n_conf=2)
    rs = np.random.RandomState(33)
    fx.home_conf, fx.away_conf = rs.randint(0, 2, fx.n), rs.randint(0, 2, fx.n)
    return _neutral_case("conf_random_per_fixture", fx, 3, "NEU_BIG_FIXTURE")


CUT_KEY = (0, 1, 2)   # (venue, home, away) of runs_cut_everywhere's long run


def _cut_fix_z(T):
    sl = NO.site_slices(T)
    _, h, a = CUT_KEY

    def fix(z, scale):
        """The long run's pair gets the largest rate product, at its (home) venue only."""
        v = scale + 0.25
        for nm, t, sign in (("standardised_attack", h, 1), ("standardised_attack", a, 1),
                            ("standardised_defence", h, -1), ("standardised_defence", a, -1),
                            ("home_attack_decentered", h, 1), ("away_defence_decentered", a, -1),
                            ("away_attack_decentered", a, 1), ("home_defence_decentered", h, -1)):
            z[sl[nm].start + t] = sign * v
        for nm, sign in (("mean_home_attack", 1), ("mean_away_attack", 1), ("mean_home_defence", -1),
                         ("mean_away_defence", -1)):
            z[sl[nm]] = sign * scale
    return fix


def runs_cut_everywhere():
    """Sorted positions [2000, 3200) are ONE run: it crosses wave boundaries in two workgroups and the boundary
    between them, so several pieces propose a first fixture for the arg-extremal index; the last workgroup's
    share is a multiple of neither 8 nor 64."""
    T, n = 4, 8203
    keys = _sorted_keys(T)
    j = keys.index(CUT_KEY)
    assert j == 4
    rest = n - 4 * 500 - 1200
    others = len(keys) - 5
    counts = [500] * 4 + [1200] + [rest // others + (i < rest % others) for i in range(others)]
    fx = _from_counts(T, keys, counts, seed=41)
    order, _ = neutral_sorted(fx)
    sel = (fx.neutral[order] == CUT_KEY[0]) & (fx.home_idx[order] == CUT_KEY[1]) & (fx.away_idx[order] == CUT_KEY[2])
    pos = np.nonzero(sel)[0]
    return _neutral_case("runs_cut_everywhere", fx, 3, "NEU_BIG_RUNS", fix_z=_cut_fix_z(T),
                         cut_lo=int(pos[0]), cut_hi=int(pos[-1]) + 1, cut_contiguous=bool((np.diff(pos) == 1).all()))


LOW_ALL, LOW_NONE, LOW_ONE = (0, 0, 1), (0, 1, 0), (1, 2, 3)   # (venue, home, away) keys of low_classes


def low_classes():
    fx = NO.synthetic_neutral(8300, 4, seed=51)

    def of(key):
        return np.nonzero((fx.neutral == key[0]) & (fx.home_idx == key[1]) & (fx.away_idx == key[2]))[0]
    i = of(LOW_ALL)
    fx.home_goals[i[:8]] = [0, 1, 0, 1, 0, 1, 0, 1]
    fx.away_goals[i[:8]] = [0, 0, 1, 1, 0, 0, 1, 1]
    fx.home_goals[i[8]], fx.away_goals[i[8]] = 255, 3
    fx.home_goals[i[9]], fx.away_goals[i[9]] = 0, 255
    i = of(LOW_NONE)
    fx.home_goals[i] += 2
    i = of(LOW_ONE)
    fx.home_goals[i], fx.away_goals[i] = 1, 0
    fx.weights[::7] = 1e-6
    fx.weights[3::11] = 3e-4
    return _neutral_case("low_classes", fx, 3, "NEU_BIG_RUNS")


def venues():
    for name, nv in (("venues_all_neutral", 1), ("venues_all_home", 0)):
        fx = NO.synthetic_neutral(8300, 4, seed=61, k=1)
        fx.neutral[:] = nv
        fx.n_teams = 5          # team 4 plays no fixture
        fx.covariates = np.random.RandomState(62).normal(size=(5, 1))
        yield _neutral_case(name, fx, 3, "NEU_BIG_RUNS")


def many_pairs():
    return _neutral_case("many_pairs", NO.synthetic_neutral(9000, 150, k=2), 7, "NEU_BIG_FIXTURE")


def lds_fallback():
    return _neutral_case("lds_fallback", NO.synthetic_neutral(9000, 5, n_conf=3), 1, "NEU_MULTI")


def _far_fix_z(T):
    sl = NO.site_slices(T)

    def fix(z, scale):
        for nm in ("mean_home_attack", "mean_away_attack", "mean_defence"):
            z[sl[nm]] = 320.0
    return fix


def far_records():
    """Cell records beyond +-300 with rates of order one (neu_big then takes exp of the differences, s_slow:
    assumed, the path getter cannot show it)."""
    fx = NO.synthetic_neutral(8300, 4, seed=71)
    fx.neutral[:] = 0
    return _neutral_case("far_records", fx, 3, "NEU_BIG_RUNS", fix_z=_far_fix_z(4))


def neutral_cases():
    out = list(runs_random())
    out += [runs_at_capacity(), runs_overflow(), heads_8_and_9(), runs_split_by_conf(), conf_random_per_fixture(),
            runs_cut_everywhere(), low_classes()]
    out += list(venues())
    out += [many_pairs(), lds_fallback(), far_records()]
    return out


NEUTRAL_POINTS = ((1, 0.2), (2, 0.5), (3, 1.0))   # (seed, scale): z uniform in +-scale, as tests/test_gpu_neutral.py


def neutral_points(case):
    D = NO.latent_dim(case.fx.n_teams, case.fx.k, case.fx.n_conf)
    for seed, scale in NEUTRAL_POINTS:
        z = np.random.RandomState(seed).uniform(-scale, scale, D)
        if case.fix_z:
            case.fix_z(z, scale)
        yield seed, scale, z


# ------------------------------------------------------------------------------------ dynamic
def dynamic_facts(fx, wgs=0, dyn_gather=1, fused_small=1):
    """The host's dispatch for dynamic fixtures `fx`, and the (gameweek, team) cells' incidence lists."""
    G, T, n = fx.n_gameweeks, fx.n_teams, fx.n
    cell_h, cell_a = fx.gameweek * T + fx.home_idx, fx.gameweek * T + fx.away_idx
    length = np.bincount(cell_h, minlength=G * T) + np.bincount(cell_a, minlength=G * T)
    home_n = np.bincount(cell_h, minlength=G * T)
    neutral_n = np.bincount(cell_h, fx.neutral, G * T) + np.bincount(cell_a, fx.neutral, G * T)
    team_blocks = -(-T // (BACK_BLOCK // 64))
    fused_shape = fused_small and G <= FUSED_DYN_MAX_G and T <= FUSED_DYN_MAX_T
    small = fused_shape and wgs <= 0 and n <= team_blocks * FUSED_DYN_BLOCK * 4 and team_blocks <= N_CU
    gather = bool(length.max() <= GATHER_MAX_INCIDENT and n < (1 << 30))
    if small:
        path = "DYN_FUSED_GATHER" if gather and dyn_gather else "DYN_FUSED_ATOMICS"
    else:
        path = "DYN_SLICED" if fused_shape else "DYN_MULTI"   # (the sliced form's LDS / residency bounds are not restated)
    return {"path": path, "length": length, "histogram": np.bincount(length), "longest": int(length.max()),
            "gather": gather, "mixed_sides": int(np.count_nonzero((home_n > 0) & (home_n < length))),
            "mixed_venues": int(np.count_nonzero((neutral_n > 0) & (neutral_n < length))),
            "empty_gameweeks": [g for g in range(G) if not (fx.gameweek == g).any()]}


GATHER_CELL = (2, 5)   # (gameweek, team) of the list that gather_lists brings to exactly GATHER_MAX_INCIDENT


def _gather_fixtures(extra=0):
    T, G, n = 13, 6, 200
    rs = np.random.RandomState(81)
    h = rs.randint(0, T, n)
    a = (h + 1 + rs.randint(0, T - 1, n)) % T
    gw = rs.choice([0, 1, 2, 3, 5], n)             # gameweek 4 is empty
    nv = (rs.rand(n) < 0.4).astype(np.int64)
    x, y = rs.poisson(1.5, n), rs.poisson(1.2, n)
    g0, t0 = GATHER_CELL
    length = np.bincount(gw * T + h, minlength=G * T) + np.bincount(gw * T + a, minlength=G * T)
    add_h, add_a, add_nv = [], [], []
    need = GATHER_MAX_INCIDENT + extra - length[g0 * T + t0]
    assert need > 0
    for j in range(need):                          # against the opponents with the shortest lists, sides and venues alternating
        row = length[g0 * T:(g0 + 1) * T].copy()
        row[t0] = 1 << 20
        opp = int(np.argmin(row))
        length[g0 * T + opp] += 1
        length[g0 * T + t0] += 1
        add_h.append(t0 if j % 2 == 0 else opp)
        add_a.append(opp if j % 2 == 0 else t0)
        add_nv.append((j // 2) % 2)
    m = len(add_h)
    h, a, nv = np.concatenate([h, add_h]), np.concatenate([a, add_a]), np.concatenate([nv, add_nv])
    gw = np.concatenate([gw, np.full(m, g0)])
    x, y = np.concatenate([x, rs.poisson(1.5, m)]), np.concatenate([y, rs.poisson(1.2, m)])
    return DO.DynFixtures(h, a, x, y, gw, nv, T, G)


def gather_lists():
    fx = _gather_fixtures()
    return Case("gather_lists", fx, "DYN_FUSED_GATHER", 0, dynamic_facts(fx))


def gather_17():
    fx = _gather_fixtures(extra=1)
    return Case("gather_17", fx, "DYN_FUSED_ATOMICS", 0, dynamic_facts(fx))


def config4():
    fx = DO.config4_recipe()
    return Case("config4", fx, "DYN_FUSED_GATHER", 0, dynamic_facts(fx))


def dynamic_cases():
    return [gather_lists(), gather_17(), config4()]


def dynamic_points(case):
    """The two points of tests/test_gpu_dynamic.py: seed 2 lifts mean_home_attack so that M > 1 and the upper
    bound's adjoint binds."""
    fx = case.fx
    D = DO.latent_dim(fx.n_gameweeks, fx.n_teams, fx.k)
    sl = DO.site_slices(fx.n_gameweeks, fx.n_teams, fx.k)
    for seed in (7, 2):
        z = np.random.RandomState(seed).uniform(-0.3, 0.3, D)
        if seed == 2:
            z[sl["mean_home_attack"]] = 1.2
        yield seed, z
