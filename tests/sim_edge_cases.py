"""Hand-built posteriors and calls that put the three base simulators (csrc/dc_season.hip.h,
csrc/dc_tournament.hip.h, csrc/dc_ppc.hip.h) on the edges of their shapes, of the shared sampler
(csrc/dc_sampler.hip.h) and of the shared league table (csrc/dc_table.hip.h).

tests/test_gpu_season_edges.py, tests/test_gpu_tournament_edges.py and tests/test_gpu_ppc_edges.py run
the cases on the device against the numpy restatements; tests/test_sim_edge_cases_host.py checks on the
CPU that every case still sits on the edge it was built for and that the restatement flags none of its
simulations (so every comparison on the device is an exact one over all of them).

Each builder returns a Case: the model, the keyword arguments of the public call, and the facts that
make it an edge.  A case's restatement is computed once per process (`season_reference`,
`tournament_reference`, `ppc_reference`) and shared by every test that asks for it.
"""
import itertools
from dataclasses import dataclass, field

import numpy as np

import loglik_ref as LR
import ppc_ref as PR
import season_ref as SR
import tournament_ref as TR
from bpl import (DixonColesMatchPredictor, ExtendedDixonColesMatchPredictor, NeutralDixonColesMatchPredictor)
from bpl.base import _prng_key
from bpl.neutral_dixon_coles import tournament_result

# the sampler ladder: log-rates from "never a goal" to "always at the cap of 255"
LADDER_LOG = (-40.0, -5.0, float(np.log(0.05)), 0.0, float(np.log(5.0)), float(np.log(20.0)), float(np.log(60.0)),
              float(np.log(150.0)), float(np.log(300.0)), 6.5)
LEVEL_LOG = -40.0                     # exp(-exp(-40)) == 1.0 in float64: every scoreline is 0-0
TABLE_LIMITS = (0, (1 << 24) - 1, 1 << 24)   # BPLHIP_SEASON_MAX_TABLE_VALUE and its neighbours
RHO_KINDS = ("zero", "lower", "upper", "clip_pos", "clip_neg")
# key (0, EQUAL_WORDS_SEED): in simulation 0 slots EQUAL_WORDS_SLOTS of a 64-slot table draw the same
# tie-break word (the host test recomputes the words).  The search, should the counter layout ever change:
# for seed = 0, 1, 2, ... take tiebreak_words(seed, 1, 64)[0] -- the o0 words of the blocks
# (0, TIEBREAK_COUNTER | slot) under key (0, seed) -- and stop at the first seed with two equal words among
# the 64 (expected after about 2e6 seeds) or, for the group key below, with two equal words among the eight
# slots 8g..8g+7 of one group (expected after about 2e7 seeds; this one came at 5.5e7)
EQUAL_WORDS_SEED = 2462971
EQUAL_WORDS_SLOTS = (21, 36)
# ... and key (0, GROUP_EQUAL_WORDS_SEED): two slots of ONE group of eight (slots 48..55) draw the same word
GROUP_EQUAL_WORDS_SEED = 55198951
GROUP_EQUAL_WORDS_SLOTS = (51, 53)


@dataclass
class Case:
    name: str
    model: object
    call: dict                          # keyword arguments of the public method
    facts: dict = field(default_factory=dict)


_REFERENCES = {}


def _once(kind, case, compute):
    k = (kind, case.name)
    if k not in _REFERENCES:
        _REFERENCES[k] = compute()
    return _REFERENCES[k]


# ------------------------------------------------------------------------------------ models
def _names(T):
    return np.array([f"t{i:03d}" for i in range(T)])


def league_model(T, S, seed, extended=False):
    """A plain (per-draw home advantage) or extended (per-team, [S, T]) posterior at league-like rates."""
    rs = np.random.RandomState(seed)
    m = ExtendedDixonColesMatchPredictor() if extended else DixonColesMatchPredictor()
    m.teams = _names(T)
    m._teams_dict = {t: i for i, t in enumerate(m.teams)}
    m.attack, m.defence = rs.normal(0, 0.3, (S, T)), rs.normal(0, 0.3, (S, T))
    m.home_advantage = rs.normal(0.25, 0.1, (S, T)) if extended else rs.normal(0.25, 0.05, S)
    m.corr_coef = rs.uniform(-0.1, 0.1, S)
    return m


def neutral_model(T, S, seed):
    rs = np.random.RandomState(seed)
    m = NeutralDixonColesMatchPredictor()
    m.teams = _names(T)
    m._teams_dict = {t: i for i, t in enumerate(m.teams)}
    m.attack, m.defence = rs.normal(0, 0.3, (S, T)), rs.normal(0, 0.3, (S, T))
    for nm in ("home_attack", "away_attack", "home_defence", "away_defence"):
        setattr(m, nm, rs.normal(0, 0.1, (S, T)))
    m.corr_coef = rs.uniform(-0.05, 0.05, S)
    return m


def _flatten(m, log_rate):
    """Every team scores at exp(log_rate) against every other, at any venue, with rho = 0."""
    m.attack[:] = log_rate
    m.defence[:] = 0.0
    m.corr_coef[:] = 0.0
    for nm in ("home_advantage", "home_attack", "away_attack", "home_defence", "away_defence"):
        if getattr(m, nm, None) is not None:
            getattr(m, nm)[:] = 0.0
    return m


def ladder_model(rho_kind, S=1):
    """20 teams, two per rung of LADDER_LOG (team i and team 10 + i score at exp(LADDER_LOG[i]) against
    anyone), and the fixtures i v 10 + j and 10 + j v i for every pair of rungs: 200 fixtures whose
    (home, away) rates take every pair of rungs twice.  rho: 0, 1e-6 inside the bound over these
    fixtures on either side, or beyond it in either direction."""
    m = _flatten(league_model(20, S, seed=0), 0.0)
    m.attack[:] = np.tile(LADDER_LOG, 2)[None, :]
    i, j = np.meshgrid(np.arange(10), np.arange(10), indexing="ij")
    h = np.concatenate([i.ravel(), 10 + j.ravel()]).astype(np.uint16)
    a = np.concatenate([10 + j.ravel(), i.ravel()]).astype(np.uint16)
    lh, la = np.exp(m.attack[0, h]), np.exp(m.attack[0, a])
    lo = float(np.max(np.maximum(-1.0 / lh, -1.0 / la)))
    hi = float(np.min(np.minimum(1.0 / (lh * la), 1.0)))
    rho = {"zero": 0.0, "lower": lo + 1e-6, "upper": hi - 1e-6, "clip_pos": 0.9, "clip_neg": -1.1}[rho_kind]
    m.corr_coef[:] = rho
    clipped = (1 - lh * la * rho < 0) | (1 + lh * rho < 0) | (1 + la * rho < 0)
    facts = {"rho": rho, "bounds": (lo, hi), "clipped": int(clipped.sum()), "log_home": m.attack[0, h],
             "log_away": m.attack[0, a]}
    return m, h, a, facts


# ------------------------------------------------------------------------------------ season
SEASON_SHAPES = ((2, 2, 1, 1, 1), (3, 3, 63, 7, 5), (64, 64, 64, 257, 64), (64, 64, 65, 257, 300),
                 (300, 64, 129, 65, 3), (20, 20, 380, 1025, 1000))     # (T, n, nf, N, S)
SEASON_SMALL = SEASON_SHAPES[:3]


def _season_inputs(case):
    kw = case.call
    return case.model._season_inputs(kw["home_team"], kw["away_team"], kw["num_simulations"], kw.get("current_table"),
                                     kw.get("teams"), kw.get("points", (3, 1, 0)))


def season_reference(case):
    """(the restatement's dict, the table's model indices in slot order) of a season case."""
    def compute():
        m = case.model
        h, a, table_idx, table, points, n = _season_inputs(case)
        ref = SR.simulate_season(m.attack, m.defence, m.home_advantage, m.corr_coef, h, a, table_idx, table, points, n,
                                 _prng_key(case.call["random_state"]))
        return ref, table_idx
    return _once("season", case, compute)


def season_reference_in_order(case, slot_order):
    """The restatement with the table's slots in `slot_order` (a permutation of the case's table, model
    indices), as the context takes them: (dict, the [n, 3] current table in that order)."""
    def compute():
        m = case.model
        h, a, table_idx, table, points, n = _season_inputs(case)
        row = {int(t): table[i] for i, t in enumerate(table_idx)}
        tab = np.array([row[int(t)] for t in slot_order], dtype=np.int64).reshape(len(slot_order), 3)
        ref = SR.simulate_season(m.attack, m.defence, m.home_advantage, m.corr_coef, h, a, slot_order, tab, points, n,
                                 _prng_key(case.call["random_state"]))
        return ref, tab
    return _once("season_in_order", case, compute)


def season_keys(case):
    """The restatement's ranking keys (points, goal difference, goals for) [N, n] as Python-sized integers."""
    ref, table_idx = season_reference(case)
    h, a, _, table, _, N = _season_inputs(case)
    slot = {int(t): i for i, t in enumerate(table_idx)}
    gf, ga = np.tile(table[:, 1], (N, 1)), np.tile(table[:, 2], (N, 1))
    x, y = ref["home_goals"].astype(np.int64), ref["away_goals"].astype(np.int64)
    for f in range(h.size):
        hs, as_ = slot[int(h[f])], slot[int(a[f])]
        gf[:, hs] += x[:, f]
        ga[:, hs] += y[:, f]
        gf[:, as_] += y[:, f]
        ga[:, as_] += x[:, f]
    return ref["points"].astype(np.int64), gf - ga, gf


def tiebreak_words(seed, N, n):
    """The slots' tie-break words [N, n] under random_state = seed."""
    r, _ = SR.threefry_block(_prng_key(seed), np.arange(N, dtype=np.uint32)[:, None],
                             (SR.TIEBREAK_COUNTER | np.arange(n)).astype(np.uint32)[None, :])
    return r.astype(np.int64)


def _pairs(rs, n, nf):
    """nf fixtures among slots 0..n-1, no team against itself."""
    h = rs.randint(0, n, nf)
    a = (h + 1 + rs.randint(0, n - 1, nf)) % n
    return h, a


def season_shape(T, n, nf, N, S):
    rs = np.random.RandomState(1000 + T + nf)
    m = league_model(T, S, seed=T + N, extended=T > 64)
    call = {"num_simulations": N, "random_state": 77 + nf}
    facts = {"shape": (T, n, nf, N, S)}
    if T == n:
        h, a = _pairs(rs, n, nf)
        call["current_table"] = {m.teams[i]: (int(rs.randint(0, 60)), int(rs.randint(0, 70)), int(rs.randint(0, 70)))
                                 for i in range(0, T, 2)}
        call["teams"] = list(m.teams)
    else:
        # a scattered subset of the model, listed out of model order; only the first 50 listed teams play
        listed = rs.choice(T, n, replace=False)
        assert (np.diff(listed) < 0).any()
        ph, pa = _pairs(rs, 50, nf)
        h, a = listed[ph], listed[pa]
        call["teams"] = [m.teams[i] for i in listed]
        call["current_table"] = {m.teams[i]: (int(rs.randint(0, 60)), int(rs.randint(0, 70)), int(rs.randint(0, 70)))
                                 for i in listed[::3]}
        facts["listed"] = listed.astype(np.uint16)
        facts["idle"] = sorted(set(listed.tolist()) - set(h.tolist()) - set(a.tolist()))
    call["home_team"], call["away_team"] = h.astype(np.uint16), a.astype(np.uint16)
    return Case("shape_T%d_n%d_nf%d_N%d_S%d" % (T, n, nf, N, S), m, call, facts)


def season_shapes():
    return [season_shape(*s) for s in SEASON_SHAPES]


def season_ladder(rho_kind):
    m, h, a, facts = ladder_model(rho_kind, S=1)
    call = {"home_team": h, "away_team": a, "num_simulations": 129, "random_state": 5150,
            "current_table": {m.teams[19]: (1, 2, 3)}}
    return Case("ladder_" + rho_kind, m, call, facts)


def season_ladders():
    return [season_ladder(k) for k in RHO_KINDS]


def season_level(n, table, seed=31, N=65):
    """Every match 0-0 and every team plays once, on a level current table (or none): every slot ties on
    points, goal difference and goals for, and the tie-break word orders the table."""
    m = _flatten(league_model(n, 2, seed=n), LEVEL_LOG)
    h, a = np.arange(0, n, 2, dtype=np.uint16), np.arange(1, n, 2, dtype=np.uint16)
    call = {"home_team": h, "away_team": a, "num_simulations": N, "random_state": seed, "teams": list(m.teams)}
    if table is not None:
        call["current_table"] = {t: table for t in m.teams}
    return Case("level_n%d_%s_seed%d" % (n, "table" if table else "empty", seed), m, call, {"table": table})


def season_levels():
    return [season_level(8, None), season_level(8, (7, 3, 3)), season_level(64, None), season_level(64, (7, 3, 3)),
            season_equal_words()]


def season_equal_words():
    """The level 64-slot table under the key for which two slots draw the SAME word in simulation 0: the
    slot index decides between them."""
    c = season_level(64, None, seed=EQUAL_WORDS_SEED, N=3)
    c.name = "level_equal_words"
    c.facts["equal_slots"] = EQUAL_WORDS_SLOTS
    return c


def season_sparse():
    """Ordinary rates, four fixtures among eight teams: every simulation has teams level on points, and
    in many two are level on all three keys."""
    m = league_model(8, 16, seed=12)
    call = {"home_team": np.array([0, 2, 4, 6], dtype=np.uint16), "away_team": np.array([1, 3, 5, 7], dtype=np.uint16),
            "num_simulations": 500, "random_state": 99}
    return Case("sparse_8", m, call)


def limit_rows():
    """All 27 (points, GF, GA) rows over TABLE_LIMITS: goal differences of -2^24 and +2^24 among them."""
    return list(itertools.product(TABLE_LIMITS, repeat=3))


def season_limits(points):
    rows = limit_rows()
    n = len(rows)
    m = league_model(n, 8, seed=27)
    h, a = _pairs(np.random.RandomState(28), n, 6)
    call = {"home_team": h.astype(np.uint16), "away_team": a.astype(np.uint16), "num_simulations": 65, "random_state": 2424,
            "current_table": {m.teams[i]: rows[i] for i in range(n)}, "points": points}
    return Case("limits_%d_%d_%d" % points, m, call, {"rows": rows})


def season_limit_cases():
    return [season_limits((1000, 1, 0)), season_limits((0, 0, 0))]


def season_cases():
    return season_shapes() + season_ladders() + season_levels() + [season_sparse()] + season_limit_cases()


# ------------------------------------------------------------------------------------ tournament
# (groups, size, advance, best_of_rest, bracket)
TOURNAMENT_FORMATS = ((2, 2, 1, 0, 2), (4, 3, 1, 0, 4), (8, 8, 2, 0, 16), (8, 8, 4, 0, 32), (3, 5, 2, 2, 8),
                      (16, 4, 2, 0, 32))
TOURNAMENT_COUNTS = ((1, 1), (7, 64), (257, 3))     # (N, S)
KNOCKOUT_BRACKETS = (2, 4, 64)


def tournament_inputs(case):
    kw = case.call
    return case.model._tournament_inputs(kw["knockout"], kw.get("groups"), kw.get("advance", 2), kw.get("best_of_rest", 0),
                                         kw.get("group_fixtures"), kw.get("current_table"), kw.get("hosts"),
                                         kw.get("points", (3, 1, 0)), kw["num_simulations"], None)


def tournament_reference(case):
    """(checked inputs, the restatement's raw dict, simulate_tournament's dict from it) of a tournament case."""
    def compute():
        inp = tournament_inputs(case)
        ref = TR.simulate_tournament(TR.model_tables(case.model), inp, _prng_key(case.call["random_state"]))
        return inp, ref, tournament_result(inp, ref)
    return _once("tournament", case, compute)


def _group_call(m, fmt, N, seed):
    g, size, adv, best, nb = fmt
    kw = TR.group_format(list(m.teams), g, size, best, seed=seed, advance=adv)
    assert len(kw["knockout"]) == nb
    kw.update(num_simulations=N, random_state=1000 + seed)
    return kw


def tournament_format(fmt, N, S):
    m = neutral_model(64, S, seed=fmt[0] + N)
    return Case("format_%dx%d_adv%d_best%d_ko%d_N%d_S%d" % (fmt + (N, S)), m, _group_call(m, fmt, N, seed=fmt[1] + N),
                {"format": fmt})


def tournament_formats():
    return [tournament_format(f, N, S) for f in TOURNAMENT_FORMATS for N, S in TOURNAMENT_COUNTS]


def tournament_knockout(nb, N, S):
    m = neutral_model(64, S, seed=nb + N)
    teams = list(np.random.RandomState(nb).permutation(m.teams)[:nb])
    return Case("knockout_%d_N%d_S%d" % (nb, N, S), m, {"knockout": teams, "num_simulations": N, "random_state": 300 + nb})


def tournament_knockouts():
    return [tournament_knockout(nb, N, S) for nb in KNOCKOUT_BRACKETS for N, S in TOURNAMENT_COUNTS]


def tournament_hosts():
    """A host listed second in its pairing (the venue swap runs) and one listed first, in a knockout-only
    bracket and in a group stage."""
    m = neutral_model(64, 16, seed=41)
    # the home tables well away from zero, so that a missed swap changes the rates
    m.home_attack += 0.4
    m.away_defence -= 0.3
    t = list(m.teams)
    ko = Case("hosts_knockout_8", m, {"knockout": t[:8], "hosts": [t[1], t[6]], "num_simulations": 257, "random_state": 51})
    kw = _group_call(m, (4, 4, 2, 0, 8), 257, seed=52)
    kw["hosts"] = [t[2], t[4]]     # third of group A: listed second against t000 and t001, first against t003
    return [ko, Case("hosts_groups_4x4", m, kw)]


def tournament_level_knockouts():
    """Every rate e^-40: all 32 attempts of every knockout match end 0-0 and the first-listed entry goes
    through, also where a host listed second is the home side."""
    out = []
    for nb, N in ((2, 3), (8, 5), (64, 5)):
        m = _flatten(neutral_model(64, 2, seed=nb), LEVEL_LOG)
        t = list(m.teams[:nb])
        hosts = [t[1]] + ([t[5], t[6]] if nb > 2 else [])
        out.append(Case("level_knockout_%d" % nb, m, {"knockout": t, "hosts": hosts, "num_simulations": N,
                                                      "random_state": 60 + nb}))
    return out


def tournament_level_groups():
    """Every group match 0-0 on a level table (or none): the group order and the best-of-rest order come
    from the tie-break words alone."""
    out = []
    for table in (None, (4, 2, 2)):
        m = _flatten(neutral_model(64, 2, seed=7), LEVEL_LOG)
        kw = _group_call(m, (3, 5, 2, 2, 8), 65, seed=70)
        kw["hosts"] = [m.teams[3]]
        if table:
            kw["current_table"] = {t: table for g in kw["groups"].values() for t in g}
        out.append(Case("level_groups_3x5_%s" % ("table" if table else "empty"), m, kw, {"table": table}))
    return out


def tournament_equal_words():
    """Eight level groups of eight under the key for which two slots of one group draw the SAME word in
    simulation 0: the slot index decides their places."""
    m = _flatten(neutral_model(64, 2, seed=8), LEVEL_LOG)
    kw = _group_call(m, (8, 8, 2, 0, 16), 3, seed=71)
    kw["random_state"] = GROUP_EQUAL_WORDS_SEED
    return Case("level_groups_8x8_equal_words", m, kw, {"equal_slots": GROUP_EQUAL_WORDS_SLOTS})


def tournament_limits(points):
    """A mid-tournament table over TABLE_LIMITS: 8 groups of 4 with two matches left in each."""
    m = neutral_model(64, 8, seed=81)
    kw = _group_call(m, (8, 4, 2, 0, 16), 65, seed=82)
    teams = [t for g in kw["groups"].values() for t in g]
    rows = limit_rows()
    order = np.random.RandomState(83).permutation(len(teams))     # rows spread over the groups
    kw["current_table"] = {teams[order[i]]: rows[i] for i in range(len(rows))}
    kw["group_fixtures"] = [(g[0], g[3]) for g in kw["groups"].values()] + [(g[2], g[1]) for g in kw["groups"].values()]
    kw["points"] = points
    return Case("limits_%d_%d_%d" % points, m, kw, {"rows": rows})


def tournament_limit_cases():
    return [tournament_limits((1000, 1, 0)), tournament_limits((0, 0, 0))]


def tournament_cases():
    return (tournament_formats() + tournament_knockouts() + tournament_hosts() + tournament_level_knockouts()
            + tournament_level_groups() + [tournament_equal_words()] + tournament_limit_cases())


def level_knockout_stage(nb):
    """The closed form of a bracket whose first-listed entry always goes through: entry 0 wins the final
    (stage R + 1), entry e > 0 goes out in round r = its number of trailing zero bits (stage r + 1)."""
    R = nb.bit_length() - 1
    return np.array([R + 1] + [1 + ((e & -e).bit_length() - 1) for e in range(1, nb)], dtype=np.uint8)


# ------------------------------------------------------------------------------------ ppc
PPC_FIXTURE_COUNTS = (1, 255, 256, 257, 1025)
PPC_COUNTS = ((1, 1), (1, 64), (63, 64), (65, 64), (5, 1))     # (R, S)


def ppc_reference(case):
    """(x, y int64 [R, m], flagged [R]) of a ppc case: the restatement's replications."""
    kw = case.call
    return _once("ppc", case, lambda: PR.replicate(case.model, kw["data"], kw["num_replications"],
                                                   _prng_key(kw["random_state"]), fixture_id=case.facts.get("fixture_id")))


def _ppc_case(name, m, d, R, seed, G, **facts):
    return Case(name, m, {"data": d, "num_replications": R, "random_state": seed, "max_goals": G}, facts)


def ppc_fixture_counts():
    out = []
    for kind in ("basic", "wc"):
        for n in PPC_FIXTURE_COUNTS:
            m = LR.hand_model(kind, S=8, T=8, seed=n)
            out.append(_ppc_case("fixtures_%s_%d" % (kind, n), m, LR.hand_data(m, n=n, seed=n + 1), 3, 13, 4))
    return out


def ppc_team_slots():
    m2 = LR.hand_model("basic", S=8, T=2, seed=2)
    m130 = LR.hand_model("basic", S=8, T=130, seed=130)
    d = LR.hand_data(m130, n=300, seed=131)
    teams = list(m130.teams)
    d["home_team"][:130] = teams                      # every team at least once
    d["away_team"][:130] = teams[1:] + teams[:1]
    return [_ppc_case("slots_2", m2, LR.hand_data(m2, n=30, seed=3), 3, 14, 4),
            _ppc_case("slots_130", m130, d, 3, 15, 4)]


def ppc_ladder(G):
    """The sampler ladder as observed fixtures: replicated goals from 0 to the cap of 255 on either axis,
    observed goals inside the grid, beyond it on one axis and on both, and at 255."""
    m, h, a, facts = ladder_model("zero", S=1)
    n = h.size
    rs = np.random.RandomState(16)
    x, y = rs.randint(0, 3, n), rs.randint(0, 3, n)
    x[:6] = [0, G + 1, 0, G + 1, 255, 255]
    y[:6] = [0, 0, G + 1, G + 1, 255, 0]
    d = {"home_team": [m.teams[i] for i in h], "away_team": [m.teams[i] for i in a], "home_goals": x, "away_goals": y}
    return _ppc_case("ladder_G%d" % G, m, d, 5, 17, G, **facts)


def ppc_grid_depths():
    m = LR.hand_model("basic", S=8, T=8, seed=18)
    d = LR.hand_data(m, n=70, seed=19)
    return [_ppc_case("depth_1", m, d, 40, 20, 1), _ppc_case("depth_15", m, d, 40, 20, 15), ppc_ladder(1), ppc_ladder(15)]


def ppc_counts():
    out = []
    for R, S in PPC_COUNTS:
        m = LR.hand_model("basic", S=S, T=8, seed=R + S)
        out.append(_ppc_case("counts_R%d_S%d" % (R, S), m, LR.hand_data(m, n=70, seed=21), R, 22, 4))
    return out


def ppc_fixture_ids():
    """Counters that are neither contiguous nor small, through the context's ppc."""
    m = LR.hand_model("basic", S=8, T=8, seed=23)
    n = 300
    rs = np.random.RandomState(24)
    fid = rs.randint(0, 1 << 32, n, dtype=np.int64)
    fid[:5] = [(1 << 32) - 1, 0, 1 << 31, (1 << 31) - 1, 1 << 30]
    fid[7] = 7                                        # one fixture whose counter is its position
    assert np.unique(fid).size == n
    return _ppc_case("fixture_ids", m, LR.hand_data(m, n=n, seed=25), 7, 26, 5, fixture_id=fid)


def ppc_cases():
    return ppc_fixture_counts() + ppc_team_slots() + ppc_grid_depths() + ppc_counts()


def release(model):
    """Close the model's device context (the cases live as long as the test session; their contexts need not)."""
    ctx = getattr(model, "_predict_ctx", None)
    if ctx is not None:
        ctx.close()
        model._predict_ctx = None
        model._uploaded = None
