"""The runs of tests/test_gpu_draw_stats.py: which sampler engine is reached with which league / neutral / dynamic
fixture, the two run shapes, the gates, and the float64 oracle of every family evaluated AT THE DRAWS THE DEVICE
RETURNED (no golden: the check works on adapted chains as well).  tests/test_draw_stats_cases_host.py keeps every
statement of this file true on the CPU.

What is pinned: per kept draw i, `potential_energy[i]` is the oracle's U(draws[i]) and `corr_coef[i]` the oracle's
rho(draws[i]).  The second is a pure sampler statistic for the venue classes -- aux[0] of the evaluation at the
accepted proposal, carried through every tree merge -- and nothing recomputes it from the draw.

The gates are those the families' parity tests put on one evaluation (tests/test_gpu_parity.py,
tests/test_gpu_neutral.py, tests/test_gpu_dynamic.py); the persistent engines are bit-identical to one launch per
leapfrog (tests/test_gpu_soak.py), so the same gates hold for them.
"""
import numpy as np

import cases
import dc_dynamic_oracle as DO
import dc_neutral_oracle as NO
import dc_oracle as O
import sampler_cases as SC

KEY = SC.KEY
# the two run shapes: (num_warmup, num_samples, thinning, max_tree_depth, step_size or None for the default)
FIXED = dict(num_warmup=0, num_samples=12, thinning=1, max_tree_depth=5, step_size=SC.STEP)
ADAPTED = dict(num_warmup=40, num_samples=21, thinning=2, max_tree_depth=4, step_size=None)   # 10 kept draws
# thinning alignment: kept row j of a thinning = 3 run of 14 samples is iteration 14 % 3 + 3 j + 2 of the same chain
THIN = dict(num_warmup=0, num_samples=14, thinning=3, max_tree_depth=5, step_size=SC.STEP)
SENSITIVITY, MIN_FRACTION = 100.0, 0.75
RHO_GATE = {"league": 1e-6, "neutral": 1e-12, "dynamic": 1e-12}


def kept_rows(num_samples, thinning):
    """nuts.hpp ChainDriver::end: with start_idx = num_warmup + num_samples % thinning, iteration `it` is kept when
    it >= start_idx and (it - start_idx) % thinning == thinning - 1, as row (it - start_idx) / thinning.  In
    post-warm-up iterations: row j is iteration num_samples % thinning + thinning * j + thinning - 1."""
    return [num_samples % thinning + thinning * j + thinning - 1 for j in range(num_samples // thinning)]


def u_gate(family, n_fixtures, U):
    if family == "league":
        return cases.u_tolerance(n_fixtures, U)
    return (1e-11 if family == "neutral" else 1e-9) * abs(U)


# ------------------------------------------------------------------------------------------------- the league
def league_single_runs():
    """(engine, case, setting) for every engine a single league chain reaches: the bindable case of SC.ALL with the
    smallest D that some setting of SC.SETTINGS dispatches to it (the first such case and setting).  SC.FINE cases
    are left out: at SC.STEP their chain never leaves its start (every transition diverges at its first leaf), and a
    column that does not change cannot be seen shifted."""
    out = []
    for engine in sorted({e for c in SC.ALL for e in c.engines}):
        hits = [(c.D, i, j, c.name, s) for i, c in enumerate(SC.ALL) for j, s in enumerate(SC.SETTINGS)
                if c.bindable and c.name not in SC.FINE and c.engine(s) == engine]
        _, _, _, name, setting = min(hits)
        out.append((engine, name, setting))
    return out


def league_fixed(case):
    """The fixed-step run shape of a league case: SC.STEP where the leaf sits in dc_eval's tail.  The kp_leaf /
    kw_leaf cases (D >= 255) take SC.FINE_STEP: at SC.STEP ten or eleven of their twelve transitions diverge in the
    float64 restatement, the chain stays put and the sensitivity condition cannot hold (0.73 and 0.36 of the pairs
    apart for b255 and e257); at SC.FINE_STEP none diverges and at least 0.9 of the pairs are apart."""
    return FIXED if case.tail else dict(FIXED, step_size=SC.FINE_STEP)


MULTI_CASE = min(SC.MULTI, key=lambda n: SC.CASES[n].D)
CHAIN_COUNTS = (2, 3, 9)
LOCKSTEP_CASE = "e128w"        # the case sampler_cases.engines_reached() takes for persistent_nuts = 0


def league_chain_runs():
    """(engine, case, chains, options) of the several-chain league runs."""
    c = SC.CASES[MULTI_CASE]
    out = [(SC.chains_engine(c.T, c.D, n), MULTI_CASE, n, {}) for n in CHAIN_COUNTS]
    l = SC.CASES[LOCKSTEP_CASE]
    out.append((SC.chains_engine(l.T, l.D, 2, persistent_nuts=0), LOCKSTEP_CASE, 2, {"persistent_nuts": 0}))
    return out


def league_engines_covered():
    return {e for e, _, _ in league_single_runs()} | {e for e, _, _, _ in league_chain_runs()}


def chain_inputs(D, n):
    """Distinct keys and distinct starts for n chains of a D-vector."""
    z0 = np.random.RandomState(2).uniform(-0.2, 0.2, (n, D))
    return [(KEY[0], KEY[1] + c) for c in range(n)], z0


def league_oracle(case):
    """z -> (U, rho) of the float64 oracle on the case's league (weights as the device holds them: float64 values
    of float32 storage, sampler_cases.fixtures)."""
    fx = SC.fixtures(case)

    def at(z):
        U, _, aux = O.potential_and_grad(case.model, fx, z)
        return U, aux["rho"]
    return at, fx.n


# ------------------------------------------------------------------------------------------- neutral and dynamic
def neutral_fixture(name):
    fx = {"plain": lambda: NO.synthetic_neutral(600, 8), "wc": lambda: NO.synthetic_neutral(600, 8, k=2, n_conf=3)}[name]()
    fx.weights = fx.weights.astype(np.float32).astype(np.float64)   # what the device holds
    return fx


def dynamic_fixture(name):
    return {"small": lambda: DO.small_recipe(), "small_cov": lambda: DO.small_recipe(k=3)}[name]()


# run_chains_persistent (bplhip.hip): a context outside dc_eval's tail takes the fused neutral leaf when the model is
# the neutral one, fused_small is on and D <= 64 LEAF_NE_MAX (and its LDS fits); else kp_leaf up to that D and
# kw_leaf beyond; device_nuts = 0 is the host tree for every model.
# (family, fixture, random_walk, options, engine, chains)
VENUE_RUNS = [
    ("neutral", "plain", None, {}, "PERSIST_NEU_FUSED", 1),
    ("neutral", "wc", None, {}, "PERSIST_NEU_FUSED", 1),
    ("neutral", "wc", None, {}, "PERSIST_NEU_FUSED", 3),
    ("neutral", "plain", None, {"fused_small": 0}, "PERSIST_KP_LEAF", 1),
    ("neutral", "wc", None, {"fused_small": 0}, "PERSIST_KP_LEAF", 2),
    ("neutral", "wc", None, {"device_nuts": 0}, "HOST_TREE", 1),
    ("dynamic", "small", True, {}, "PERSIST_KW_LEAF", 1),
    ("dynamic", "small", False, {}, "PERSIST_KW_LEAF", 1),
    ("dynamic", "small_cov", True, {}, "PERSIST_KW_LEAF", 2),
    ("dynamic", "small_cov", False, {}, "PERSIST_KW_LEAF", 1),
    ("dynamic", "small_cov", True, {"device_nuts": 0}, "HOST_TREE", 1),
]
VENUE_ENGINES = {"PERSIST_NEU_FUSED", "PERSIST_KP_LEAF", "PERSIST_KW_LEAF", "HOST_TREE"}
VENUE_STEP = {"neutral": 0.02, "dynamic": 0.01}   # the fixed steps tests/test_gpu_dynamic.py runs such leagues with


def venue_dim(family, fx):
    if family == "neutral":
        return NO.latent_dim(fx.n_teams, fx.k, fx.n_conf)
    return DO.latent_dim(fx.n_gameweeks, fx.n_teams, fx.k)


def venue_oracle(family, fx, random_walk):
    def at(z):
        U, _, aux = NO.potential_and_grad(fx, z) if family == "neutral" else DO.potential_and_grad(fx, z, random_walk)
        return float(U), float(aux["rho"])
    return at, fx.n


# ---------------------------------------------------------------------------------------------- shared assertions
def oracle_columns(at, draws):
    cols = np.array([at(z) for z in draws])
    return cols[:, 0], cols[:, 1]


def sensitivity(family, n_fixtures, U, rho):
    """The fraction of consecutive kept pairs whose oracle values differ by more than SENSITIVITY gates, for U and
    for rho: below MIN_FRACTION a column shifted by one row could pass the comparison."""
    gate = np.array([u_gate(family, n_fixtures, u) for u in U])
    du = np.abs(np.diff(U)) > SENSITIVITY * np.maximum(gate[:-1], gate[1:])
    dr = np.abs(np.diff(rho)) > SENSITIVITY * RHO_GATE[family]
    return float(du.mean()), float(dr.mean())


# ------------------------------------------------------------------------------------------ divergent transitions
# The basic model on the reference's dummy league, fixed step, identity mass matrix, max_tree_depth 5, key KEY.
# DIVERGENT_STEPS are the candidates; the rule was: keep the first for which the restatement (oracle/nuts_oracle.py
# on the float64 C potential) gives, within 8 transitions, at least two divergent and at least two non-divergent
# ones.  NO candidate meets it: this posterior is stiff enough that at every one of them each transition diverges at
# its FIRST leaf (energy error > max_delta_energy = 1000 after one leapfrog), from the uniform start of the other runs
# and from a point of the typical set alike; the chain never moves.  The change from "never" to "always" happens
# between steps 0.03125 (no divergence in 12 transitions, trees of 31 leapfrogs) and 0.0625, and a step tuned into
# that window would give runs whose flags depend on the last bits of the potential.  What is run instead:
#   DIVERGENT_FIRST_LEAF  the first candidate, 0.5: every transition diverges at its first leaf; the draw must equal
#                         its predecessor and the statistics must be those of that (unchanged) point -- the "stale
#                         aux" case;
#   DIVERGENT_LATER       the candidates halved on, 0.0625 from DIVERGENT_START: every transition diverges, but after
#                         2 to 6 leapfrogs, and two of the first 8 (four of 12) accept a proposal from the leaves
#                         before the divergence, so the statistics must be those of an inner leaf of a truncated tree.
# The non-divergent kind is every transition of the FIXED runs.  tests/test_draw_stats_cases_host.py re-derives the
# flags below with the restatement.
DIVERGENT_STEPS = (0.5, 1.0, 2.0, 4.0)
DIVERGENT_TRANSITIONS = 8
DIVERGENT_FLAGS = {s: [1] * 8 for s in DIVERGENT_STEPS}            # restatement: diverging, per transition
DIVERGENT_TREE_SIZES = {s: [1] * 8 for s in DIVERGENT_STEPS}       # restatement: num_steps
DIVERGENT_FIRST_LEAF = 0.5
DIVERGENT_LATER = 0.0625
DIVERGENT_LATER_FLAGS = [1, 1, 1, 1, 1, 1, 1, 1]
DIVERGENT_LATER_TREE_SIZES = [4, 4, 3, 3, 2, 3, 3, 3]
DIVERGENT_LATER_MOVED = [0, 1, 0, 0, 0, 0, 0, 1]
# a draw of an adapted float64 chain on this league, rounded to two decimals
DIVERGENT_START = np.array([
    1.39, -1.39, 0.72, 1.18, -0.28, 2.22, 1.06, -1.23, -0.62, -0.76, -0.17, 0.56, 0.88, -0.69, -0.62, 0.6, -0.19, -0.96,
    -1.74, 0.11, 1.46, -0.74, -0.67, -0.55, -0.42, 2.12, 0.38, 0.41, 0.32, 0.11, -1.83, -3.16, 0.36, 1.17, -0.45, 1.03,
    0.69, 1.05, 0.57, -0.61, -0.37, 0.24, -0.49, -2.71, -2.77])
# every engine that binds the basic dummy league (T = 20, D = 45: dc_eval's tail): (engine, options, chains)
DIVERGENT_ENGINES = [
    (SC.engines_for(20, 45)[s], SC.OPTIONS[s], 1) for s in SC.SETTINGS
] + [(SC.chains_engine(20, 45, 2), {}, 2), (SC.chains_engine(20, 45, 9), {}, 9),
     (SC.chains_engine(20, 45, 2, persistent_nuts=0), {"persistent_nuts": 0}, 2)]
