"""CPU: every case of tests/sampler_cases.py still sits on the edge it was built for -- the D arithmetic, the side of
every boundary of the host's dispatch (constants read out of the sources), a start point the float64 oracle can
evaluate -- and its golden is the recipe's (oracle/make_nuts_golden.py)."""
import os
import re

import numpy as np
import pytest

import dc_oracle as O
import dc_oracle_c as OC
import sampler_cases as SC

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
C = SC.CASES


def test_constants_come_from_the_sources():
    # (their order only: the values are the sources' business; a case that leaves its edge fails below)
    assert SC.LOOP_LNE1_MAX_D == SC.WAVE == SC.TAIL_LANES == SC.TAIL_MAX_T
    assert SC.LOOP_LNE1_MAX_D < SC.LOOP_MAX_D <= 2 * SC.WAVE < SC.TAIL_MAX_D == SC.LEAF_NE_MAX * SC.WAVE
    assert SC.TAIL_MAX_D < SC.KW_NTB and SC.KW_MAX_WG >= 2
    assert 8 < SC.XS_STAGED_MAX_K < SC.LOOP_COEF_MAX_K and 2 <= SC.GRIDY_MAX_CHAINS


def test_engine_constants_match_the_header():
    from bpl import _ffi

    header = open(os.path.join(os.path.dirname(GOLD), os.pardir, "include", "bplhip.h")).read()
    declared = {k: int(v) for k, v in re.findall(r"BPLHIP_ENGINE_([A-Z0-9_]+) = (\d+)", header)}
    assert declared == {nm: getattr(_ffi, "ENGINE_" + nm) for nm in _ffi.ENGINE_NAMES}
    assert [getattr(_ffi, "ENGINE_" + nm) for nm in _ffi.ENGINE_NAMES] == list(range(len(_ffi.ENGINE_NAMES)))
    assert SC.LEAGUE_ENGINES == set(_ffi.ENGINE_NAMES) - {"NONE", "PERSIST_NEU_FUSED"}   # (the neutral model's own)


def test_the_cases_reach_every_engine():
    assert SC.engines_reached() == SC.LEAGUE_ENGINES
    assert len(SC.ALL) == 18 and len(C) == 18


@pytest.mark.parametrize("name", list(C))
def test_case_arithmetic_and_engines(name):
    c = C[name]
    fx = SC.fixtures(c)
    assert O.latent_dim(c.model, c.T, c.K) == c.D
    assert fx.n_teams == c.T and (fx.k if c.model == O.MODEL_EXTENDED else 0) == c.K and fx.n == c.n
    assert (fx.weights is not None) == c.weighted and (c.model == O.MODEL_EXTENDED or not (c.weighted and c.K))
    assert (fx.home_idx != fx.away_idx).all() and set(fx.home_idx) | set(fx.away_idx) == set(range(c.T))
    if c.weighted:      # float32 storage: what the device is handed is what the oracle sees
        assert np.array_equal(fx.weights, fx.weights.astype(np.float32).astype(np.float64)) and fx.weights.min() > 0
    # the engines DESIGN.md section 40's table states are the ones the restated dispatch gives
    assert dict(zip(SC.SETTINGS, c.engines)) == SC.engines_for(c.T, c.D)


def test_each_case_is_on_its_side_of_its_boundaries():
    W, NE = SC.WAVE, SC.LEAF_NE_MAX
    slots = lambda n: -(-C[n].D // W)                 # elements per lane of the staged / register leaf
    last = lambda n: C[n].D - (slots(n) - 1) * W      # ... and how many lanes hold one in the last slot
    # launch_loop_t: one element per lane up to 64
    assert C["b63"].D == SC.LOOP_LNE1_MAX_D - 1 and C["e64w"].D == SC.LOOP_LNE1_MAX_D
    assert C["b65"].D == C["b65w"].D == SC.LOOP_LNE1_MAX_D + 1 and last("b65") == 1
    assert (slots("b63"), last("b63")) == (1, W - 1) and (slots("e64w"), last("e64w")) == (1, W)
    # loop_ok: two up to 128
    assert C["e127"].D == C["e127k33"].D == SC.LOOP_MAX_D - 1 and C["e128w"].D == C["e128k32"].D == SC.LOOP_MAX_D
    assert C["e129"].D == SC.LOOP_MAX_D + 1 and (slots("e129"), last("e129")) == (3, 1)
    assert (slots("e127"), last("e127")) == (2, W - 1) and (slots("e128w"), last("e128w")) == (2, W)
    assert SC.LOOP_LNE1_MAX_D < C["e77w"].D < SC.LOOP_MAX_D and SC.LOOP_LNE1_MAX_D < C["e101"].D < SC.LOOP_MAX_D
    # leaf_in_tail: T <= 64 and D <= 64 LEAF_NE_MAX
    assert (slots("e193"), last("e193")) == (NE, 1) and (slots("e256"), last("e256")) == (NE, W)
    assert C["e256"].D == SC.TAIL_MAX_D and C["e256"].T == SC.TAIL_MAX_T - 1
    assert C["e257"].D == SC.TAIL_MAX_D + 1 and C["e257"].T == SC.TAIL_MAX_T      # the latent size alone decides
    for n in ("b255", "e256g", "b257", "b1025"):
        assert C[n].T > SC.TAIL_MAX_T                                              # the team count does
    # kp_leaf (one wave, LeafState<LEAF_NE_MAX>) up to 256, kw_leaf beyond
    assert C["b255"].D == SC.TAIL_MAX_D - 1 and C["e256g"].D == SC.TAIL_MAX_D and C["b257"].D == SC.TAIL_MAX_D + 1
    assert SC.kw_workgroups(C["e257"].D) == SC.kw_workgroups(C["b257"].D) == 1
    assert C["b1025"].D == SC.KW_NTB + 1 and SC.kw_workgroups(C["b1025"].D) == 2 and SC.kw_workgroups(SC.KW_NTB) == 1
    # covariate counts: xs_staged, LOOP_COEF_MAX_K, the K <= 8 one-pass sums (either side, inside the loop kernel)
    assert C["e101"].K == SC.XS_STAGED_MAX_K + 1 and C["e77w"].K <= 8 < C["e101"].K
    assert C["e128k32"].K == SC.LOOP_COEF_MAX_K and C["e127k33"].K == SC.LOOP_COEF_MAX_K + 1
    assert 0 < C["e128w"].K <= 8 and C["e129"].K == 1 and C["e127"].K == 0
    # dc_eval_loop<W, C, LNE>: the instantiations these cases run in.  (The library's basic model takes no weights --
    # bplhip_set_fixtures refuses them -- so <true, false, *> cannot be reached and b65w runs only in the oracle;
    # <false, true, 1> is the unweighted extended fit of tests/test_gpu_fit.py::test_time_weighted_vs_not.)
    seen = {(c.weighted, c.model == O.MODEL_EXTENDED, c.engine("persistent")) for c in SC.ALL
            if c.engine("persistent").startswith("LOOP_") and c.bindable}
    assert seen == {(False, False, "LOOP_LNE1"), (False, False, "LOOP_LNE2"), (False, True, "LOOP_LNE2"),
                    (True, True, "LOOP_LNE1"), (True, True, "LOOP_LNE2")}
    assert [c.name for c in SC.ALL if not c.bindable] == ["b65w"]
    # chain counts either side of gridy_max_chains
    assert max(k for k in SC.MULTI_CHAINS if k <= SC.GRIDY_MAX_CHAINS) == SC.GRIDY_MAX_CHAINS
    assert min(k for k in SC.MULTI_CHAINS if k > SC.GRIDY_MAX_CHAINS) == SC.GRIDY_MAX_CHAINS + 1
    for n in SC.MULTI:
        assert C[n].tail
    for n in SC.BITWISE + SC.SPEC:
        assert C[n].engine("persistent").startswith("LOOP_") and C[n].engine("kernel0") == "PERSIST_TAIL"


@pytest.mark.parametrize("name", list(C))
def test_oracle_at_the_start_point(name):
    c = C[name]
    cf = OC.CFixtures(c.model, SC.fixtures(c))
    z0 = SC.start(c)
    U, g, aux = OC.potential_and_grad(cf, z0, 1)
    rho, LB, UB, _ = aux
    assert cf.D == c.D and np.isfinite(U) and np.isfinite(g).all()
    assert LB < rho < UB
    gold = np.load(os.path.join(GOLD, f"nuts_edge_{name}.npz"))
    assert np.array_equal(gold["z0"], z0) and gold["draws"].shape == (SC.TRANSITIONS, c.D)
    assert float(gold["step_size0"]) == SC.STEP and tuple(gold["key"]) == SC.KEY and int(gold["num_warmup"]) == 0
    moved = not np.array_equal(gold["draws"][2], z0)
    assert moved == (name not in SC.FINE)
    if name in SC.FINE:
        fine = np.load(os.path.join(GOLD, f"nuts_edge_{name}_fine.npz"))
        assert float(fine["step_size0"]) == SC.FINE_STEP and not fine["diverging"].any()
        assert (fine["accept_prob"][:3] > 1e-2).all() and fine["num_steps"].sum() > 500
    if name in SC.ADAPTED:
        ad = np.load(os.path.join(GOLD, f"nuts_edge_{name}_adapt_shallow.npz"))
        assert (int(ad["num_warmup"]), int(ad["num_samples"]), int(ad["max_tree_depth"])) == (22, 6, 2)
