"""tests/draw_stats_cases.py on the CPU: every engine of sampler_cases.engines_reached() has a run, the thinning rule
is nuts.hpp's, and the divergence flags recorded there are what the float64 restatement (oracle/nuts_oracle.py on the C
potential) gives; the sensitivity condition of the league runs holds on the float64 CPU chain (the GPU tests assert it
on the device's own draws)."""
import re

import numpy as np
import pytest

import cases
import dc_oracle as O
import dc_oracle_c as OC
import draw_stats_cases as DS
import nuts_oracle as NU
import sampler_cases as SC
from eval_path_cases import _read


def test_every_engine_has_a_run():
    assert DS.league_engines_covered() == SC.engines_reached() == SC.LEAGUE_ENGINES
    for engine, name, setting in DS.league_single_runs():
        case = SC.CASES[name]
        assert case.bindable and case.engine(setting) == engine and name not in SC.FINE
        smaller = [c for c in SC.ALL if c.bindable and c.name not in SC.FINE and engine in c.engines and c.D < case.D]
        assert not smaller, (engine, name, [c.name for c in smaller])
    assert {n for _, _, n, _ in DS.league_chain_runs()} == set(DS.CHAIN_COUNTS) and max(DS.CHAIN_COUNTS) <= 9
    assert {r[4] for r in DS.VENUE_RUNS} == DS.VENUE_ENGINES
    assert {(r[0], r[1], r[2]) for r in DS.VENUE_RUNS} >= {
        ("neutral", "plain", None), ("neutral", "wc", None), ("dynamic", "small", True), ("dynamic", "small", False),
        ("dynamic", "small_cov", True), ("dynamic", "small_cov", False)}
    names = set(re.findall(r"BPLHIP_ENGINE_(\w+)\s*=", _read("../../include/bplhip.h")))
    assert names - {"NONE"} == SC.LEAGUE_ENGINES | DS.VENUE_ENGINES   # no engine value is left without a run


def test_venue_engines_follow_the_dispatch_rule():
    """run_chains_persistent: generic (a neutral or dynamic context never sits in dc_eval's tail); the fused neutral
    leaf for the neutral model with fused_small up to 64 LEAF_NE_MAX latent entries, kp_leaf up to that size, kw_leaf
    beyond; device_nuts = 0 is the host tree."""
    for family, fixture, rw, opts, engine, nch in DS.VENUE_RUNS:
        fx = DS.neutral_fixture(fixture) if family == "neutral" else DS.dynamic_fixture(fixture)
        D = DS.venue_dim(family, fx)
        if opts.get("device_nuts", 1) == 0:
            want = "HOST_TREE"
        elif D > SC.TAIL_MAX_D:
            want = "PERSIST_KW_LEAF"
        elif family == "neutral" and opts.get("fused_small", 1):
            want = "PERSIST_NEU_FUSED"
        else:
            want = "PERSIST_KP_LEAF"
        assert engine == want and (nch == 1 or engine != "HOST_TREE"), (family, fixture, opts)
        assert 1 <= nch <= 9 and fx.n <= 4000


def test_thinning_rule_is_the_drivers():
    src = _read("nuts.hpp")
    assert "start_idx = cfg.num_warmup + cfg.num_samples % cfg.thinning;" in src
    assert "if (it >= start_idx && (it - start_idx) % cfg.thinning == cfg.thinning - 1) {" in src
    assert "const int idx = (it - start_idx) / cfg.thinning;" in src
    for samples, thin in ((14, 3), (21, 2), (12, 1), (7, 7), (9, 4)):
        start = samples % thin
        want = [it for it in range(samples) if it >= start and (it - start) % thin == thin - 1]
        assert DS.kept_rows(samples, thin) == want and len(want) == samples // thin
    assert DS.kept_rows(14, 3) == [4, 7, 10, 13] and DS.kept_rows(21, 2) == list(range(2, 21, 2))


@pytest.fixture(scope="module")
def dummy_pot():
    cf = OC.CFixtures(O.MODEL_BASIC, cases.fixtures("dummy"))

    def pot(z):
        U, g, _ = OC.potential_and_grad(cf, z)
        return U, g
    return pot


def _restated(pot, z0, step):
    with np.errstate(all="ignore"):
        o = NU.run_chain(pot, DS.KEY, 0, DS.DIVERGENT_TRANSITIONS, z0=z0, step_size=step, max_depth=5)
    moved = (o["draws"] != np.vstack([z0[None], o["draws"][:-1]])).any(axis=1)
    return o["diverging"].astype(int).tolist(), o["num_steps"].tolist(), moved.astype(int).tolist()


def test_no_candidate_step_gives_both_kinds(dummy_pot):
    """The recorded flags: at every candidate each of the 8 transitions diverges at its first leaf, from the other
    runs' uniform start and from the typical point alike -- so the selection rule (two of each kind) keeps none."""
    for z0 in (DS.chain_inputs(45, 1)[1][0], DS.DIVERGENT_START):
        for step in DS.DIVERGENT_STEPS:
            div, sizes, moved = _restated(dummy_pot, z0, step)
            assert div == DS.DIVERGENT_FLAGS[step] and sizes == DS.DIVERGENT_TREE_SIZES[step] and not any(moved)
            assert not (sum(div) >= 2 and len(div) - sum(div) >= 2)
    assert DS.DIVERGENT_FIRST_LEAF == DS.DIVERGENT_STEPS[0]


def test_later_divergences_are_as_recorded(dummy_pot):
    div, sizes, moved = _restated(dummy_pot, DS.DIVERGENT_START, DS.DIVERGENT_LATER)
    assert (div, sizes, moved) == (DS.DIVERGENT_LATER_FLAGS, DS.DIVERGENT_LATER_TREE_SIZES, DS.DIVERGENT_LATER_MOVED)
    assert min(sizes) >= 2 and sum(moved) >= 2 and DS.DIVERGENT_LATER == DS.DIVERGENT_STEPS[0] / 8
    # and half that step no longer diverges at all: the window between the two kinds is narrower than a halving
    div, sizes, _ = _restated(dummy_pot, DS.DIVERGENT_START, DS.DIVERGENT_LATER / 2)
    assert not any(div) and sizes == [31] * 8


@pytest.mark.parametrize("engine,name,setting", DS.league_single_runs())
def test_league_runs_are_sensitive_on_the_float64_chain(engine, name, setting):
    case = SC.CASES[name]
    cf = OC.CFixtures(case.model, SC.fixtures(case))
    at, n = DS.league_oracle(case)
    for shape in (DS.league_fixed(case), DS.ADAPTED):
        rc, d, _, _ = OC.nuts_dc(cf, shape["num_warmup"], shape["num_samples"], DS.KEY, depth=shape["max_tree_depth"],
                                 thin=shape["thinning"], z0=SC.start(case), step_size=shape["step_size"] or 1.0)
        assert rc == 0 and d.shape[0] == shape["num_samples"] // shape["thinning"]
        fu, fr = DS.sensitivity("league", n, *DS.oracle_columns(at, d))
        assert fu >= DS.MIN_FRACTION and fr >= DS.MIN_FRACTION, (name, fu, fr)
