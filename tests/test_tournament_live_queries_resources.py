"""The live tournament-query kernels (csrc/dc_tournament_live_queries.hip.h): 24 recording kernels under their own
namespace, one per (query, tie-break order, knockout rule, ranked / table), without scratch, within 128 VGPRs, with no
more static LDS than their kick-off twins (the states, the sides and the scores live in
registers); and the two weight kernels they share with simulate_tournament are still one each (no GPU needed: read
from the code object's metadata in the built library, as tests/test_tournament_live_resources.py does)."""
import pytest

import code_object

# a live kernel and its kick-off twin: (namespace, name) as their mangled names hold them before the template arguments
TWINS = {"14cup_paths_liveI": ("6dcpath", "12dc_paths_simI"), "20cup_paths_live_tableI": ("6dcpath", "15paths_alloc_simI"),
         "13cup_scen_liveI": ("4dcts", "12dc_tscen_simI"), "19cup_scen_live_tableI": ("4dcts", "14scen_alloc_simI"),
         "16cup_gpoints_liveI": ("4dcgq", "11dc_gpts_simI"), "22cup_gpoints_live_tableI": ("4dcgq", "16points_alloc_simI")}
FORMS = tuple(f"Lb{h}ELb{e}EEE" for h in (0, 1) for e in (0, 1))   # <H2H, ET>


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object.read_kernels(tmp_path_factory)


def _mine(kernels):
    return {k: v for k, v in kernels.items() if k.startswith("_ZN4dctq")}


def test_twenty_four_kernels_one_per_form_within_the_bounds(kernels):
    mine = _mine(kernels)
    assert len(mine) == 24, sorted(mine)
    for live in TWINS:
        for form in FORMS:
            assert sum(k.startswith("_ZN4dctq" + live + form) for k in mine) == 1, (live, form, sorted(mine))
    for name, k in mine.items():
        assert k["scratch"] == 0, (name, k)
        assert k["vgpr"] <= 128, (name, k)
        assert k["lds"] <= 64 * 1024, (name, k)


def test_a_live_kernel_keeps_no_more_static_lds_than_its_kick_off_twin(kernels):
    for live, (space, twin) in TWINS.items():
        for form in FORMS:
            mine = [v for k, v in _mine(kernels).items() if k.startswith("_ZN4dctq" + live + form)]
            theirs = [v for k, v in kernels.items() if k.startswith("_ZN" + space + twin + form)]
            assert len(mine) == 1 and len(theirs) == 1, (live, twin, form)
            assert mine[0]["lds"] <= theirs[0]["lds"], (live, form, mine[0], theirs[0])


def test_the_weight_kernels_are_still_one_each_and_the_names_stay_clear(kernels):
    assert sum("live_weights" in k for k in kernels) == 1
    assert sum("live_cup_loglik" in k for k in kernels) == 1
    # no new kernel carries a name the existing resource tests count by
    taken = ("dc_tournament", "cup_alloc", "dc_paths_sim", "paths_alloc_sim", "dc_tscen_sim", "tscen", "scen_alloc_sim",
             "dc_gpts", "points_alloc_sim", "live_leverage_sim", "live_points_sim", "live_scenario_sim", "live_cup",
             "live_weights", "6dclive", "4dclq", "4dctl", "dc_season", "dc_leverage", "dc_points", "dc_scenario", "dc_paths_",
             "dc_playoff", "dc_ppc", "4dctr", "3dcg", "3dcu", "4dcps")
    for name in _mine(kernels):
        for word in taken:
            assert word not in name, (name, word)
