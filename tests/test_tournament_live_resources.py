"""The live-tournament kernels (csrc/dc_tournament_live.hip.h): the eight simulators and the one log-likelihood
kernel exist under their own namespace, without scratch, within 128 VGPRs and 64 KB of LDS; a simulator's static LDS
is no more than its kick-off twin's (the states and the search live in registers), the
log-likelihood kernel keeps none, and the weights and the scan are still dc_live.hip.h's one kernel (no GPU needed:
read from the code object's metadata in the built library, as tests/test_allocation_resources.py does)."""
import pytest

import code_object

# a live simulator and its kick-off twin, by what their mangled names hold before the template argument
TWINS = {"8live_cupI": "13dc_tournamentI", "11live_cup_etI": "16dc_tournament_etI",
         "14live_cup_tableI": "9cup_allocI", "17live_cup_table_etI": "12cup_alloc_etI"}
FORMS = ("Lb0EEE", "Lb1EEE")   # the overall and the head-to-head order


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object.read_kernels(tmp_path_factory)


def _mine(kernels):
    return {k: v for k, v in kernels.items() if k.startswith("_ZN4dctl")}


def test_eight_simulators_and_one_loglik_kernel_within_the_bounds(kernels):
    mine = _mine(kernels)
    sims = {k: v for k, v in mine.items() if "live_cupI" in k or "live_cup_etI" in k or "live_cup_tableI" in k
            or "live_cup_table_etI" in k}
    loglik = {k: v for k, v in mine.items() if "live_cup_loglik" in k}
    assert len(sims) == 8 and len(loglik) == 1 and len(mine) == 9, sorted(mine)
    for live in TWINS:
        for form in FORMS:
            assert sum(live + form in k for k in sims) == 1, (live, form, sorted(sims))
    for name, k in mine.items():
        assert k["scratch"] == 0, (name, k)
        assert k["vgpr"] <= 128, (name, k)
        assert k["lds"] <= 64 * 1024, (name, k)
    assert next(iter(loglik.values()))["lds"] == 0


def test_a_simulator_keeps_no_more_static_lds_than_its_kick_off_twin(kernels):
    for live, twin in TWINS.items():
        for form in FORMS:
            mine = [v for k, v in _mine(kernels).items() if live + form in k]
            theirs = [v for k, v in kernels.items() if k.startswith("_ZN3dct") and twin + form in k]
            assert len(mine) == 1 and len(theirs) == 1, (live, twin, form)
            assert mine[0]["lds"] <= theirs[0]["lds"], (live, form, mine[0], theirs[0])


def test_the_weights_and_the_scan_are_still_one_kernel(kernels):
    assert sum("live_weights" in k for k in kernels) == 1
    # and no new kernel carries a name the existing resource tests count by
    taken = ("dc_tournament", "cup_alloc", "dc_paths_sim", "paths_alloc_sim", "dc_tscen_sim", "tscen", "scen_alloc_sim",
             "dc_gpts", "points_alloc_sim", "6dclive", "4dclq", "dc_season", "dc_leverage", "dc_points_count",
             "dc_scenario", "4dctr", "3dcg", "3dcu", "4dcps")
    for name in _mine(kernels):
        for word in taken:
            assert word not in name, (name, word)
