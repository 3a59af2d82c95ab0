"""The tournament_scenarios kernels (csrc/dc_tscen.hip.h) are in the built library and stay within the tournament
kernels' gates: no scratch, at most 64 KB of LDS and 128 VGPRs; their names stay clear of the substrings by which the
other resource tests find their kernels; and the counting kernels they reuse are still the only ones of their kind (no
GPU needed: read from the code object's metadata in the built library, as tests/test_paths_resources.py does)."""
import pytest

import code_object

# the substrings the existing resource tests search the mangled names for
TAKEN = ("dc_scenario", "dc_paths_", "dc_tournament", "dc_season", "dc_leverage", "dc_points", "dc_playoff", "dc_ppc")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object.read_kernels(tmp_path_factory)


def test_tournament_scenarios_kernel_resources(kernels):
    sims = {k: v for k, v in kernels.items() if "dc_tscen_sim" in k}
    # head-to-head x extra time: four recording kernels
    assert len(sims) == 4, sorted(kernels)
    assert {("ILb%dELb%dE" % (h, e)) in "".join(sims) for h in (0, 1) for e in (0, 1)} == {True}
    for name, k in sims.items():
        assert k["scratch"] == 0, (name, k)
        assert k["lds"] <= 64 * 1024, (name, k)
        assert k["vgpr"] <= 128, (name, k)


def test_names_stay_clear_of_the_other_kernels(kernels):
    ours = [k for k in kernels if "tscen" in k]
    assert len(ours) == 4, ours
    for name in ours:
        assert "dcts" in name
        for taken in TAKEN:
            assert taken not in name, (name, taken)


def test_the_counting_kernels_are_not_instantiated_again(kernels):
    assert len([k for k in kernels if "dc_scenario_count" in k]) == 1
    assert len([k for k in kernels if "dc_leverage_count" in k]) == 1
    # and the recording kernels of the two calls it stands between are as many as before
    assert len([k for k in kernels if "dc_scenario_sim" in k]) == 2
    assert len([k for k in kernels if "dc_paths_sim" in k]) == 4
