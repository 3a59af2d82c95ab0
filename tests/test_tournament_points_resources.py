"""The tournament_points kernels (csrc/dc_group_points.hip.h) are in the built library and stay within the tournament
kernels' gates: no scratch, at most 64 KB of LDS and 128 VGPRs; their names stay clear of the substrings by which the
other resource tests find their kernels; and the existing recording and counting kernels are as many as before (no GPU
needed: read from the code object's metadata in the built library, as tests/test_paths_resources.py does)."""
import pytest

import code_object

# the substrings the existing resource tests search the mangled names for
TAKEN = ("dc_scenario", "dc_paths_", "dc_tournament", "dc_season", "dc_leverage", "dc_points", "dc_playoff", "dc_ppc",
         "tscen", "dcl", "dcs", "3dcg", "3dcu", "3dcr", "3dcm", "4dctr", "4dcps", "4dcip", "4dcsl", "5dcloo", "6dclive",
         "dcppc", "outcome_", "market_", "ratings_", "inplay_")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object.read_kernels(tmp_path_factory)


def _gates(name, k):
    assert k["scratch"] == 0, (name, k)
    assert k["lds"] <= 64 * 1024, (name, k)
    assert k["vgpr"] <= 128, (name, k)


def test_tournament_points_kernel_resources(kernels):
    sims = {k: v for k, v in kernels.items() if "dc_gpts_sim" in k}
    # head-to-head x extra time: four recording kernels
    assert len(sims) == 4, sorted(kernels)
    assert {("ILb%dELb%dE" % (h, e)) in "".join(sims) for h in (0, 1) for e in (0, 1)} == {True}
    for name, k in sims.items():
        _gates(name, k)
    counts = {k: v for k, v in kernels.items() if "dc_gpts_count" in k}
    assert len(counts) == 1, sorted(kernels)
    for name, k in counts.items():
        _gates(name, k)
        assert k["lds"] >= 256 * 17 * 4      # the largest row: 256 bins x (1 + 8 targets + 8 places) words


def test_names_stay_clear_of_the_other_kernels(kernels):
    ours = [k for k in kernels if "dc_gpts" in k]
    assert len(ours) == 5, ours
    for name in ours:
        assert "4dcgq" in name
        for taken in TAKEN:
            assert taken not in name, (name, taken)


def test_the_existing_kernels_are_as_many_as_before(kernels):
    assert len([k for k in kernels if "dc_tscen_sim" in k]) == 4
    assert len([k for k in kernels if "dc_paths_sim" in k]) == 4
    assert len([k for k in kernels if "dc_scenario_count" in k]) == 1
    assert len([k for k in kernels if "dc_leverage_count" in k]) == 1
    assert len([k for k in kernels if "dc_paths_count" in k]) == 1
    assert len([k for k in kernels if "dc_points_count" in k]) == 1
