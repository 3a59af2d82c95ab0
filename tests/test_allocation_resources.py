"""The best-of-rest allocation has kernels of its own, the existing kernels' text with ALLOC set
(csrc/dc_tournament.hip.h: cup_alloc, cup_alloc_et; csrc/dc_paths.hip.h: paths_alloc_sim; csrc/dc_tscen.hip.h:
scen_alloc_sim; csrc/dc_group_points.hip.h: points_alloc_sim), so the built library still holds exactly four kernels
of each of the four tournament simulators under their own names, as the existing resource tests count them, and the
sixteen new ones stay within the same gates -- no scratch, at most 64 KB of LDS, at most 128 VGPRs (no GPU needed:
read from the code object's metadata, as tests/test_paths_resources.py does)."""
import pytest

import code_object

# what the kernels of one simulator have in common in their mangled names, and those of its allocation kernels
FAMILIES = {"dc_tournament": "cup_alloc", "dc_paths_sim": "paths_alloc_sim", "dc_tscen_sim": "scen_alloc_sim",
            "dc_gpts_sim": "points_alloc_sim"}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object.read_kernels(tmp_path_factory)


def _within(found):
    for name, k in found.items():
        assert k["scratch"] == 0, (name, k)
        assert k["lds"] <= 64 * 1024, (name, k)
        assert k["vgpr"] <= 128, (name, k)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_four_kernels_of_each_simulator_within_the_bounds(kernels, family):
    found = {k: v for k, v in kernels.items() if family in k}
    assert len(found) == 4, (family, sorted(found))
    _within(found)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_four_allocation_kernels_of_each_simulator_within_the_bounds(kernels, family):
    found = {k: v for k, v in kernels.items() if FAMILIES[family] in k}
    assert len(found) == 4, (family, sorted(found))
    assert not [k for k in found if family in k], sorted(found)     # (the existing tests count by those names)
    _within(found)
    # the allocation's LDS is theirs alone: a word per wave, and the slot histogram in simulate_tournament's
    plain = sorted(v["lds"] for k, v in kernels.items() if family in k)
    extra = 16 + (16 * 16 * 4 if family == "dc_tournament" else 0)
    assert sorted(v["lds"] for v in found.values()) == [x + extra for x in plain]
