"""The built library holds the two play-off kernels (csrc/dc_playoff.hip.h: `dc_playoff<false>` for the overall
order, `dc_playoff<true>` for the head-to-head order), and each keeps the bounds of the simulation kernels: no
scratch, at most 64 KB of static LDS -- and little enough that four workgroups fit a CU's 160 KB, as for dc_season
-- and at most 128 VGPRs (no GPU needed: read from the code object's metadata, as tests/test_season_resources.py
does)."""
import pytest

import code_object

# Itanium mangling: <length><name>I<template argument>E
INSTANTIATIONS = {"10dc_playoffILb0EE": "overall order", "10dc_playoffILb1EE": "head-to-head order"}
CU_LDS_BYTES = 160 * 1024
WORKGROUPS_PER_CU = 4


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object.read_kernels(tmp_path_factory)


def test_two_playoff_instantiations_within_the_bounds(kernels):
    playoff = {k: v for k, v in kernels.items() if "dc_playoff" in k}
    assert len(playoff) == 2, sorted(playoff)
    for args, what in INSTANTIATIONS.items():
        found = [k for k in playoff if args in k]
        assert len(found) == 1, (what, sorted(playoff))
        k = playoff[found[0]]
        print(what, k)
        assert k["scratch"] == 0, (what, k)
        assert k["lds"] <= 64 * 1024, (what, k)
        assert WORKGROUPS_PER_CU * k["lds"] <= CU_LDS_BYTES, (what, k)
        assert k["vgpr"] <= 128, (what, k)


def test_the_names_stay_clear_of_the_other_kernels_tests(kernels):
    """The other resource tests find their kernels by substring: the play-off kernels match none of them."""
    for name in kernels:
        if "dc_playoff" in name:
            for other in ("dc_tournament", "dc_season", "dc_leverage", "dc_ppc"):
                assert other not in name, (name, other)
