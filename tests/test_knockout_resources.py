"""The built library holds the four kernels of the one tournament body (csrc/dc_tournament_body.hip.inc)
-- overall / head-to-head order x redraw (`dc_tournament<*>`) / extra-time rule (`dc_tournament_et<*>`,
csrc/dc_knockout.hip.h) -- and each keeps the bounds of tests/test_tournament_resources.py: no scratch, at most
64 KB of LDS and 128 VGPRs (no GPU needed)."""
import pytest

import code_object

# Itanium mangling: <length><name>I<template argument>E
INSTANTIATIONS = {"13dc_tournamentILb0EE": "overall, redraw", "13dc_tournamentILb1EE": "head-to-head, redraw",
                  "16dc_tournament_etILb0EE": "overall, extra time", "16dc_tournament_etILb1EE": "head-to-head, extra time"}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object.read_kernels(tmp_path_factory)


def test_four_tournament_instantiations_within_the_bounds(kernels):
    tournament = {k: v for k, v in kernels.items() if "dc_tournament" in k}
    assert len(tournament) == 4, sorted(tournament)
    for args, what in INSTANTIATIONS.items():
        found = [k for k in tournament if args in k]
        assert len(found) == 1, (what, sorted(tournament))
        k = tournament[found[0]]
        assert k["scratch"] == 0, (what, k)
        assert k["lds"] <= 64 * 1024, (what, k)
        assert k["vgpr"] <= 128, (what, k)
