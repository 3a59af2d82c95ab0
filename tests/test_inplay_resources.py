"""The in-play kernels (csrc/dc_inplay.hip.h): both exist in both rate forms, without scratch, within the register
and LDS budget of DESIGN.md section 25 (no GPU needed: read from the code object's metadata in the built library,
as tests/test_markets_resources.py does)."""
import pytest

import code_object

MAX_DRAWS = 12288            # include/bplhip.h BPLHIP_INPLAY_MAX_DRAWS
LDS_BUDGET = 160 * 1024      # a gfx950 workgroup's LDS


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object.read_kernels(tmp_path_factory)


def _mine(kernels):
    return {k: v for k, v in kernels.items() if "4dcip" in k and "inplay_" in k}


def test_inplay_kernels_exist_without_scratch(kernels):
    mine = _mine(kernels)
    names = " ".join(mine)
    for kind in ("inplay_valuesILb0", "inplay_valuesILb1", "inplay_summaryILb0", "inplay_summaryILb1"):
        assert kind in names, f"{kind} is not in the library"
    assert len(mine) == 4, names
    for name, k in mine.items():
        assert k["scratch"] == 0, (name, k)


def test_inplay_values_uses_no_lds_and_keeps_four_waves(kernels):
    # registers only, as market_values; at most 128 VGPRs keep 4 waves per SIMD (the section 16 argument)
    for name, k in _mine(kernels).items():
        if "inplay_values" in name:
            assert k["lds"] == 0, (name, k)
            assert k["vgpr"] <= 128, (name, k)


def test_inplay_summary_fits_the_lds_with_the_most_draws(kernels):
    # static LDS (histograms, segment totals) plus the dynamic 12 bytes per draw (keys, two index buffers)
    for name, k in _mine(kernels).items():
        if "inplay_summary" in name:
            assert k["lds"] + 12 * MAX_DRAWS <= LDS_BUDGET, (name, k)
            assert k["vgpr"] <= 128, (name, k)
