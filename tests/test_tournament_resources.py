"""The tournament kernel (csrc/dc_tournament.hip.h) keeps everything in registers and LDS: no scratch,
at most 64 KB of LDS and 128 VGPRs, so that four 256-thread workgroups fit on a CU (no GPU needed:
read from the code object's metadata in the built library, as tests/test_season_resources.py does)."""
import pytest

import code_object


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object.read_kernels(tmp_path_factory)


def test_tournament_kernel_resources(kernels):
    tournament = {k: v for k, v in kernels.items() if "dc_tournament" in k}
    assert tournament, "the tournament kernel is not in the library"
    for name, k in tournament.items():
        assert k["scratch"] == 0, (name, k)
        assert k["lds"] <= 64 * 1024, (name, k)
        assert k["vgpr"] <= 128, (name, k)
