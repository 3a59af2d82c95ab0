"""The leverage kernels (csrc/dc_leverage.hip.h) keep everything in registers and LDS: no scratch
(no GPU needed: read from the code object's metadata in the built library, as
tests/test_season_resources.py does)."""
import pytest

import code_object


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object.read_kernels(tmp_path_factory)


def test_leverage_kernels_have_no_scratch(kernels):
    leverage = {k: v for k, v in kernels.items() if "dc_leverage" in k}
    assert any("dc_leverage_sim" in k for k in leverage), "the simulation stage is not in the library"
    assert any("dc_leverage_count" in k for k in leverage), "the counting stage is not in the library"
    for name, k in leverage.items():
        assert k["scratch"] == 0, (name, k)
        assert k["lds"] <= 64 * 1024, (name, k)
