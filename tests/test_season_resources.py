"""The season kernel (csrc/dc_season.hip.h) keeps everything in registers and LDS: no scratch
(no GPU needed: read from the code object's metadata in the built library, as
tests/test_kernel_resources.py does)."""
import pytest

import code_object


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object.read_kernels(tmp_path_factory)


def test_season_kernel_has_no_scratch(kernels):
    season = {k: v for k, v in kernels.items() if "dc_season" in k}
    assert season, "the season kernel is not in the library"
    for name, k in season.items():
        assert k["scratch"] == 0, (name, k)
        assert k["lds"] <= 64 * 1024, (name, k)
