"""The head-to-head instantiations of the table simulators (csrc/dc_h2h.hip.h) keep everything in registers and LDS: no scratch, at most 64 KB
of static LDS (the pair matrices are dynamic LDS on top, sized by the table), and the tournament one at most 128
VGPRs as its model kernel (no GPU needed: read from the code object's metadata in the built library, as
tests/test_season_resources.py does)."""
import pytest

import code_object

KERNELS = ("dc_seasonILb1EEE", "dc_leverage_simILb1EEE", "dc_tournamentILb1EEE")   # <true>: head to head


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object.read_kernels(tmp_path_factory)


@pytest.mark.parametrize("kernel", KERNELS)
def test_head_to_head_kernel_resources(kernels, kernel):
    found = {k: v for k, v in kernels.items() if kernel in k}
    assert len(found) == 1, (kernel, sorted(found))
    for name, k in found.items():
        assert k["scratch"] == 0, (name, k)
        assert k["lds"] <= 64 * 1024, (name, k)
        if kernel == "dc_tournamentILb1EEE":
            assert k["vgpr"] <= 128, (name, k)


def test_the_default_path_kernels_are_still_there(kernels):
    """The head-to-head forms are additions: the kernels the default keywords launch are there, once each."""
    for kernel in ("dc_seasonILb0EEE", "dc_leverage_simILb0EEE", "dc_leverage_countENS", "dc_tournamentILb0EEE"):
        assert sum(kernel in k for k in kernels) == 1, kernel
