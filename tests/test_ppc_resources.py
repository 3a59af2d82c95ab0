"""The posterior predictive kernels (csrc/dc_ppc.hip.h) keep everything in registers and LDS: no scratch, at
most 64 KB of LDS per workgroup, and the VGPR bound of DESIGN.md section 13 (no GPU needed: read from the code
object's metadata in the built library, as tests/test_loglik_resources.py does)."""
import pytest

import code_object


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object.read_kernels(tmp_path_factory)


def _ppc(kernels):
    return {k: v for k, v in kernels.items() if "dcppc" in k and "dc_ppc" in k}


def test_ppc_kernels_exist_without_scratch(kernels):
    mine = _ppc(kernels)
    assert len(mine) == 2, sorted(mine)   # the plain and the venue form
    for name, k in mine.items():
        assert k["scratch"] == 0, (name, k)
        assert k["lds"] <= 64 * 1024, (name, k)


def test_ppc_vgprs(kernels):
    # up to 96 VGPRs keep 5 waves per SIMD (one 256-lane workgroup per replication)
    for name, k in _ppc(kernels).items():
        assert k["vgpr"] <= 96, (name, k)
