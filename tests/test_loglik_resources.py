"""The log-likelihood kernels (csrc/dc_loglik.hip.h) keep everything in registers and LDS: no scratch,
at most 64 KB of LDS per workgroup (no GPU needed: read from the code object's metadata in the built library, as
tests/test_kernel_resources.py does)."""
import pytest

import code_object


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object.read_kernels(tmp_path_factory)


def test_loglik_kernels_have_no_scratch(kernels):
    mine = {k: v for k, v in kernels.items() if "dcl" in k and ("loglik" in k or "transpose_f64" in k)}
    names = " ".join(mine)
    for kind in ("loglik_summary", "loglik_matrix", "transpose_f64"):
        assert kind in names, f"{kind} is not in the library"
    for name, k in mine.items():
        assert k["scratch"] == 0, (name, k)
        assert k["lds"] <= 64 * 1024, (name, k)


def test_loglik_summary_vgprs(kernels):
    # its ~44 KB of LDS admit 3 workgroups (3 waves per SIMD) per CU; up to 168 VGPRs
    # keep 3 waves per SIMD, so the registers cost no occupancy
    summ = {k: v for k, v in kernels.items() if "dcl" in k and "loglik_summary" in k}
    assert summ
    for name, k in summ.items():
        assert k["vgpr"] <= 168, (name, k)
