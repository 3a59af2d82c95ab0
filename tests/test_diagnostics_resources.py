"""The diagnostics kernels (csrc/dc_diagnostics.hip.h) exist in the built library, keep everything in registers and
LDS, and stay within the bounds DESIGN.md section 20 derives from their occupancy (no GPU needed: read from the
code object's metadata, as tests/test_loglik_resources.py does)."""
import pytest

import code_object

DIAG_LDS_DRAWS = 12288   # csrc/dc_diagnostics.hip.h: S up to here sorts in LDS, 12 bytes per draw


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return {k: v for k, v in code_object.read_kernels(tmp_path_factory).items() if "3dcg" in k}


def test_diagnostics_kernels_exist_without_scratch(kernels):
    names = " ".join(kernels)
    for kind in ("diag_rank", "diag_ess"):
        assert kind in names, f"{kind} is not in the library"
    for name, k in kernels.items():
        assert k["scratch"] == 0, (name, k)


def test_diag_rank_fits_one_cu_at_its_largest_lds_sort(kernels):
    # static LDS (histograms, chain records) + 12 bytes per draw of dynamic LDS at S = 12 288 within 160 KiB per CU;
    # at the dynamic model's S = 4000 (46.9 KiB dynamic) two workgroups share a CU, far below what 128 VGPRs
    # (4 waves per SIMD) admit, so the registers cost no occupancy
    (name, k), = [(n, v) for n, v in kernels.items() if "diag_rank" in n]
    assert k["lds"] <= 16 * 1024, (name, k)
    assert k["lds"] + 12 * DIAG_LDS_DRAWS <= 160 * 1024, (name, k)
    assert 2 * (k["lds"] + 12 * 4000) <= 160 * 1024, (name, k)
    assert k["vgpr"] <= 128, (name, k)


def test_diag_ess_keeps_six_waves_per_simd(kernels):
    # 4 waves x 512 chain means = 16 KiB per workgroup: six workgroups (6 waves per SIMD) need 96 KiB and <= 80 VGPRs
    (name, k), = [(n, v) for n, v in kernels.items() if "diag_ess" in n]
    assert k["lds"] <= 16 * 1024, (name, k)
    assert k["vgpr"] <= 80, (name, k)
