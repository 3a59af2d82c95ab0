"""The sensitivity kernel (csrc/dc_sensitivity.hip.h) exists in the built library, without scratch, within the
register and LDS budget of DESIGN.md section 33 (no GPU needed: read from the code object's metadata in the built
library, as tests/test_inplay_resources.py does)."""
import pytest

import code_object

LDS_DRAWS = 12288            # csrc/dc_sensitivity.hip.h SHIFT_LDS_DRAWS: S up to here sorts in LDS, 12 bytes per draw
LDS_BUDGET = 160 * 1024      # a gfx950 workgroup's LDS


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return {k: v for k, v in code_object.read_kernels(tmp_path_factory).items() if "4dcps" in k}


def test_shift_summary_exists_without_scratch(kernels):
    assert [k for k in kernels if "shift_summary" in k], "shift_summary is not in the library"
    assert len(kernels) == 1, " ".join(kernels)
    for name, k in kernels.items():
        assert k["scratch"] == 0, (name, k)


def test_shift_summary_fits_the_lds_with_the_most_draws_in_it(kernels):
    # static LDS (histograms, segment totals) plus the dynamic 12 bytes per draw (keys, two index buffers); at the
    # dynamic model's S = 4000 (46.9 KiB dynamic) three workgroups share a CU, 3 waves per SIMD: 128 VGPRs admit 4
    (name, k), = kernels.items()
    assert k["lds"] + 12 * LDS_DRAWS <= LDS_BUDGET, (name, k)
    assert 3 * (k["lds"] + 12 * 4000) <= LDS_BUDGET, (name, k)
    assert k["vgpr"] <= 128, (name, k)
