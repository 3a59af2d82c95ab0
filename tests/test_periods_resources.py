"""The period kernel (csrc/dc_period.hip.h): it exists in both rate forms, without scratch, within the register
budget of DESIGN.md section 39 and with no static LDS (no GPU needed: read from the code object's metadata in
the built library, as tests/test_slate_resources.py does)."""
import pytest

import code_object


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object.read_kernels(tmp_path_factory)


def _mine(kernels):
    return {k: v for k, v in kernels.items() if "4dcpd" in k and "period_values" in k}


def test_period_values_exists_in_both_rate_forms_without_scratch(kernels):
    mine = _mine(kernels)
    names = " ".join(mine)
    for kind in ("period_valuesILb0", "period_valuesILb1"):
        assert kind in names, f"{kind} is not in the library"
    assert len(mine) == 2, names
    for name, k in mine.items():
        # the eight accumulators and the block's eight values sit under static indices: no scratch
        assert k["scratch"] == 0, (name, k)


def test_vgprs(kernels):
    # as market_values: bound by float64 VALU issue, with 4 waves per SIMD (512 / 128 VGPRs)
    # counted on to cover the wave-uniform weight loads and the chains inside exp
    for name, k in _mine(kernels).items():
        assert k["vgpr"] <= 128, (name, k)


def test_no_static_lds(kernels):
    # registers only: the summary's histograms belong to market_summary
    for name, k in _mine(kernels).items():
        assert k["lds"] == 0, (name, k)
