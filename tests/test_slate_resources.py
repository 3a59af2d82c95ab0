"""The slate kernel (csrc/dc_slate.hip.h): it exists in both rate forms, without scratch, within the register
budget of DESIGN.md section 31 and with no static LDS (no GPU needed: read from the code object's metadata in
the built library, as tests/test_markets_resources.py does)."""
import pytest

import code_object


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object.read_kernels(tmp_path_factory)


def _mine(kernels):
    return {k: v for k, v in kernels.items() if "4dcsl" in k and "slate_values" in k}


def test_slate_values_exists_in_both_rate_forms_without_scratch(kernels):
    mine = _mine(kernels)
    names = " ".join(mine)
    for kind in ("slate_valuesILb0", "slate_valuesILb1"):
        assert kind in names, f"{kind} is not in the library"
    assert len(mine) == 2, names
    for name, k in mine.items():
        # the eight accumulators are selected under static indices: no dynamic register indexing, no scratch
        assert k["scratch"] == 0, (name, k)


def test_vgprs(kernels):
    # as market_values: bound by float64 VALU issue, with 4 waves per SIMD (512 / 128 VGPRs) counted on to cover
    # the wave-uniform table loads, the LDS reads of the convolution and the chains inside exp
    for name, k in _mine(kernels).items():
        assert k["vgpr"] <= 128, (name, k)


def test_no_static_lds(kernels):
    # the running pmf is the only LDS and it is dynamic, (P + 1) 512 bytes per call: a small slate leaves room
    # for many workgroups per CU, and nothing static shifts the base off its 16-byte alignment
    for name, k in _mine(kernels).items():
        assert k["lds"] == 0, (name, k)
