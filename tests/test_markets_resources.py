"""The market kernels (csrc/dc_market.hip.h): both exist in both rate forms, without scratch, within the LDS
and register budget of DESIGN.md section 16 (no GPU needed: read from the code object's metadata in the built
library, as tests/test_scores_resources.py does)."""
import pytest

import code_object


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object.read_kernels(tmp_path_factory)


def _mine(kernels):
    return {k: v for k, v in kernels.items() if "3dcm" in k and "market_" in k}


def test_market_kernels_exist_without_scratch(kernels):
    mine = _mine(kernels)
    names = " ".join(mine)
    for kind in ("market_valuesILb0", "market_valuesILb1", "market_summaryILb0", "market_summaryILb1"):
        assert kind in names, f"{kind} is not in the library"
    assert len(mine) == 4, names
    for name, k in mine.items():
        assert k["scratch"] == 0, (name, k)
        assert k["lds"] <= 64 * 1024, (name, k)


def test_market_values_uses_no_lds(kernels):
    # registers only: the weights come through wave-uniform loads, not LDS
    for name, k in _mine(kernels).items():
        if "market_values" in name:
            assert k["lds"] == 0, (name, k)


def test_vgprs(kernels):
    # market_values is bound by float64 VALU issue; its wave-uniform weight loads are
    # issued one cell (9 float64 instructions, 36 issue cycles) ahead, and the design counts on 4 waves per
    # SIMD to cover the rest of their latency and the chains inside exp.  Up to 128 VGPRs keep 4 waves per
    # SIMD (512 / 128; the next allocation step, 136, drops to 3).  market_summary holds a handful of values
    # per lane and is latency bound on its passes over the stored values: 8 waves per SIMD, at most 64 VGPRs.
    for name, k in _mine(kernels).items():
        assert k["vgpr"] <= (128 if "market_values" in name else 64), (name, k)
