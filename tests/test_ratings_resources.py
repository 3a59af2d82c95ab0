"""The rating kernels (csrc/dc_ratings.hip.h): both exist in both rate forms, without scratch, within the LDS
and register budget of DESIGN.md section 27 (no GPU needed: read from the code object's metadata in the built
library, as tests/test_markets_resources.py does)."""
import pytest

import code_object


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object.read_kernels(tmp_path_factory)


def _mine(kernels):
    return {k: v for k, v in kernels.items() if "3dcr" in k and "ratings_" in k}


def test_rating_kernels_exist_without_scratch(kernels):
    mine = _mine(kernels)
    names = " ".join(mine)
    for kind in ("ratings_valuesILb0", "ratings_valuesILb1", "ratings_rankILb0", "ratings_rankILb1"):
        assert kind in names, f"{kind} is not in the library"
    assert len(mine) == 4, names
    for name, k in mine.items():
        assert k["scratch"] == 0, (name, k)


def test_ratings_values_uses_no_lds_and_keeps_four_waves(kernels):
    # registers only; bound by float64 VALU issue in dcs::outcome_probs' walk and the chains inside exp: up to 128
    # VGPRs keep 4 waves per SIMD (512 / 128), the argument of tests/test_markets_resources.py
    for name, k in _mine(kernels).items():
        if "ratings_values" in name:
            assert k["lds"] == 0, (name, k)
            assert k["vgpr"] <= 128, (name, k)


def test_ratings_rank_budget(kernels):
    # two int32 rows of RATINGS_MAX_TEAMS counters per wave; latency bound on its passes over the stored values:
    # 8 waves per SIMD by registers, at most 64 VGPRs
    for name, k in _mine(kernels).items():
        if "ratings_rank" in name:
            assert 0 < k["lds"] <= 64 * 1024, (name, k)
            assert k["vgpr"] <= 64, (name, k)
