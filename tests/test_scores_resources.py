"""The scoring kernels (csrc/dc_score.hip.h) keep everything in registers: no scratch, no LDS to speak of
(no GPU needed: read from the code object's metadata in the built library, as
tests/test_loglik_resources.py does)."""
import pytest

import code_object


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object.read_kernels(tmp_path_factory)


def _mine(kernels):
    return {k: v for k, v in kernels.items() if "dcs" in k and "outcome_" in k}


def test_score_kernels_exist_without_scratch(kernels):
    mine = _mine(kernels)
    names = " ".join(mine)
    for kind in ("outcome_tilesILb0", "outcome_tilesILb1", "outcome_reduce"):
        assert kind in names, f"{kind} is not in the library"
    for name, k in mine.items():
        assert k["scratch"] == 0, (name, k)
        assert k["lds"] <= 64 * 1024, (name, k)


def test_outcome_tiles_vgprs(kernels):
    # the kernel is bound by float64 VALU issue and uses no LDS, so the registers alone
    # set the occupancy; the design counts on 4 waves per SIMD (16 per CU, one workgroup per SIMD row) to
    # cover the table loads and the dependent chains of exp and log.  Up to 128 VGPRs keep 4 waves per SIMD
    # (512 / 128; the next allocation step, 136, drops to 3)
    tiles = {k: v for k, v in _mine(kernels).items() if "outcome_tiles" in k}
    assert len(tiles) == 2
    for name, k in tiles.items():
        assert k["vgpr"] <= 128, (name, k)
