"""The sequential-update kernels (csrc/dc_sequential.hip.h) exist for both rate forms, use no scratch and stay
within the register and LDS numbers of DESIGN.md section 17 (no GPU needed: read from the code object's
metadata in the built library, as tests/test_scores_resources.py does)."""
import pytest

import code_object


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object.read_kernels(tmp_path_factory)


def _mine(kernels):
    return {k: v for k, v in kernels.items() if "3dcu" in k}


def test_sequential_kernels_exist_without_scratch(kernels):
    mine = _mine(kernels)
    names = " ".join(mine)
    for kind in ("block_ll_tilesILb0", "block_ll_tilesILb1", "block_ll_reduce", "psis_rows", "weighted_tilesILb0",
                 "weighted_tilesILb1", "weighted_reduce"):
        assert kind in names, f"{kind} is not in the library"
    assert len(mine) == 7
    for name, k in mine.items():
        assert k["scratch"] == 0, (name, k)


def test_tiles_use_registers_only(kernels):
    # block_ll_tiles and weighted_tiles keep everything in registers (no LDS, no barrier).
    # Both are bound by float64 VALU issue on wave-uniform, coalesced loads; as in section 15 the design counts on
    # 4 waves per SIMD to cover the loads and the dependent chains of exp and log: at most 128 VGPRs (512 / 128;
    # the next allocation step, 136, drops to 3)
    tiles = {k: v for k, v in _mine(kernels).items() if "_tiles" in k}
    assert len(tiles) == 4
    for name, k in tiles.items():
        assert k["lds"] == 0, (name, k)
        assert k["vgpr"] <= 128, (name, k)


def test_psis_rows_budget(kernels):
    # one wave per workgroup: 8 KB keys + 2 KB draw indices + 1 KB histogram + the cutoff, a quarter of
    # loglik_summary's LDS; at most 128 VGPRs, so that 4 single-wave workgroups fit a SIMD and registers
    # never bound the number of blocks in flight before the 160 KB of LDS do (14 workgroups per CU)
    rows = {k: v for k, v in _mine(kernels).items() if "psis_rows" in k}
    assert len(rows) == 1
    for name, k in rows.items():
        assert k["lds"] <= 11 * 1024 + 64, (name, k)
        assert k["vgpr"] <= 128, (name, k)


def test_reduce_kernels_are_small(kernels):
    for name, k in _mine(kernels).items():
        if "_reduce" in name:
            assert k["lds"] == 0 and k["vgpr"] <= 64, (name, k)
