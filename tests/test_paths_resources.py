"""The tournament_paths kernels (csrc/dc_paths.hip.h) are in the built library and stay within the tournament
kernels' gates: no scratch, at most 64 KB of LDS and 128 VGPRs (no GPU needed: read from the code object's metadata
in the built library, as tests/test_tournament_resources.py does)."""
import pytest

import code_object


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object.read_kernels(tmp_path_factory)


def test_paths_kernel_resources(kernels):
    sims = {k: v for k, v in kernels.items() if "dc_paths_sim" in k}
    count = {k: v for k, v in kernels.items() if "dc_paths_count" in k}
    # head-to-head x extra time: four recording kernels, and the one counting kernel
    assert len(sims) == 4 and len(count) == 1, sorted(kernels)
    for name, k in {**sims, **count}.items():
        assert k["scratch"] == 0, (name, k)
        assert k["lds"] <= 64 * 1024, (name, k)
        assert k["vgpr"] <= 128, (name, k)
    # the counting kernel's one LDS table: [64][64] u32
    assert next(iter(count.values()))["lds"] == 64 * 64 * 4
    # the group-fixture tables come from match_leverage's counting kernel, which is still the only one of its kind
    assert len([k for k in kernels if "dc_leverage_count" in k]) == 1
