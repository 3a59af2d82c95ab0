"""The trajectory kernels (csrc/dc_trajectory.hip.h): the simulator in both tie-break forms and the two counting
kernels exist, without scratch, within 128 VGPRs, and their static LDS stays within the bounds DESIGN.md section 29
writes down (no GPU needed: read from the code object's metadata in the built library, as
tests/test_live_resources.py does)."""
import pytest

import code_object

# DESIGN.md section 29, static LDS in bytes
SIM_LDS = 4 * 3 * 64 * 4                # the four waves' tables; the head-to-head matrices are dynamic, dc_h2h.hip.h's
COUNT_LDS = 64 * 4 + 2 * 8 * 4 + 2 * 8  # positions, inside / inside at the end per target, the two sums
PATHS_LDS = 2 * 8 * 257 * 4             # matchdays inside and secured-from, K = 8 and R = 256
H2H_DYNAMIC_MAX = 4 * 48 * 49 * 4       # dch::lds_bytes at its largest (n = 48, four waves)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object.read_kernels(tmp_path_factory)


def _mine(kernels):
    return {k: v for k, v in kernels.items() if "4dctr" in k}


def test_trajectory_kernels_exist_without_scratch_within_128_vgprs(kernels):
    mine = _mine(kernels)
    names = " ".join(mine)
    for kind in ("dc_trajectory_simILb0EEE", "dc_trajectory_simILb1EEE", "dc_trajectory_countENS", "dc_trajectory_pathsENS"):
        assert kind in names, f"{kind} is not in the library"
    assert len(mine) == 4, names
    for name, k in mine.items():
        assert k["scratch"] == 0, (name, k)
        assert k["vgpr"] <= 128, (name, k)


def test_lds_within_the_bounds_written_down(kernels):
    for name, k in _mine(kernels).items():
        bound = SIM_LDS if "trajectory_sim" in name else COUNT_LDS if "trajectory_count" in name else PATHS_LDS
        assert k["lds"] <= bound, (name, k, bound)
    # static plus the largest dynamic part: within the 64 KB a launch gets without an attribute
    assert SIM_LDS + H2H_DYNAMIC_MAX <= 64 * 1024 and PATHS_LDS <= 64 * 1024
