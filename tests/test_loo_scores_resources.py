"""The leave-one-out forecast kernel (csrc/dc_loo.hip.h) keeps everything in registers and LDS: no scratch, at
most 64 KB of LDS per workgroup, and no more registers than keep loglik_summary's occupancy (no GPU needed: read
from the code object's metadata in the built library, as tests/test_loglik_resources.py does)."""
import pytest

import code_object


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object.read_kernels(tmp_path_factory)


def _mine(kernels):
    return {k: v for k, v in kernels.items() if "5dcloo" in k and "loo_forecast" in k}


def test_both_forms_are_in_the_library(kernels):
    mine = _mine(kernels)
    assert len(mine) == 2, sorted(mine)
    for form in ("loo_forecastILb0EEE", "loo_forecastILb1EEE"):   # <false>: plain, <true>: venue
        assert sum(form in k for k in mine) == 1, (form, sorted(mine))


def test_no_scratch_and_the_lds_of_loglik_summary(kernels):
    mine = _mine(kernels)
    assert mine
    for name, k in mine.items():
        assert k["scratch"] == 0, (name, k)
        assert k["lds"] <= 64 * 1024, (name, k)


def test_vgprs_keep_three_waves_per_simd(kernels):
    # DESIGN.md sections 12 and 32: the ~44 KB of LDS admit 3 workgroups (3 waves per SIMD) per CU; up to 168 VGPRs
    # keep 3 waves per SIMD, so the registers cost no occupancy
    mine = _mine(kernels)
    assert mine
    for name, k in mine.items():
        assert k["vgpr"] <= 168, (name, k)


def test_the_kernel_is_outside_the_other_files_filters(kernels):
    # the name filters of tests/test_loglik_resources.py and tests/test_scores_resources.py
    for name in _mine(kernels):
        assert "loglik" not in name and "outcome_" not in name and "dcs" not in name, name
