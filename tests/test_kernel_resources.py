"""Register budget of the kernels whose occupancy was measured to matter (no GPU needed: read
from the code object's metadata in the built library).  dc_eval runs 512-thread workgroups;
above 128 VGPRs only one fits a CU, which costs ~20 % when 8-32 chains share a GPU
(DESIGN.md section 5), and scratch means spilling in the evaluation's hot loop."""
import pytest

import code_object


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object.read_kernels(tmp_path_factory)


def _eval_name(weighted, clip, staged, nuts):
    b = lambda v: "Lb1E" if v else "Lb0E"
    # (round 4: five pointers and four ints in front of the argument block -- the ones gfx950 preloads into SGPRs)
    return f"_ZN2dc7dc_evalI{b(weighted)}{b(clip)}{b(staged)}{b(nuts)}EEvPKdPKjS4_S4_S4_iiiiNS_8EvalArgsE"


def test_every_eval_variant_is_built(kernels):
    for w in (0, 1):
        for c in (0, 1):
            for s in (0, 1):
                for n in (0, 1):
                    assert _eval_name(w, c, s, n) in kernels


def test_every_persistent_loop_variant_is_built(kernels):
    """dc_eval_loop<weighted, clip, leaf elements per lane>: presence only (their register and scratch figures are
    not budgeted here)."""
    for w in (0, 1):
        for c in (0, 1):
            for lne in (1, 2):
                assert f"_ZN2dc12dc_eval_loopILb{w}ELb{c}ELi{lne}EEEvNS_8EvalArgsE" in kernels


def test_headline_kernels_fit_two_workgroups_per_cu(kernels):
    # the basic model, <= 64 teams: plain evaluation and the NUTS-aware launch
    for nuts in (0, 1):
        k = kernels[_eval_name(0, 0, 1, nuts)]
        assert k["vgpr"] <= 128, k
        assert k["scratch"] == 0, k
    # the extended model's NUTS-aware launch stays at two workgroups per CU as well
    k = kernels[_eval_name(0, 1, 1, 1)]
    assert k["vgpr"] <= 128 and k["scratch"] == 0, k


def test_no_spills_in_unweighted_staged_kernels(kernels):
    for c in (0, 1):
        for n in (0, 1):
            assert kernels[_eval_name(0, c, 1, n)]["scratch"] == 0
