"""The live query kernels (csrc/dc_live_queries.hip.h): the three recording kernels exist in both tie-break forms,
without scratch, within the 128 VGPRs dc_season_live is held to, and with no more static LDS than their kick-off
twins -- the search of the scan and the conditional sampler live in registers (no GPU needed: read from the code
object's metadata in the built library, as tests/test_season_resources.py does)."""
import pytest

import code_object

# (live kernel, its kick-off twin, the twin's namespace as mangled)
PAIRS = (("live_leverage_sim", "dc_leverage_sim", "5dclev"), ("live_points_sim", "dc_points_sim", "4dcpt"),
         ("live_scenario_sim", "dc_scenario_sim", "4dcsc"))
FORMS = ("ILb0EEE", "ILb1EEE")   # <false>: the overall order, <true>: head to head


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object.read_kernels(tmp_path_factory)


def _mine(kernels):
    return {k: v for k, v in kernels.items() if k.startswith("_ZN4dclq")}


def test_the_six_instantiations_exist_without_scratch_within_128_vgprs(kernels):
    mine = _mine(kernels)
    names = " ".join(mine)
    for live, _, _ in PAIRS:
        for form in FORMS:
            assert sum(live + form in k for k in mine) == 1, f"{live}{form}: {names}"
    assert len(mine) == 6, names
    for name, k in mine.items():
        assert k["scratch"] == 0, (name, k)
        assert k["vgpr"] <= 128, (name, k)


def test_static_lds_is_no_more_than_the_kick_off_twins(kernels):
    for live, twin, space in PAIRS:
        for form in FORMS:
            mine = [v for k, v in _mine(kernels).items() if live + form in k]
            theirs = [v for k, v in kernels.items() if k.startswith("_ZN" + space) and twin + form in k]
            assert len(mine) == 1 and len(theirs) == 1, (live, form)
            assert mine[0]["lds"] <= theirs[0]["lds"], (live, form, mine[0], theirs[0])


def test_the_counting_kernels_are_not_instantiated_again(kernels):
    for count in ("dc_leverage_count", "dc_points_count", "dc_scenario_count"):
        assert sum(count in k for k in kernels) == 1, count
