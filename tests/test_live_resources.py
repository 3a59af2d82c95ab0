"""The live-season kernels (csrc/dc_live.hip.h): all three exist (the simulator in both tie-break forms), without
scratch, within 128 VGPRs, and the simulator's static LDS is dc_season's -- DESIGN.md section 26 adds nothing to it
(no GPU needed: read from the code object's metadata in the built library, as tests/test_season_resources.py does)."""
import pytest

import code_object

LIVE_LDS_EXTRA = 0   # the search of the scan and the conditional sampler live in registers


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object.read_kernels(tmp_path_factory)


def _mine(kernels):
    return {k: v for k, v in kernels.items() if "6dclive" in k}


def test_live_kernels_exist_without_scratch_within_128_vgprs(kernels):
    mine = _mine(kernels)
    names = " ".join(mine)
    for kind in ("live_loglikENS", "live_weightsENS", "dc_season_liveILb0EEE", "dc_season_liveILb1EEE"):
        assert kind in names, f"{kind} is not in the library"
    assert len(mine) == 4, names
    for name, k in mine.items():
        assert k["scratch"] == 0, (name, k)
        assert k["vgpr"] <= 128, (name, k)


def test_the_simulator_keeps_dc_seasons_static_lds(kernels):
    for form in ("ILb0EEE", "ILb1EEE"):
        season = [v for k, v in kernels.items() if "3dcs" in k and "dc_season" + form in k]
        live = [v for k, v in _mine(kernels).items() if "dc_season_live" + form in k]
        assert len(season) == 1 and len(live) == 1
        assert live[0]["lds"] <= season[0]["lds"] + LIVE_LDS_EXTRA, (form, live[0], season[0])


def test_the_small_kernels_fit_any_number_of_draws(kernels):
    # live_loglik keeps no LDS; live_weights' is static (the segment totals and the wave maxima), whatever S is
    for name, k in _mine(kernels).items():
        if "live_loglik" in name:
            assert k["lds"] == 0, (name, k)
        if "live_weights" in name:
            assert k["lds"] <= 4096, (name, k)
