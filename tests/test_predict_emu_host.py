"""The float32 method of `predict_score_grid` by itself: the numpy emulation of the kernel's walk
(tests/predict_emu.py) against the float64 restatement (tests/fake_ctx.py:FakePredictCtx) on a representative
subset of the input sets of tests/test_gpu_predict.py.  It has to stay within HALF of the grid gate
(err <= 3e-6 * want + 1e-12 per cell): then the inputs are fair, and a device result outside the gate is the
kernel's fault, not the method's.  An input set above 0.5 is replaced, the figure stays."""
import numpy as np
import pytest

import predict_emu as PE
from fake_ctx import FakePredictCtx
from loglik_ref import KINDS


def _ratio(kind, S, T, M, G, pattern=None):
    venue, args, h, a, kw = PE.case(kind, S, T, M, pattern=pattern)
    emu, ref = PE.GridEmu(), FakePredictCtx()
    PE.set_posterior(emu, venue, args)
    PE.set_posterior(ref, venue, args)
    got = emu.predict_score_grid(h, a, G, **kw)
    want = ref.predict_score_grid(h, a, G, kw.get("neutral"), kw.get("conf"))
    assert got.shape == want.shape and not np.isnan(got).any() and (got >= 0.0).all()
    ratio = (np.abs(got - want) / PE.grid_bound(want)).max()
    print(f"{kind} S={S} T={T} M={M} max_goals={G} {pattern or ''}: largest err / bound {ratio:.3f}")
    return ratio, got, want


@pytest.mark.parametrize("S,G", [(S, 16) for S in (1, 2, 63, 64, 65, 127, 128, 255, 256, 257, 320, 321)]
                         + [(1, 63), (257, 63), (321, 63), (64, 0), (65, 15), (256, 15)])
def test_draw_counts_and_depths(S, G):
    assert _ratio("basic", S, 6, 5, G)[0] <= 0.5


@pytest.mark.parametrize("M,S,G", [(9, 65, 17), (1, 65, 17), (3, 130, 31), (3, 130, 32), (3, 130, 47), (3, 130, 48)])
def test_fixture_counts_and_tile_edges(M, S, G):
    assert _ratio("basic", S, 6, M, G)[0] <= 0.5


@pytest.mark.parametrize("kind", KINDS)
def test_all_kinds(kind):
    assert _ratio(kind, 257, 8, 7, 31)[0] <= 0.5


@pytest.mark.parametrize("kind", ["extended", "wc"])
def test_three_hundred_teams(kind):
    assert _ratio(kind, 65, 300, 7, 17)[0] <= 0.5


@pytest.mark.parametrize("kind,S,T,M,G", [("basic", 130, 8, 5, 17), ("wc", 130, 8, 5, 17), ("neutral", 321, 8, 9, 20),
                                          ("basic", 257, 8, 5, 17), ("basic", 5, 3, 5, 17), ("wc", 65, 6, 5, 17),
                                          ("extended", 64, 5, 5, 17)])
def test_cross_check_and_replacement_inputs(kind, S, T, M, G):
    assert _ratio(kind, S, T, M, G)[0] <= 0.5


@pytest.mark.parametrize("S", [64, 257])
@pytest.mark.parametrize("pattern", PE.CLIP_PATTERNS)
def test_clipped_tau(pattern, S):
    ratio, got, want = _ratio("basic", S, 6, 5, 15, pattern=pattern)
    assert ratio <= 0.5
    tau = (np.abs(got - want) / PE.grid_bound(want))[:, :2, :2].max()
    print(f"{pattern} S={S}: the four tau cells, largest err / bound {tau:.3f}")
    zero = want == 0.0
    if pattern == "all":
        assert zero[:, 1, 1].all()
    assert (got[zero] == 0.0).all()
