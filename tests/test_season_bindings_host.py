"""The six season query bindings of bpl/_ffi.py without a GPU (match_leverage, season_points, season_scenarios and
their _live forms), under both tie-breaks: the symbol each reaches, an argument list as long as the symbol's
signature, every scalar argument, which pointers are null, and for the live forms the in-play columns behind their
pointers.  A stand-in library in the manner of tests/test_h2h_host.py's records every call while the arrays are alive."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from bpl import _ffi

N, NF, SIMS, KEY = 3, 4, 10, (7, 9)
SEASON = ([0, 1, 0, 2], [1, 0, 2, 1], [0, 1, 2], [[1, 2, 3], [4, 5, 6], [0, 0, 0]], (3, 1, 0), SIMS, KEY)
IN_PLAY = ([1, 2], [2, 0], [1, 0], [0, 3], [0.25, 0.5])
COLUMNS = (np.uint16, np.uint16, np.uint8, np.uint8, np.float64)
LOG_WEIGHTS = [0.0, -1.0, 0.5]
# per query: the arguments after `key`, the scalars between chunk_sims and the outputs, the number of outputs
QUERIES = {"match_leverage": (([1, 3],), [], 3), "season_points": (([1, 3], 2, 40), [2, 40], 4),
           "season_scenarios": (([1, 3], [0, 5], [1, 2]), [2], 4)}    # (the two keys ride with the outputs)


class _KeepingLib:
    """Stands in for the loaded library: every bplhip_* call succeeds; kept are its name, its arguments with the
    pointers reduced to None / True, and the arrays behind the live request's five columns and log weights."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("bplhip_"):
            raise AttributeError(name)

        def call(*args):
            argtypes = _ffi._SIGNATURES[name][1]
            seen = [a if t is not C.c_void_p else (None if a is None or not a.value else True)
                    for a, t in zip(args, argtypes)] if len(args) == len(argtypes) else None
            live = None
            if name.endswith("_live"):
                at = len(args) - 10
                rows = args[at]
                live = [np.ctypeslib.as_array(C.cast(p, C.POINTER(np.ctypeslib.as_ctypes_type(t))), shape=(rows,)).copy()
                        for p, t in zip(args[at + 1:at + 6], COLUMNS)]
                live.append(np.ctypeslib.as_array(C.cast(args[at + 7], C.POINTER(C.c_double)), shape=(len(LOG_WEIGHTS),)).copy())
            self.calls.append((name, len(args), seen, live))
            return 0
        return call


class _NoTorch:
    class cuda:
        device = staticmethod(lambda device: contextlib.nullcontext())


def _hollow_context():
    ctx = _ffi.HipContext.__new__(_ffi.HipContext)
    ctx._lib, ctx._torch, ctx._h, ctx.device = _KeepingLib(), _NoTorch, None, None
    ctx._stream = lambda: None
    return ctx


@pytest.mark.parametrize("head_to_head", [False, True], ids=["overall", "head_to_head"])
@pytest.mark.parametrize("live", [False, True], ids=["kick_off", "live"])
@pytest.mark.parametrize("query", list(QUERIES))
def test_binding_reaches_its_symbol_with_its_arguments(query, live, head_to_head):
    own, own_scalars, n_out = QUERIES[query]
    ctx = _hollow_context()
    kw = dict(chunk_sims=64, head_to_head=head_to_head)       # pair_init None: the zero matrix where the entry reads it
    if live:
        kw.update(in_play=IN_PLAY, reweight=False, log_weights=LOG_WEIGHTS)
    out = getattr(ctx, query + ("_live" if live else ""))(*SEASON, *own, **kw)
    (name, n_args, seen, columns), = ctx._lib.calls
    # match_leverage's kick-off form alone has a symbol per tie-break, the second with pair_init last
    suffix = "_live" if live else "_h2h" if head_to_head and query == "match_leverage" else ""
    assert name == "bplhip_" + query + suffix
    assert n_args == len(_ffi._SIGNATURES[name][1])
    rows = NF + (len(IN_PLAY[0]) if live else 0)
    head = [None, NF, True, True, N, True, True, True, True, 3, 1, 0, SIMS, *KEY, 2, True, 64]
    outputs = [True] * n_out
    tail = [None]                                             # the stream
    if suffix != "" or query != "match_leverage":
        # pair_init: null without the rule; with it the zero matrix, but null for bplhip_match_leverage_h2h
        tail.append(True if head_to_head and suffix != "_h2h" else None)
    if live:
        tail += [len(IN_PLAY[0]), True, True, True, True, True, 0, True, True, True]
    assert seen == head + own_scalars + outputs + tail
    if live:
        for got, want, dtype in zip(columns, IN_PLAY, COLUMNS):
            assert got.dtype == dtype
            np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(columns[5], LOG_WEIGHTS)
        assert (out["ess"], out["log_evidence"]) == (0.0, 0.0)
    else:
        assert "ess" not in out and "log_evidence" not in out
    # the outputs' shapes follow the concatenated list
    if query == "match_leverage":
        assert out["outcome"].shape == (rows, 3) and out["joint"].shape == (rows, 3, N, 2)
    elif query == "season_points":
        assert out["team_target"].shape == (N, 40, 2) and out["gap"].shape == (N - 1, 40)
    else:
        assert out["scenario"].shape == (15,) and out["joint"].shape == (15, N, 2)
    ctx._h = None


def test_live_request_is_checked_before_any_call():
    ctx = _hollow_context()
    for query, (own, _, _) in QUERIES.items():
        with pytest.raises(ValueError, match="in-play columns must have equal length"):
            getattr(ctx, query + "_live")(*SEASON, *own, in_play=([1], [2, 0], [1], [0], [0.5]))
    with pytest.raises(ValueError, match="one-dimensional and of equal length"):
        ctx.season_scenarios_live(*SEASON, [1], [0, 5], [1], in_play=IN_PLAY)
    assert ctx._lib.calls == []
    ctx._h = None
