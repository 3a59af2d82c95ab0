"""The five summary bindings of bpl/_ffi.py without a GPU (market_summary, period_summary, inplay_summary,
slate_summary, team_ratings), in the manner of tests/test_season_bindings_host.py: the symbol each reaches, an
argument list as long as the symbol's signature, every scalar argument, which pointers are null (with and without
return_draws, log_weights and conf; without quantiles the count 0 is pinned, not what the two pointers are: the binding
passes its empty arrays as they stand), and what the method makes of the buffers the library fills: the
stand-in library writes the ramp 0, 1, 2, ... into every output, so the shapes, the key order and the transposes
of the returned dict are pinned ([m, K, S] to [S, K, m]; slate's [J, P+1, S] to [S, J, P+1] and [8, m] to
"leg_proba" [m, 8]; in-play's [m, S] to "draw_log_evidence" [S, m]).  Then the ValueErrors the methods raise
themselves, and the P / K slate_summary derives where the library would refuse the call."""
import contextlib
import ctypes as C
import re

import numpy as np
import pytest

from bpl import _ffi

S, M, K, G = 3, 2, 2, 2
H, A = [0, 2], [1, 3]
# per method: the symbol's parameter names after the context, the outputs among them with their dtypes
PARAMS = {
    "market_summary": "q max_goals n_markets weights n_quantiles quantiles mean sd quantile draws workspace stream",
    "period_summary": "q split max_goals n_markets weights n_quantiles quantiles mean sd quantile draws workspace stream",
    "inplay_summary": "q elapsed max_goals n_markets weights n_quantiles quantiles reweight log_weights mean sd quantile "
                      "ess log_evidence draws draw_log_evidence workspace stream",
    "slate_summary": "q max_goals n_slates start n_tables tables leg_table n_quantiles quantiles mean sd quantile "
                     "leg_mean draws workspace stream",
    "team_ratings": "n_teams teams team_conf n_opponents opponents opponent_conf venue max_goals points rank_by "
                    "n_quantiles quantiles mean sd quantile rank_count better_count matches draws workspace stream",
}
INT32_OUT = ("rank_count", "better_count", "matches")


class _FillingLib:
    """Stands in for the loaded library: every bplhip_* call succeeds and is kept as (name, argument count, the
    arguments by parameter name: scalars as they are, pointers as None / True, the fixtures record as (m, venue,
    its non-null columns)).  `sizes` (parameter name -> element count, set by the test) are the outputs it fills
    with 0, 1, 2, ..."""

    def __init__(self):
        self.calls, self.sizes = [], {}

    def __getattr__(self, name):
        if not name.startswith("bplhip_"):
            raise AttributeError(name)

        def call(*args):
            names = ["ctx"] + PARAMS[name[len("bplhip_"):]].split()
            seen = {}
            for key, a, t in zip(names, args, _ffi._SIGNATURES[name][1]):
                if t is _ffi._fx:
                    rec = a._obj
                    seen[key] = (rec.m, rec.venue, sorted(f for f, _ in rec._fields_[2:] if getattr(rec, f)))
                elif t is C.c_void_p:
                    seen[key] = None if a is None or not a.value else True
                    if key in self.sizes and seen[key]:
                        ctype = C.c_int32 if key in INT32_OUT else C.c_double
                        np.ctypeslib.as_array(C.cast(a, C.POINTER(ctype)), shape=(self.sizes[key],))[:] = np.arange(self.sizes[key])
                else:
                    seen[key] = a
            self.calls.append((name, len(args), seen))
            return 0
        return call


class _NoTorch:
    class cuda:
        device = staticmethod(lambda device: contextlib.nullcontext())


def _hollow_context():
    ctx = _ffi.HipContext.__new__(_ffi.HipContext)
    ctx._lib, ctx._torch, ctx._h, ctx.device = _FillingLib(), _NoTorch, None, None
    ctx._stream = lambda: None
    ctx.pred_draws = S
    return ctx


def _ramp(*shape):
    return np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape)


def _one_call(ctx):
    (name, n_args, seen), = ctx._lib.calls
    assert n_args == len(_ffi._SIGNATURES[name][1])
    if seen["n_quantiles"] == 0:          # (what address numpy gives an empty array is not the binding's to decide)
        seen["quantiles"] = seen["quantile"] = None
    return name, seen


def _check_returned(out, keys, want):
    assert list(out) == keys
    for key, value in want.items():
        assert out[key].shape == value.shape and out[key].dtype == value.dtype and out[key].flags.c_contiguous, key
        np.testing.assert_array_equal(out[key], value)


@pytest.mark.parametrize("quantiles", [(), (0.25, 0.75)], ids=["no_quantiles", "two_quantiles"])
@pytest.mark.parametrize("venue", [False, True], ids=["plain", "venue_conf"])
@pytest.mark.parametrize("return_draws", [False, True], ids=["summary", "draws"])
@pytest.mark.parametrize("method", ["market_summary", "period_summary", "inplay_summary"])
def test_fixture_summaries_reach_their_symbol(method, return_draws, venue, quantiles):
    ctx = _hollow_context()
    NQ = len(quantiles)
    kw = dict(quantiles=quantiles, return_draws=return_draws, workspace_bytes=4096)
    if venue:
        kw.update(neutral=[0, 1], conf=([0, 1], [1, 0]))
    ctx._lib.sizes = dict(mean=K * M, sd=K * M, quantile=K * NQ * M, draws=M * K * S, ess=M, log_evidence=M,
                          draw_log_evidence=M * S)
    cells = (G + 1) ** (4 if method == "period_summary" else 2)
    if method == "market_summary":
        out = ctx.market_summary(H, A, G, np.zeros((K, cells)), **kw)
    elif method == "period_summary":
        out = ctx.period_summary(H, A, [0.5, 0.25], G, np.zeros((K, cells)), **kw)
    else:
        kw.update(reweight=False, log_weights=[0.0, -1.0, 0.5] if return_draws else None)
        out = ctx.inplay_summary(H, A, [1, 0], [0, 0], [0.5, 0.25], G, np.zeros((K, cells)), **kw)
    name, seen = _one_call(ctx)
    assert name == "bplhip_" + method
    columns = ["away_idx", "home_idx"] + (["away_goals", "home_goals"] if method == "inplay_summary" else [])
    want = dict(ctx=None, q=(M, int(venue), sorted(columns + (["away_conf", "home_conf", "neutral_venue"] if venue else []))),
                max_goals=G, n_markets=K, weights=True, n_quantiles=NQ, quantiles=True if NQ else None, mean=True,
                sd=True, quantile=True if NQ else None, draws=True if return_draws else None, workspace=4096, stream=None)
    if method == "period_summary":
        want.update(split=True)
    if method == "inplay_summary":
        want.update(elapsed=True, reweight=0, log_weights=True if return_draws else None, ess=True, log_evidence=True,
                    draw_log_evidence=True if return_draws else None)
    assert seen == want
    keys = ["mean", "sd", "quantile"] + (["ess", "log_evidence"] if method == "inplay_summary" else [])
    values = dict(mean=_ramp(K, M), sd=_ramp(K, M))
    if NQ:
        values.update(quantile=_ramp(K, NQ, M))
    if method == "inplay_summary":
        values.update(ess=_ramp(M), log_evidence=_ramp(M))
    if return_draws:
        keys.append("draws")
        values.update(draws=_ramp(M, K, S).transpose(2, 1, 0).copy())
        if method == "inplay_summary":
            keys.append("draw_log_evidence")
            values.update(draw_log_evidence=_ramp(M, S).T.copy())
    _check_returned(out, keys, values)
    assert out["quantile"].shape == (K, NQ, M)
    ctx._h = None


@pytest.mark.parametrize("quantiles", [(), (0.25, 0.75)], ids=["no_quantiles", "two_quantiles"])
@pytest.mark.parametrize("venue", [False, True], ids=["plain", "venue_conf"])
@pytest.mark.parametrize("return_draws", [False, True], ids=["summary", "draws"])
def test_slate_summary_reaches_its_symbol(return_draws, venue, quantiles):
    ctx = _hollow_context()
    NQ, m, J, P = len(quantiles), 3, 2, 4            # tops 1 and 3: slates of 1 + 3 and 3 points
    KS = 2 * (P + 1) + 2
    tables = np.zeros((2, G + 1, G + 1), dtype=np.uint8)
    tables[0, 1, 0], tables[1, 2, 2] = 1, 3
    kw = dict(quantiles=quantiles, return_draws=return_draws, workspace_bytes=4096)
    if venue:
        kw.update(neutral=1, conf=([0, 1, 0], [1, 0, 1]))
    ctx._lib.sizes = dict(mean=KS * J, sd=KS * J, quantile=KS * NQ * J, leg_mean=8 * m, draws=J * (P + 1) * S)
    out = ctx.slate_summary([0, 2, 1], [1, 3, 0], G, tables, [0, 1, 1], [0, 2, 3], **kw)
    name, seen = _one_call(ctx)
    assert name == "bplhip_slate_summary"
    columns = ["away_idx", "home_idx"] + (["away_conf", "home_conf", "neutral_venue"] if venue else [])
    assert seen == dict(ctx=None, q=(m, int(venue), sorted(columns)), max_goals=G, n_slates=J, start=True, n_tables=2,
                        tables=True, leg_table=True, n_quantiles=NQ, quantiles=True if NQ else None, mean=True, sd=True,
                        quantile=True if NQ else None, leg_mean=True, draws=True if return_draws else None,
                        workspace=4096, stream=None)
    values = dict(mean=_ramp(KS, J), sd=_ramp(KS, J), leg_proba=_ramp(8, m).T.copy())
    if NQ:
        values.update(quantile=_ramp(KS, NQ, J))
    if return_draws:
        values.update(draws=_ramp(J, P + 1, S).transpose(2, 0, 1).copy())
    _check_returned(out, ["mean", "sd", "quantile", "leg_proba"] + (["draws"] if return_draws else []), values)
    assert out["quantile"].shape == (KS, NQ, J)
    ctx._h = None


@pytest.mark.parametrize("quantiles", [(), (0.25, 0.75)], ids=["no_quantiles", "two_quantiles"])
@pytest.mark.parametrize("conf", [False, True], ids=["plain", "conf"])
@pytest.mark.parametrize("return_draws", [False, True], ids=["summary", "draws"])
def test_team_ratings_reaches_its_symbol(return_draws, conf, quantiles):
    ctx = _hollow_context()
    NQ, R, NO, KR = len(quantiles), 3, 4, 5
    kw = dict(rank_by=2, quantiles=quantiles, return_draws=return_draws, workspace_bytes=4096)
    if conf:
        kw.update(team_conf=[0, 1, 0], opponent_conf=[1, 0, 1, 0])
    ctx._lib.sizes = dict(mean=KR * R, sd=KR * R, quantile=KR * NQ * R, rank_count=R * R, better_count=R * R, matches=R,
                          draws=R * KR * S)
    out = ctx.team_ratings([0, 1, 2], [0, 1, 2, 3], 1, G, (3, 1, 0), **kw)
    name, seen = _one_call(ctx)
    assert name == "bplhip_team_ratings"
    assert seen == dict(ctx=None, n_teams=R, teams=True, team_conf=True if conf else None, n_opponents=NO,
                        opponents=True, opponent_conf=True if conf else None, venue=1, max_goals=G, points=True,
                        rank_by=2, n_quantiles=NQ, quantiles=True if NQ else None, mean=True, sd=True,
                        quantile=True if NQ else None, rank_count=True, better_count=True, matches=True,
                        draws=True if return_draws else None, workspace=4096, stream=None)
    counts = np.arange(R * R, dtype=np.int32).reshape(R, R)
    values = dict(mean=_ramp(KR, R), sd=_ramp(KR, R), rank_count=counts, better_count=counts,
                  matches=np.arange(R, dtype=np.int32))
    if NQ:
        values.update(quantile=_ramp(KR, NQ, R))
    if return_draws:
        values.update(draws=_ramp(R, KR, S).transpose(2, 1, 0).copy())
    _check_returned(out, ["mean", "sd", "quantile", "rank_count", "better_count", "matches"]
                    + (["draws"] if return_draws else []), values)
    assert out["quantile"].shape == (KR, NQ, R)
    ctx._h = None


W2, W4 = np.zeros((K, (G + 1) ** 2)), np.zeros((K, (G + 1) ** 4))
TABLES = np.zeros((2, G + 1, G + 1), dtype=np.uint8)
REFUSED = [
    ("market_summary", (H, A, G, W4), {}, "weights must have shape [K, max_goals+1, max_goals+1]"),
    ("market_summary", (H, [1], G, W2), {}, "query arrays must have equal length"),
    ("period_summary", (H, A, [0.5], G, W4), {}, "split must have one value per fixture"),
    ("period_summary", (H, A, [0.5, 0.5], G, W2), {},
     "weights must have shape [K, max_goals+1, max_goals+1, max_goals+1, max_goals+1]"),
    ("inplay_summary", (H, A, [0, 0], [0, 0], [0.5], G, W2), {}, "elapsed must have one value per fixture"),
    ("inplay_summary", (H, A, [0, 0], [0, 0], [0.5, 0.5], G, W4), {},
     "weights must have shape [K, max_goals+1, max_goals+1]"),
    ("inplay_summary", (H, A, [0, 0], [0, 0], [0.5, 0.5], G, W2), dict(log_weights=[0.0] * (S + 1)),
     "log_weights must have shape [draws]"),
    ("inplay_summary", (H, A, [0, 0], [0, 0], [0.5, 0.5], G, W2), dict(log_weights=[[0.0] * S]),
     "log_weights must have shape [draws]"),
    ("slate_summary", (H, A, G, TABLES[:0], [0, 0], [0, 2]), {},
     "tables must have shape [L, max_goals+1, max_goals+1], L >= 1"),
    ("slate_summary", (H, A, G, TABLES[:, :2], [0, 0], [0, 2]), {},
     "tables must have shape [L, max_goals+1, max_goals+1], L >= 1"),
    ("slate_summary", (H, A, G, TABLES, [0], [0, 2]), {},
     "leg_table must have one index per fixture and start at least two entries"),
    ("slate_summary", (H, A, G, TABLES, [0, 0], [0]), {},
     "leg_table must have one index per fixture and start at least two entries"),
    ("team_ratings", ([0, 1], [2, 3], 0, G, (3, 1, 0)), dict(team_conf=[0]), "one confederation per team and per opponent"),
    ("team_ratings", ([0, 1], [2, 3], 0, G, (3, 1, 0)), dict(opponent_conf=[0, 1, 0]),
     "one confederation per team and per opponent"),
    ("team_ratings", ([0, 1], [2, 3], 0, G, (3, 1)), {}, "points must be (win, draw, loss)"),
]


@pytest.mark.parametrize("method,args,kw,message", REFUSED, ids=[f"{r[0]}_{i}" for i, r in enumerate(REFUSED)])
def test_shape_faults_raise_before_any_call(method, args, kw, message):
    ctx = _hollow_context()
    with pytest.raises(ValueError, match="^" + re.escape(message) + "$"):
        getattr(ctx, method)(*args, **kw)
    assert ctx._lib.calls == []
    ctx._h = None


def test_max_goals_beyond_the_grid_is_left_to_the_library():
    """The weights' shape is compared only for a max_goals the library takes (0..63, period 0..31)."""
    ctx = _hollow_context()
    ctx.market_summary(H, A, 64, W2)
    ctx.inplay_summary(H, A, [0, 0], [0, 0], [0.5, 0.5], -1, W2)
    ctx.period_summary(H, A, [0.5, 0.5], 32, W2)
    ctx.slate_summary(H, A, 64, TABLES, [0, 0], [0, 2])
    assert [(c[0], c[2]["max_goals"]) for c in ctx._lib.calls] == [
        ("bplhip_market_summary", 64), ("bplhip_inplay_summary", -1), ("bplhip_period_summary", 32),
        ("bplhip_slate_summary", 64)]
    ctx._h = None


@pytest.mark.parametrize("leg_table,start,P", [([0, 1, 5], [0, 2, 3], 0), ([0, 1, -1], [0, 2, 3], 0),
                                               ([0, 1, 1], [0, 2, 9], 4), ([0, 1, 1], [-4, 2, 3], 4),
                                               ([1, 1, 1], [0, 3], 9)],
                         ids=["leg_table_beyond", "leg_table_negative", "start_beyond", "start_negative", "one_slate"])
def test_slate_sizes_for_calls_the_library_refuses(leg_table, start, P):
    """P as slate_summary derives it for the outputs: 0 with a leg table index out of range, `start` clipped to
    0..m; K = 2 (P + 1) + 2."""
    ctx = _hollow_context()
    tables = np.zeros((2, G + 1, G + 1), dtype=np.uint8)
    tables[0, 1, 0], tables[1, 2, 2] = 1, 3
    out = ctx.slate_summary([0, 2, 1], [1, 3, 0], G, tables, leg_table, start, quantiles=(0.5,), return_draws=True)
    J, KS = len(start) - 1, 2 * (P + 1) + 2
    assert ctx._lib.calls[0][2]["n_slates"] == J
    assert out["mean"].shape == out["sd"].shape == (KS, J) and out["quantile"].shape == (KS, 1, J)
    assert out["draws"].shape == (S, J, P + 1) and out["leg_proba"].shape == (3, 8)
    ctx._h = None
