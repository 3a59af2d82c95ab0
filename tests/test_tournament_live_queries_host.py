"""`in_play`, `reweight` and `log_weights` of tournament_paths, tournament_scenarios and tournament_points without a
GPU: every argument check (all made on the host before any device call, in simulate_tournament's words), the defaults
reaching the kick-off device methods, the restatement (tests/tournament_live_queries_ref.py) at kick-off states against
the kick-off restatements, and its flagged share on every case the GPU test compares tables against."""
import os
import re

import numpy as np
import pytest

import paths_ref as PR
import tournament_live_queries_cases as Q
import tournament_live_queries_ref as QR
import tournament_points_ref as TP
import tournament_ref as TR
import tournament_scenarios_ref as TS
from bpl import _ffi
from bpl.base import _prng_key, points_axis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ("tournament_paths", "tournament_scenarios", "tournament_points")


def _extra(method, name="A", kick_off=False):
    keys, caps = Q.KEYS[name]
    keys = (65, 1, 2) if kick_off else keys   # (positions inside the F = 66 fixtures of a kick-off call)
    return {"fixtures": keys, "margin_cap": caps} if method == "tournament_scenarios" else {}


def _raises(m, method, match, **kwargs):
    before = m._predict_ctx
    with pytest.raises(ValueError, match=match):
        getattr(m, method)(**kwargs)
    assert m._predict_ctx is before   # the call made no device context (without a GPU there is none at all)


@pytest.mark.parametrize("method", METHODS)
def test_argument_checks_run_on_the_host(method):
    m, kw, _, _ = Q.call("A", "overall-redraw")
    kw = dict(kw, **_extra(method))
    ip = kw["in_play"]
    _raises(m, method, "explicit group_fixtures", **dict(kw, group_fixtures=None))
    _raises(m, method, "must have home_team", **dict(kw, in_play={k: v for k, v in ip.items() if k != "elapsed"}))
    _raises(m, method, "same length", **dict(kw, in_play=dict(ip, elapsed=[0.1, 0.2])))
    _raises(m, method, "unknown team", **dict(kw, in_play=dict(ip, home_team=["nobody", "t00", "t05"])))
    _raises(m, method, "cannot play itself", **dict(kw, in_play=dict(ip, away_team=["t02", "t01", "t06"])))
    _raises(m, method, "two different teams of one group", **dict(kw, in_play=dict(ip, away_team=["t04", "t01", "t06"])))
    for bad in (64, -1, 1.5, True, float("nan")):
        _raises(m, method, "current goals must be integers", **dict(kw, in_play=dict(ip, home_goals=[0, 1, bad])))
    for bad in (1.0, -0.1, float("nan")):
        _raises(m, method, r"elapsed must be in \[0, 1\)", **dict(kw, in_play=dict(ip, elapsed=[0.0, 0.5, bad])))
    _raises(m, method, "elapsed = 0 with a score", **dict(kw, in_play=dict(ip, elapsed=[0.0, 0.0, 0.7])))
    _raises(m, method, "log_weights must have shape", **dict(kw, log_weights=np.zeros(299)))
    _raises(m, method, "log_weights must be finite", **dict(kw, log_weights=np.full(300, np.inf)))
    # F + L within the limit: simulate_tournament's for all three, tournament_paths' own 4096 before it
    limit = 1 << 20
    many = (kw["group_fixtures"] * (limit // 66 + 1))[:limit - 2]
    _raises(m, method, "group fixtures, those in play included", **dict(kw, group_fixtures=many))
    if method == "tournament_paths":
        _raises(m, method, "at most 4096 group fixtures, those in play included",
                **dict(kw, group_fixtures=(kw["group_fixtures"] * 63)[:4094]))
    # without groups: in_play is refused for all three, log_weights alone only by the two that need groups
    mc, kc, _, _ = Q.call("C", "overall-redraw", with_lw=True)
    kc = dict(kc, **_extra(method))
    _raises(mc, method, "in_play needs groups", **dict(kc, in_play=ip))
    if method == "tournament_scenarios":
        _raises(mc, method, "needs groups and at least one group fixture", **kc)
    if method == "tournament_points":
        _raises(mc, method, "needs groups", **kc)
    # a key beyond the concatenated list
    if method == "tournament_scenarios":
        _raises(m, method, "a key fixture must be an integer in 0..68", **dict(kw, fixtures=[69]))


class _Reached(Exception):
    pass


class StandInCtx:
    """TEST-ONLY stand-in for HipContext: records which device method a public call reaches and with which keywords,
    then stops the call."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def method(*args, **kwargs):
            self.calls.append((name, kwargs))
            raise _Reached(name)
        return method


@pytest.mark.parametrize("method", METHODS)
def test_defaults_reach_the_kick_off_device_methods(method):
    m, kw, inp, _ = Q.call("A", "h2h-extra_time")
    ctx = StandInCtx()
    m._device = lambda: ctx
    try:
        with pytest.raises(_Reached):
            getattr(m, method)(**Q.plain(kw), **_extra(method, kick_off=True))
        name, sent = ctx.calls[-1]
        assert name == method
        assert not {"in_play", "log_weights", "reweight", "live"} & set(sent)
        assert sent["fix_p"].size == 66
        # the same call with the three keywords spelled out at their defaults
        with pytest.raises(_Reached):
            getattr(m, method)(in_play=None, reweight=True, log_weights=None, **Q.plain(kw),
                               **_extra(method, kick_off=True))
        assert ctx.calls[-1][0] == method and set(ctx.calls[-1][1]) == set(sent)
        # live: the live device method, the fixtures still to kick off and the states apart
        with pytest.raises(_Reached):
            getattr(m, method)(**kw, **_extra(method))
        name, sent = ctx.calls[-1]
        assert name == method + "_live" and sent["fix_p"].size == 66 and sent["reweight"] is True
        np.testing.assert_array_equal(sent["in_play"][0], inp["in_play"][0])
        assert sent["log_weights"] is None
        if method == "tournament_points":
            # the axis is formed from the concatenated list's meetings
            cat = QR.shown(inp, inp["in_play"])
            assert (sent["points_min"], sent["n_bins"]) == points_axis(inp["table"][:, 0], cat["fix_p"], cat["fix_q"],
                                                                       inp["points"])
            assert sent["n_bins"] > [c for c in ctx.calls if c[0] == method][0][1]["n_bins"]
        # log_weights alone is live too
        with pytest.raises(_Reached):
            getattr(m, method)(**dict(kw, in_play=None, log_weights=np.zeros(300)), **_extra(method, kick_off=True))
        assert ctx.calls[-1][0] == method + "_live" and ctx.calls[-1][1]["in_play"][0].size == 0
    finally:
        del m._device


@pytest.mark.parametrize("mode_id", Q.MODE_IDS)
def test_kick_off_states_are_the_kick_off_restatements(mode_id):
    name = "A2"
    states, pairs = Q.kick_off(name)
    m, common, inp, dev = Q.call(name, mode_id, in_play=states, reweight=False)
    key, tables = _prng_key(Q.SEED), TR.model_tables(m)
    h2h, pair = common["tiebreak"] == "head_to_head", dev["kwargs"].get("pair_init")
    got = QR.simulate(tables, inp, key, inp["in_play"], False, None, h2h, pair)
    assert got["ess"] == 300.0 and np.isnan(got["log_evidence"])
    np.testing.assert_array_equal(got["draw"], np.arange(Q.N) % 300)
    plain = QR.shown(inp, inp["in_play"])
    assert plain["fix_p"].size == 66
    want = PR.simulate(tables, plain, key, head_to_head=h2h, pair_init=pair)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    keys, caps = Q.KEYS[name]
    ws = TS.simulate(tables, plain, key, keys, caps, head_to_head=h2h, pair_init=pair)
    np.testing.assert_array_equal(QR.scenario(got["margin"], keys, caps), ws["scenario"])
    np.testing.assert_array_equal(QR.target_set(got["stage"], got["position"], inp["rounds"]), ws["target_set"])
    wp = TP.simulate(tables, plain, key, head_to_head=h2h, pair_init=pair)
    for k, v in QR.points_records(got).items():
        np.testing.assert_array_equal(v, wp[k], err_msg=k)


@pytest.mark.parametrize("case", Q.REF_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_the_restatement_flags_at_most_one_percent(case):
    ref = Q.restatement(*case)
    print(f"{case}: flagged {int(ref['flagged'].sum())} of {Q.N}")
    assert ref["flagged"].mean() <= 0.01
    name = case[0]
    m, kw, _, _, ip, _ = Q.shape(name)
    L = len(ip["home_team"]) if ip else 0
    F = len(kw.get("group_fixtures", ()))
    assert ref["group_outcome"].shape == (Q.N, F + L) and ref["pair"].shape[0] == Q.N
    if L:
        # a match in play is classed by its final score in the listed order, never below the state
        margin = Q.listed_margin(ref)
        np.testing.assert_array_equal(ref["margin"][:, F:], margin)
        assert (ref["in_play_home_goals"] >= np.array(ip["home_goals"])).all()
        assert (ref["in_play_away_goals"] >= np.array(ip["away_goals"])).all()


def test_the_new_symbols_are_in_the_header_and_the_library():
    with open(os.path.join(ROOT, "include", "bplhip.h")) as f:
        header = f.read()
    lib = _ffi.load_library()
    for method in METHODS:
        sym = f"bplhip_{method}_live"
        assert len(re.findall(rf"^int {sym}\(", header, flags=re.M)) == 1
        assert sym in _ffi.ABI_SYMBOLS and getattr(lib, sym) is not None
        # the kick-off entry's argument list, then the live block
        kick, live = _ffi._SIGNATURES[f"bplhip_{method}"][1], _ffi._SIGNATURES[sym][1]
        tail = _ffi._live_request + ([] if method == "tournament_points" else [_ffi._vp] * 3)
        assert live == kick + tail
