"""simulate_tournament's `in_play`, `reweight` and `log_weights` without a GPU: every argument check (all made on the
host before any device call), the restatement (tests/tournament_live_ref.py) against the restatements it is composed
from, its flagged share on every case the GPU test compares, and the new symbol in the header and the library."""
import os
import re

import numpy as np
import pytest

import h2h_ref as H
import knockout_ref as K
import tournament_live_cases as C
import tournament_live_ref as TLR
import tournament_ref as TR
from bpl import _ffi
from bpl.base import _prng_key

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _raises(m, match, **kwargs):
    with pytest.raises(ValueError, match=match):
        m.simulate_tournament(**kwargs)
    assert m._predict_ctx is None   # no device context was ever made


def _public(name, **changes):
    m, common, _, _ = C.call(name, "overall-redraw")
    return m, dict(common, **changes)


def test_argument_checks_run_on_the_host():
    m, kw = _public("A")
    ip = kw["in_play"]
    # in_play needs groups and an explicit list of the matches still to kick off
    _raises(m, "explicit group_fixtures", **dict(kw, group_fixtures=None))
    mc, kc = _public("C")
    _raises(mc, "in_play needs groups", **dict(kc, in_play=ip))
    # the columns
    _raises(m, "must have home_team", **dict(kw, in_play={k: v for k, v in ip.items() if k != "elapsed"}))
    _raises(m, "same length", **dict(kw, in_play=dict(ip, elapsed=[0.1, 0.2])))
    _raises(m, "unknown team", **dict(kw, in_play=dict(ip, home_team=["nobody", "t00", "t05"])))
    _raises(m, "unknown team", **dict(kw, in_play=dict(ip, away_team=[3, "t01", "t06"])))
    _raises(m, "cannot play itself", **dict(kw, in_play=dict(ip, away_team=["t02", "t01", "t06"])))
    _raises(m, "two different teams of one group", **dict(kw, in_play=dict(ip, away_team=["t04", "t01", "t06"])))
    # the states
    for bad in (64, -1, 1.5, True, float("nan")):
        _raises(m, "current goals must be integers", **dict(kw, in_play=dict(ip, home_goals=[0, 1, bad])))
    for bad in (1.0, -0.1, float("nan")):
        _raises(m, r"elapsed must be in \[0, 1\)", **dict(kw, in_play=dict(ip, elapsed=[0.0, 0.5, bad])))
    _raises(m, "elapsed = 0 with a score", **dict(kw, in_play=dict(ip, elapsed=[0.0, 0.0, 0.7])))
    # F + L within the group-fixture limit
    limit = 1 << 20
    many = (kw["group_fixtures"] * (limit // 66 + 1))[:limit - 2]
    _raises(m, f"at most {limit} group fixtures", **dict(kw, group_fixtures=many))
    # the log weights
    _raises(m, "log_weights must have shape", **dict(kw, log_weights=np.zeros(299)))
    _raises(m, "log_weights must be finite", **dict(kw, log_weights=np.full(300, np.inf)))
    _raises(mc, "log_weights must have shape", **dict(kc, log_weights=np.zeros(3)))


def test_defaults_reach_the_kick_off_call():
    # with the four keywords at their defaults `_tournament_call` hands the device method what it handed it before
    m, kw, hosts, _, _, _ = C.shape("A")
    args = (kw["knockout"], kw["groups"], 2, 0, kw["group_fixtures"], None, hosts, (3, 1, 0), 10, 1, None, "overall", None,
            "redraw", None, 1 / 3, None, False)
    inp, dev = m._tournament_call(*args)
    assert "in_play" not in inp and "in_play" not in dev["kwargs"] and "log_weights" not in dev["kwargs"]
    _, live = m._tournament_call(*args, None, None, None, True)
    assert set(live["kwargs"]) == set(dev["kwargs"]) | {"in_play", "log_weights"}


@pytest.mark.parametrize("mode_id", C.MODE_IDS)
def test_kick_off_states_without_weights_are_the_concatenated_list(mode_id):
    states, pairs = C.kick_off("A")
    m, common, inp, dev = C.call("A", mode_id, in_play=states, reweight=False)
    key = _prng_key(C.SEED)
    h2h, pair = common["tiebreak"] == "head_to_head", dev["kwargs"].get("pair_init")
    got = TLR.simulate_tournament_live(TR.model_tables(m), inp, key, inp["in_play"], False, None, h2h, pair)
    assert got["weights"] is None and got["ess"] == 300.0 and np.isnan(got["log_evidence"])
    np.testing.assert_array_equal(got["draw"], np.arange(C.N) % 300)
    fixtures = list(C.shape("A")[1]["group_fixtures"]) + pairs
    _, _, plain, _ = C.call("A", mode_id, in_play=None)
    plain = dict(plain, fix_p=np.concatenate([inp["fix_p"], inp["in_play"][0]]),
                 fix_q=np.concatenate([inp["fix_q"], inp["in_play"][1]]))
    assert len(fixtures) == plain["fix_p"].size == 69
    tables = TR.model_tables(m)
    if inp["knockout_rule"] == "extra_time":
        want = K.simulate_tournament(tables, plain, key, h2h, pair)
    elif h2h:
        want = H.simulate_tournament(tables, plain, key, pair)
    else:
        want = TR.simulate_tournament(tables, plain, key)
    for k in ("stage", "position", "stage_counts", "position_counts", "flagged"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    if "decided" in want:
        np.testing.assert_array_equal(got["decided"], want["decided"])


@pytest.mark.parametrize("case", C.GPU_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_the_restatement_flags_at_most_one_percent(case):
    ref = C.restatement(*case)
    share = ref["flagged"].mean()
    print(f"{case}: flagged {int(ref['flagged'].sum())} of {C.N}")
    assert share <= 0.01
    name, _, _, with_lw = case
    L = len(C.shape(name)[4]["home_team"]) if C.shape(name)[4] else 0
    assert ref["weights"] is not None and ref["in_play_home_goals"].shape == (C.N, L)
    assert 1.0 <= ref["ess"] <= ref["L"].size and np.isfinite(ref["log_evidence"])
    if L == 0:
        np.testing.assert_array_equal(ref["L"], C.log_weights(name))


def test_a_host_listed_second_swaps_the_sides_and_the_goals():
    m, _, inp, _ = C.call("A", "overall-redraw")
    hs, as_, on, a, b, swap = TLR.oriented(inp, inp["in_play"])
    # (t02, t03) neutral, (t00, t01) at the host t01's venue, (t05, t06) neutral
    np.testing.assert_array_equal(swap, [False, True, False])
    np.testing.assert_array_equal(on, [False, True, False])
    np.testing.assert_array_equal(np.stack([hs, as_]), [[2, 1, 5], [3, 0, 6]])
    np.testing.assert_array_equal(np.stack([a, b]), [[0, 0, 2], [0, 1, 1]])
    # the final scores never fall below the state, in the listed order
    ref = C.restatement("A", "overall-redraw", False, False)
    assert (ref["in_play_home_goals"] >= np.array([0, 1, 2])).all() and (ref["in_play_away_goals"] >= np.array([0, 0, 1])).all()


def test_the_new_symbol_is_in_the_header_and_the_library():
    with open(os.path.join(ROOT, "include", "bplhip.h")) as f:
        header = f.read()
    assert len(re.findall(r"^int bplhip_simulate_tournament_live\(", header, flags=re.M)) == 1
    assert "bplhip_simulate_tournament_live" in _ffi.ABI_SYMBOLS
    lib = _ffi.load_library()
    assert getattr(lib, "bplhip_simulate_tournament_live") is not None
