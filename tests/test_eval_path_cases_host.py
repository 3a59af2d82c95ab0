"""CPU: every case of tests/eval_path_cases.py still has the facts it was built for, so that none drifts off
the kernel form (and the edge inside it) that tests/test_gpu_eval_paths.py runs it for."""
import numpy as np
import pytest

import dc_neutral_oracle as NO
import eval_path_cases as E

NEUTRAL = {c.name: c for c in E.neutral_cases()}
DYNAMIC = {c.name: c for c in E.dynamic_cases()}


def test_constants_come_from_the_headers():
    # (orders of magnitude only: the values themselves are the headers' business)
    assert E.NEU_RUNS_MAX >= 8 and E.NEU_RUN_W >= 9 and E.NEU_BIG_BLOCK % 64 == 0
    assert E.FUSED_MAX_N >= 1024 and E.GATHER_MAX_INCIDENT >= 4 and E.LDS_LIMIT <= 160 * 1024
    assert E.P_N == 6 and E.A_N == 6   # (records and accumulators per team: big_lds_bytes restated with them)


def test_path_constants_match_the_header():
    import os
    import re

    from bpl import _ffi

    header = open(os.path.join(E.ROOT, "include", "bplhip.h")).read()
    declared = dict(re.findall(r"BPLHIP_PATH_([A-Z_]+) = (\d+)", header))
    assert {k: int(v) for k, v in declared.items()} == {nm: getattr(_ffi, "PATH_" + nm) for nm in _ffi.PATH_NAMES}
    assert [getattr(_ffi, "PATH_" + nm) for nm in _ffi.PATH_NAMES] == list(range(len(_ffi.PATH_NAMES)))


@pytest.mark.parametrize("name", list(NEUTRAL))
def test_neutral_case_takes_the_form_it_was_built_for(name):
    c = NEUTRAL[name]
    f = c.facts
    assert c.fx.n > E.FUSED_MAX_N                     # (or neu_fused takes it)
    assert f["path"] == c.path
    assert 1 <= c.wgs <= 7 and f["nbig"] == c.wgs     # independent of the CU count
    if c.path == "NEU_BIG_RUNS":
        assert E.neutral_facts(c.fx, c.wgs, neu_runs=0)["path"] == "NEU_BIG_FIXTURE"
    assert E.neutral_facts(c.fx, c.wgs, fused_small=0)["path"] == "NEU_MULTI"
    # what the device is handed is what the oracle sees
    assert c.fx.home_goals.max() <= 255 and c.fx.weights.min() > 0 and (c.fx.home_idx != c.fx.away_idx).all()


@pytest.mark.parametrize("name", [n for n in NEUTRAL if n.startswith("runs_random")])
def test_runs_random(name):
    f = NEUTRAL[name].facts
    assert f["table_fits"] and f["accepted"] and f["max_runs"] <= 3


def test_capacity_is_pinned_from_both_sides():
    at, over = NEUTRAL["runs_at_capacity"].facts, NEUTRAL["runs_overflow"].facts
    for f in (at, over):
        assert f["cap"] == 2560 and f["table_fits"] and f["lds_fits"]
        assert (f["runs"].reshape(-1)[1:] <= 3).all()           # only wave 0 of workgroup 0 is full
    assert at["runs"][0, 0] == 15 and 2 * 15 + 1 <= E.NEU_RUNS_MAX and at["accepted"]
    assert over["runs"][0, 0] == 16 and 2 * 16 + 1 > E.NEU_RUNS_MAX and not over["accepted"]
    # a wave of the full table walks steps that straddle several runs
    assert at["max_heads"] >= 4


def test_heads_threshold():
    f = NEUTRAL["heads_8_and_9"].facts
    assert not f["accepted"] and f["lds_fits"] and {8, 9} <= f["heads_seen"] and f["max_heads"] == 9


def test_confederations_split_runs():
    c = NEUTRAL["runs_split_by_conf"]
    f = c.facts
    assert c.fx.n_conf == 2 and f["total_runs"] == 4 * 12 and f["accepted"] and f["nbig"] == 3
    _, rkey = E.neutral_sorted(c.fx)
    per_pair = [len(np.unique(rkey[(rkey >> 16) == p])) for p in np.unique(rkey >> 16)]
    assert per_pair == [4] * 12
    r = NEUTRAL["conf_random_per_fixture"].facts
    assert r["table_fits"] and not r["accepted"] and r["runs"].min() > 100


def test_cut_run():
    c = NEUTRAL["runs_cut_everywhere"]
    f = c.facts
    cap, last = f["cap"], int(f["n_mine"][-1])
    assert last % 8 != 0 and last % 64 != 0 and last != cap
    lo, hi = f["cut_lo"], f["cut_hi"]
    assert f["cut_contiguous"] and lo < cap < hi                # across a workgroup boundary
    per_wave = -(-cap // E.WAVES)
    assert any(lo < w * per_wave < min(hi, cap) for w in range(1, E.WAVES))            # and wave boundaries on
    assert any(lo < cap + w * per_wave < hi for w in range(1, E.WAVES))                # either side of it
    # its pair attains the largest rate product at every test point, and the upper bound binds
    nv, h, a = E.CUT_KEY
    for _, _, z in E.neutral_points(c):
        _, _, aux = NO.potential_and_grad(c.fx, z)
        eh = aux["attack"][h] - aux["defence"][a] + (1 - nv) * (aux["home_attack"][h] - aux["away_defence"][a])
        ea = aux["attack"][a] - aux["defence"][h] + (1 - nv) * (aux["away_attack"][a] - aux["home_defence"][h])
        assert aux["UB"] < 1.0 and abs(np.exp(eh + ea) * aux["UB"] - 1.0) < 1e-12


def test_low_classes():
    fx = NEUTRAL["low_classes"].fx

    def classes(key):
        i = (fx.neutral == key[0]) & (fx.home_idx == key[1]) & (fx.away_idx == key[2])
        x, y = fx.home_goals[i], fx.away_goals[i]
        low = (x <= 1) & (y <= 1)
        return set(zip(x[low].tolist(), y[low].tolist())), int(i.sum())
    assert classes(E.LOW_ALL)[0] == {(0, 0), (1, 0), (0, 1), (1, 1)}
    assert classes(E.LOW_NONE) == (set(), classes(E.LOW_NONE)[1]) and classes(E.LOW_NONE)[1] > 100
    assert classes(E.LOW_ONE)[0] == {(1, 0)} and classes(E.LOW_ONE)[1] > 100
    assert fx.home_goals.max() == 255 and fx.away_goals.max() == 255
    w32 = fx.weights.astype(np.float32)
    assert 0 < w32.min() <= 1e-6 and NEUTRAL["low_classes"].facts["accepted"]


def test_venues_and_idle_team():
    for name, nv in (("venues_all_neutral", 1), ("venues_all_home", 0)):
        fx = NEUTRAL[name].fx
        assert (fx.neutral == nv).all() and fx.n_teams == 5
        assert 4 not in set(fx.home_idx.tolist()) | set(fx.away_idx.tolist())
        assert NEUTRAL[name].facts["accepted"]


def test_many_pairs_lds_fallback_far_records():
    f = NEUTRAL["many_pairs"].facts
    assert f["table_fits"] and not f["accepted"] and f["runs"].min() > 100 and f["max_heads"] > 8
    f = NEUTRAL["lds_fallback"].facts
    assert f["cap"] == 9000 and not f["lds_fits"] and 4 * f["cap"] * 8 > E.LDS_LIMIT
    c = NEUTRAL["far_records"]
    assert c.fx.n_conf == 0 and (c.fx.neutral == 0).all() and c.facts["accepted"]
    for _, _, z in E.neutral_points(c):
        _, _, aux = NO.potential_and_grad(c.fx, z)
        rec = np.concatenate([aux["attack"] + aux["home_attack"], aux["attack"] + aux["away_attack"],
                              aux["defence"] + aux["home_defence"], aux["defence"] + aux["away_defence"]])
        assert np.abs(rec).min() > 300.0                        # the records the home venue uses
        assert 0.0 < -1.0 / aux["LB"] < 1e3 and aux["UB"] > 1e-6   # rates of order one: finite in the oracle


@pytest.mark.parametrize("name", list(DYNAMIC))
def test_dynamic_case_takes_the_form_it_was_built_for(name):
    c = DYNAMIC[name]
    fx, f = c.fx, c.facts
    assert c.wgs == 0 and f["path"] == c.path
    assert fx.n <= -(-fx.n_teams // 4) * 1024 and fx.n_gameweeks <= 64 and fx.n_teams <= 1024
    assert E.dynamic_facts(fx, dyn_gather=0)["path"] == "DYN_FUSED_ATOMICS"
    assert E.dynamic_facts(fx, fused_small=0)["path"] == "DYN_MULTI"


def test_gather_lists_histogram():
    c = DYNAMIC["gather_lists"]
    f, fx = c.facts, c.fx
    hist = f["histogram"]
    M = E.GATHER_MAX_INCIDENT
    assert M == 16 and len(hist) == M + 1 and hist[M] == 1 and f["longest"] == M and f["gather"]
    assert hist[0] >= fx.n_teams                                 # (at least the empty gameweek's cells)
    for lo in range(1, M + 1, 4):                                # 1-4, 5-8, 9-12, 13-16: first round, reload rounds
        assert hist[lo:lo + 4].sum() >= 1, lo
    g0, t0 = E.GATHER_CELL
    assert f["length"][g0 * fx.n_teams + t0] == M
    assert f["mixed_sides"] >= 10 and f["mixed_venues"] >= 10
    assert f["empty_gameweeks"] == [4]
    assert 0.3 < fx.neutral.mean() < 0.5 and (fx.home_idx != fx.away_idx).all()
    g = DYNAMIC["gather_17"]
    assert g.facts["longest"] == M + 1 and not g.facts["gather"] and g.fx.n == fx.n + 1
    assert g.facts["length"][g0 * fx.n_teams + t0] == M + 1
    c4 = DYNAMIC["config4"].facts
    assert c4["longest"] == 1 and c4["gather"]
