"""tournament_points without a GPU: bpl.group_points.from_counts on hand-written integers (NaN placement,
points_needed, quantiles with -1 for a missing place, rest_points_needed, cut_line), the new argument checks (all before
any device call), the result through a stand-in device in the manner of tests/test_tournament_scenarios_host.py's
ScenariosCtx, and the new symbol's declaration and call."""
import ctypes
import os
import re

import numpy as np
import pytest

import tournament_points_ref as G
import tournament_ref as R
from bpl import (NeutralDixonColesMatchPredictor, NeutralDixonColesMatchPredictorWC, _ffi, group_points)
from bpl.base import _prng_key, points_from_counts
from fake_ctx import FakePredictCtx
from test_paths_host import _cpu_case
from test_tournament_host import conf_of, hand_posterior

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 400


class PointsCtx(FakePredictCtx):
    """TEST-ONLY stand-in for HipContext.tournament_points: records the call and answers with the restatement's
    records (tests/tournament_points_ref.py) cross-tabulated into the raw tables the device returns."""

    def __init__(self, model, inp, seed):
        self.model, self.inp, self.seed, self.calls = model, inp, seed, []

    def tournament_points(self, team_idx, bracket, n_sims, key, points_min=0, n_bins=1, gd_cap=3, **kwargs):
        self.calls.append(dict(kwargs, team_idx=team_idx, bracket=bracket, n_sims=n_sims, key=key,
                               points_min=points_min, n_bins=n_bins, gd_cap=gd_cap))
        inp = self.inp
        assert tuple(key) == tuple(_prng_key(self.seed)) and n_sims == inp["num_simulations"]
        rec = G.simulate(R.model_tables(self.model), inp, key, head_to_head=kwargs.get("head_to_head", False))
        c = G.counts(rec, inp, points_min, n_bins, gd_cap)
        names = {"team_points_count": "team_points", "team_target_count": "team_target", "team_place_count": "team_place",
                 "place_points_count": "place_points", "place_gap_count": "place_gap", "rest_count": "rest_count",
                 "rest_through_count": "rest_through", "rest_rank_count": "rest_rank"}
        raw = {names[k]: v.astype(np.uint64) for k, v in c.items()}
        self.records = rec
        return raw


def _raises(m, *args, **kwargs):
    with pytest.raises(ValueError):
        m.tournament_points(*args, **kwargs)
    assert m._predict_ctx is None   # no device context was ever made


def test_new_argument_errors_come_before_the_device():
    m = hand_posterior()
    t = list(m.teams)
    euro = R.euro_24(t)
    groups, ko = euro["groups"], euro["knockout"]
    kw = dict(groups=groups, advance=2, best_of_rest=4, num_simulations=10)
    # no groups: no group points
    _raises(m, t[:4])
    _raises(m, t[:4], num_simulations=10, gd_cap=1)
    # gd_cap
    for bad in (True, False, 1.0, 9, -1, "3", None, [3]):
        _raises(m, ko, gd_cap=bad, **kw)
    # levels
    for bad in ((), [0.0], [1.5], [0.5, -0.1], "x", None, 0.5, [float("nan")]):
        _raises(m, ko, levels=bad, **kw)
    # an axis over 256 bins: a win is worth 100 points, three matches each
    _raises(m, ko, points=(100, 1, 0), **kw)
    _raises(m, ko, current_table={"t00": (300, 0, 0)}, **kw)
    # simulate_tournament's own errors, through the same code
    _raises(m, ko, groups=groups, advance=2, best_of_rest=2, num_simulations=10)
    _raises(m, ko, tiebreak="coin", **kw)
    _raises(m, ko, legs=2, **kw)
    _raises(m, ko, team_conf=conf_of(m), **kw)
    w = hand_posterior(NeutralDixonColesMatchPredictorWC)
    _raises(w, ko, **kw)                                                       # the World-Cup class needs team_conf
    # 256 bins themselves pass every check (3 x 85 = 255), as do gd_cap 0 and 8: the call reaches the device
    inp = m._tournament_inputs(ko, groups, 2, 4, None, None, None, (85, 1, 0), 10, None)
    for cap in (0, 8):
        m._predict_ctx = ctx = PointsCtx(m, inp, 1)
        m._uploaded = None
        res = m.tournament_points(ko, points=(85, 1, 0), random_state=1, gd_cap=cap, **kw)
        assert ctx.calls[0]["n_bins"] == 256 and ctx.calls[0]["points_min"] == 0 and ctx.calls[0]["gd_cap"] == cap
        assert res["points"].shape == (256,) and res["rest_count"].shape == (256, 2 * cap + 1)
        m._predict_ctx = None


def test_the_method_is_on_both_neutral_classes():
    assert callable(NeutralDixonColesMatchPredictor.tournament_points)
    assert NeutralDixonColesMatchPredictorWC.tournament_points is NeutralDixonColesMatchPredictor.tournament_points
    import bpl
    assert "group_points" in bpl.__all__ and bpl.group_points is group_points


# ---- from_counts on hand-written integers: n = 2 slots, P = 4 bins from 3 points up, K = 3 targets (R = 1), Gn = 2
# groups with Z = 2 places of which group 1 lacks place 1, N = 10 (arithmetic only: the tables need not be one tournament's)
TP = np.array([[0, 4, 6, 0], [5, 0, 0, 5]])
TT = np.zeros((2, 4, 3), dtype=np.int64)
TT[0, 1], TT[0, 2] = [1, 0, 4], [6, 3, 0]
TT[1, 0], TT[1, 3] = [0, 0, 5], [5, 5, 0]
TZ = np.zeros((2, 4, 2), dtype=np.int64)
TZ[0, 1], TZ[0, 2], TZ[1, 0], TZ[1, 3] = [1, 3], [6, 0], [0, 5], [5, 0]
PP = np.array([[[0, 0, 5, 5], [5, 5, 0, 0]], [[1, 2, 3, 4], [0, 0, 0, 0]]])     # group 1 has no place 1
GAP = np.array([[[2, 3, 5, 0]], [[0, 0, 0, 0]]])
# B = 2 ranks, D = 3: the best of the rest, then the other one; pooled, and those that went through (best_of_rest = 1)
RR = np.array([[[0, 0, 0], [1, 0, 0], [0, 3, 1], [0, 5, 0]], [[0, 2, 0], [3, 0, 0], [0, 5, 0], [0, 0, 0]]])
RC, RT = RR.sum(axis=0), RR[0]
LEVELS = (0.5, 0.9, 1.0)


@pytest.fixture(scope="module")
def hand():
    return group_points.from_counts(TP, TT, TZ, PP, GAP, 3, 10, LEVELS, RC, RT, RR, best_of_rest=1)


def test_from_counts_team_tables_are_points_needed_s(hand):
    base = points_from_counts(TP, TT, PP.reshape(4, 4), GAP.reshape(2, 4), 3, 10, np.array(LEVELS))
    for k in ("points", "levels", "team_points_count", "team_points_proba", "team_target_count", "target_count",
              "target_proba", "proba_given_points", "se_given_points", "proba_given_at_least", "points_needed"):
        assert hand[k].dtype == base[k].dtype, k
        np.testing.assert_array_equal(hand[k], base[k], err_msg=k)
    np.testing.assert_array_equal(hand["points"], [3, 4, 5, 6])
    # NaN exactly where the team never ended on / never reached the bin
    np.testing.assert_array_equal(np.isnan(hand["proba_given_points"][:, :, 0]), TP == 0)
    np.testing.assert_array_equal(np.isnan(hand["se_given_points"][:, :, 0]), TP == 0)
    np.testing.assert_array_equal(np.isnan(hand["proba_given_at_least"][:, :, 0]), [[False] * 3 + [True], [False] * 4])
    np.testing.assert_array_equal(np.isnan(hand["place_given_points"][:, :, 0]), TP == 0)
    # slot 0, target 0: P(inside | >= 3) = 7 / 10, >= 4 the same, >= 5 = 6 / 6; never reached 6
    np.testing.assert_array_equal(hand["proba_given_at_least"][0, :3, 0], [0.7, 0.7, 1.0])
    np.testing.assert_array_equal(hand["points_needed"][0, 0], [3.0, 5.0, 5.0])
    # slot 0, target 2 is never reached with certainty: 4 / 10, 4 / 10, 0 / 6
    np.testing.assert_array_equal(hand["points_needed"][0, 2], [np.nan] * 3)
    # slot 1, target 1: 5 / 10 at >= 3, then 5 / 5 from 4 on (bins nobody ended on count: "at least")
    np.testing.assert_array_equal(hand["points_needed"][1, 1], [3.0, 4.0, 4.0])
    np.testing.assert_array_equal(hand["round_proba"], hand["target_count"][:, :2] / 10)
    np.testing.assert_array_equal(hand["group_position_proba"], [[0.7, 0.3], [0.5, 0.5]])
    np.testing.assert_array_equal(hand["place_given_points"][0, 1], [0.25, 0.75])


def test_from_counts_places_quantiles_and_missing_places(hand):
    assert hand["place_points_quantile"].dtype == np.int64 and hand["place_points_quantile"].shape == (3, 2, 2)
    # group 0 place 0: 5 and 6 points, five times each; place 1: 3 and 4; group 1 place 0: 3 x1, 4 x2, 5 x3, 6 x4
    np.testing.assert_array_equal(hand["place_points_quantile"][:, 0, 0], [5, 6, 6])
    np.testing.assert_array_equal(hand["place_points_quantile"][:, 0, 1], [3, 4, 4])
    np.testing.assert_array_equal(hand["place_points_quantile"][:, 1, 0], [5, 6, 6])
    np.testing.assert_array_equal(hand["place_points_quantile"][:, 1, 1], [-1, -1, -1])
    np.testing.assert_array_equal(hand["place_points_mean"], [[5.5, 3.5], [5.0, np.nan]])
    np.testing.assert_array_equal(hand["level_proba"], [[0.2], [0.0]])
    assert hand["place_gap_count"].dtype == np.int64 and hand["place_points_count"].dtype == np.int64


def test_from_counts_rest_tables_and_the_cut_line(hand):
    np.testing.assert_array_equal(hand["goal_difference"], [-1, 0, 1])
    want = np.array([[np.nan, 0.0, np.nan], [0.25, np.nan, np.nan], [np.nan, 0.375, 1.0], [np.nan, 1.0, np.nan]])
    np.testing.assert_array_equal(hand["rest_proba"], want)
    # pooled over the goal difference: through / had, at least p: 10 / 20, 10 / 18, 9 / 14, 5 / 5
    np.testing.assert_array_equal(hand["rest_proba_given_at_least"], [0.5, 10 / 18, 9 / 14, 1.0])
    np.testing.assert_array_equal(hand["rest_points_needed"], [3.0, 6.0, 6.0])
    np.testing.assert_array_equal(hand["cut_points_proba"], [0.0, 0.1, 0.4, 0.5])
    np.testing.assert_array_equal(hand["cut_proba"], RR[0] / 10)
    assert group_points.cut_line(hand) == (6, 0, 0.5)
    # a level nothing reaches: NaN, as in points_needed
    none = group_points.from_counts(TP, TT, TZ, PP, GAP, 3, 10, [1.0], RC, RT * 0, RR, best_of_rest=1)
    np.testing.assert_array_equal(none["rest_points_needed"], [np.nan])
    # without a best of the rest the rest keys are absent, and cut_line has nothing to say
    bare = group_points.from_counts(TP, TT, TZ, PP, GAP, 3, 10, LEVELS)
    assert not [k for k in bare if k.startswith(("rest", "cut", "goal"))] and group_points.cut_line(bare) is None
    with pytest.raises(ValueError):
        group_points.from_counts(TP, TT, TZ, PP, GAP, 3, 10, [])


# ---- the public call through a stand-in device
@pytest.fixture(scope="module")
def case():
    # 3 groups of 4, the two best thirds, R = 3; t01 is a host, listed second in fixture 0 (t00 v t01)
    m, kw, inp = _cpu_case(hosts=["t01"])
    m._predict_ctx = ctx = PointsCtx(m, inp, 5)
    m._uploaded = None
    res = m.tournament_points(num_simulations=N, random_state=5, hosts=["t01"], gd_cap=2, levels=(0.5, 0.9), **kw)
    m._predict_ctx = None
    return m, kw, inp, res, ctx


def test_keys_shapes_and_the_device_call(case):
    m, kw, inp, res, ctx = case
    call = ctx.calls[0]
    assert call["advance"] == 2 and call["best_of_rest"] == 2 and (call["points_min"], call["n_bins"], call["gd_cap"]) == (0, 10, 2)
    np.testing.assert_array_equal(call["fix_p"], inp["fix_p"])
    n, Rr, P_, Z, Gn, B, D, L = 12, 3, 10, 4, 3, 3, 5, 2
    K = Rr + 2
    shapes = {"teams": (n,), "groups": (Gn,), "targets": (K,), "points": (P_,), "levels": (L,), "goal_difference": (D,),
              "team_points_count": (n, P_), "team_points_proba": (n, P_), "team_target_count": (n, P_, K),
              "target_count": (n, K), "target_proba": (n, K), "round_proba": (n, Rr + 1),
              "team_place_count": (n, P_, Z), "group_position_proba": (n, Z), "proba_given_points": (n, P_, K),
              "se_given_points": (n, P_, K), "proba_given_at_least": (n, P_, K), "points_needed": (n, K, L),
              "place_given_points": (n, P_, Z), "place_points_count": (Gn, Z, P_), "place_points_mean": (Gn, Z),
              "place_points_quantile": (L, Gn, Z), "place_gap_count": (Gn, Z - 1, P_), "level_proba": (Gn, Z - 1),
              "rest_count": (P_, D), "rest_through_count": (P_, D), "rest_rank_count": (B, P_, D), "rest_proba": (P_, D),
              "rest_proba_given_at_least": (P_,), "rest_points_needed": (L,), "cut_points_proba": (P_,),
              "cut_proba": (P_, D)}
    assert {k: np.shape(v) for k, v in res.items()} == shapes
    assert list(res["targets"]) == ["round_0", "round_1", "round_2", "winner", "group_winner"]
    assert list(res["teams"]) == list(inp["teams"]) and list(res["groups"]) == ["A", "B", "C"]
    for k in res:
        if k.endswith("_count") or k in ("points", "goal_difference", "place_points_quantile"):
            assert res[k].dtype == np.int64, k
    # the sums
    assert (res["team_points_count"].sum(axis=1) == N).all() and res["rest_count"].sum() == 3 * N
    assert res["rest_through_count"].sum() == 2 * N and (res["rest_rank_count"].sum(axis=(1, 2)) == N).all()
    np.testing.assert_array_equal(res["rest_rank_count"].sum(axis=0), res["rest_count"])
    # against the records
    rec = ctx.records
    stage, pos, pts = rec["stage"], rec["position"], rec["points"]
    np.testing.assert_array_equal(res["round_proba"], (stage[:, :, None] >= np.arange(1, Rr + 2)).sum(axis=0) / N)
    np.testing.assert_array_equal(res["group_position_proba"], (pos[:, :, None] == np.arange(Z)).sum(axis=0) / N)
    np.testing.assert_array_equal(res["team_points_count"][3], np.bincount(pts[:, 3], minlength=P_))
    np.testing.assert_array_equal(res["level_proba"], res["place_gap_count"][..., 0] / N)
    text = group_points.format_table(res, "t01")
    assert text.splitlines()[0] == "t01" and "most likely last qualifier" in text
    with pytest.raises(ValueError):
        group_points.format_table(res, "nobody")


def test_an_empty_fixture_list_with_a_table_is_allowed():
    m = hand_posterior(T=8, S=4, seed=3)
    kw = {"groups": {"A": list(m.teams[:4]), "B": list(m.teams[4:])}, "advance": 2,
          "knockout": [("A", 1), ("B", 2), ("B", 1), ("A", 2)], "group_fixtures": [],
          "current_table": {t: (3 * (i % 4), i % 4, 0) for i, t in enumerate(m.teams)}}
    inp = m._tournament_inputs(kw["knockout"], kw["groups"], 2, 0, [], kw["current_table"], None, (3, 1, 0), 50, None)
    m._predict_ctx = ctx = PointsCtx(m, inp, 2)
    m._uploaded = None
    res = m.tournament_points(num_simulations=50, random_state=2, **kw)
    m._predict_ctx = None
    assert ctx.calls[0]["n_bins"] == 10 and len(ctx.calls[0]["fix_p"]) == 0
    assert (res["team_points_count"].max(axis=1) == 50).all() and "rest_count" not in res
    np.testing.assert_array_equal(res["place_points_mean"], [[9.0, 6.0, 3.0, 0.0]] * 2)


# ---- the symbol and the call
class _Lib:
    """Records the arguments HipContext.tournament_points hands to the library."""

    def __init__(self):
        self.args = None

    def bplhip_tournament_points(self, *args):
        self.args = args
        return 0


class _Cuda:
    class device:
        def __init__(self, *_):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *_):
            return False


class _Torch:
    cuda = _Cuda


def _bare_context():
    ctx = _ffi.HipContext.__new__(_ffi.HipContext)
    ctx._lib, ctx._h, ctx._torch, ctx.device = _Lib(), 1, _Torch, 0
    ctx._stream = lambda: None
    ctx._check = lambda code: None
    return ctx


def test_the_call_passes_what_the_signature_declares():
    _, argtypes = _ffi._SIGNATURES["bplhip_tournament_points"]
    grp = dict(team_idx=[0, 1, 2, 3, 4, 5], team_group=[0, 0, 0, 1, 1, 1], bracket=[0x0001, 0x0101, 0x0002, 0xFF01],
               n_sims=10, key=(0, 1), fix_p=[0, 3], fix_q=[1, 4], advance=2, points_min=0, n_bins=4)
    for best in (0, 1):
        ctx = _bare_context()
        out = ctx.tournament_points(best_of_rest=best, **grp)
        args = ctx._lib.args
        assert len(args) == len(argtypes) == 44
        # the rest pointers are NULL exactly when there is no best of the rest
        assert all(a is not None for a in args[36:41])
        assert [a is None for a in args[41:]] == [best == 0] * 3
        assert ("rest_rank" in out) == (best > 0)
        if best:
            assert out["rest_rank"].shape == (2, 4, 7) and out["rest_count"].shape == (4, 7)
        assert out["team_target"].shape == (6, 4, 4) and out["place_gap"].shape == (2, 2, 4)
        assert args[32:36] == (0, 0, 4, 3)                      # chunk_sims, points_min, n_bins, gd_cap
    ctx = _bare_context()
    ctx.tournament_points(chunk_sims=7, gd_cap=0, **grp)
    assert ctx._lib.args[32] == 7 and ctx._lib.args[35] == 0


def test_header_declares_the_new_symbol():
    header = open(os.path.join(ROOT, "include", "bplhip.h")).read()
    declared = set(re.findall(r"\b(bplhip_[a-z_0-9]+)\s*\(", header)) - {"bplhip_ctx"}
    assert "bplhip_tournament_points" in declared and declared == set(_ffi.ABI_SYMBOLS)
    decl = re.search(r"int bplhip_tournament_points\((.*?)\);", header, re.S).group(1)
    params = [p.strip() for p in decl.split(",")]
    restype, argtypes = _ffi._SIGNATURES["bplhip_tournament_points"]
    assert restype is ctypes.c_int and len(params) == len(argtypes) == 44
    assert [a is _ffi._vp for a in argtypes] == ["*" in p for p in params]
    base = re.search(r"int bplhip_tournament_scenarios\((.*?)\);", header, re.S).group(1)
    theirs = [p.strip().split()[-1].lstrip("*") for p in base.split(",")]
    ours = [p.split()[-1].lstrip("*") for p in params]
    assert theirs[32] == "chunk_sims" and ours[:33] == theirs[:33]
    assert ours[33:] == ["points_min", "n_bins", "gd_cap", "team_points", "team_target", "team_place", "place_points",
                         "place_gap", "rest_count", "rest_through", "rest_rank"]
    assert int(re.search(r"#define BPLHIP_GROUP_POINTS_MAX_BINS (\d+)", header).group(1)) == 256 == group_points.MAX_BINS
    assert int(re.search(r"#define BPLHIP_GROUP_POINTS_MAX_GD_CAP (\d+)", header).group(1)) == 8 == group_points.GD_CAP_MAX
    assert (_ffi.GROUP_POINTS_MAX_BINS, _ffi.GROUP_POINTS_MAX_GD_CAP) == (256, 8)
    assert _ffi.load_library().bplhip_tournament_points is not None
    assert int(re.search(r"#define BPLHIP_ABI_VERSION (\d+)", header).group(1)) == 2 == _ffi.ABI_VERSION
