"""loo_scores / pit_histogram without a GPU: result keys, shapes and dtypes for each class through a stand-in
context whose `loo_scores` is the numpy restatement (tests/loo_scores_ref.py), `compare_scores` next to
forecast_scores, every argument check made on the host before a device context is touched, the PIT histogram by
hand, identities of the restatement itself, and the new C symbol's declaration."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import loglik_ref as LR
import loo_scores_ref as OR
import scores_ref as SR
from bpl import _ffi, compare_scores
from bpl.scoring import pit_histogram
from fake_ctx import FakePredictCtx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ({"kind", "n", "outcome", "outcome_proba", "calibration", "outcome_proba_in_sample", "in_sample", "elpd_loo_i",
         "elpd_loo", "pareto_k", "ess", "tail_len", "reliable", "warning", "pit_home", "pit_away"}
        | {f"{name}{suffix}" for name in ("log_score", "brier", "rps") for suffix in ("", "_i", "_se")})


class FailCtx:
    """A device context that must never be touched."""

    def __getattr__(self, name):
        raise AssertionError(f"device call {name} before the host checks finished")


class LooCtx(FakePredictCtx):
    """FakePredictCtx plus `loo_scores` and `outcome_scores`, computed by the restatements from the uploaded posterior."""

    def __init__(self):
        self.calls = []

    def loo_scores(self, home_idx, away_idx, home_goals, away_goals, max_goals, r_eff=1.0, neutral=None, conf=None):
        h, a = np.asarray(home_idx, int), np.asarray(away_idx, int)
        self.calls.append(h.size)
        eh, ea = self._log_rates(h, a, neutral, conf)
        lh, la = np.exp(eh), np.exp(ea)
        ll = LR.ll_from_rates(lh, la, home_goals, away_goals, self.cc)
        return OR.device_part(ll, lh, la, self.cc, np.asarray(home_goals), np.asarray(away_goals), max_goals, r_eff)

    def outcome_scores(self, home_idx, away_idx, home_goals, away_goals, max_goals, neutral=None, conf=None):
        h, a = np.asarray(home_idx, int), np.asarray(away_idx, int)
        eh, ea = self._log_rates(h, a, neutral, conf)
        return SR.device_part(np.exp(eh), np.exp(ea), self.cc, home_goals, away_goals, max_goals)


@pytest.mark.parametrize("kind", LR.KINDS)
def test_result_keys_shapes_and_dtypes(kind):
    m = LR.hand_model(kind, S=40, T=6, seed=1)
    d = LR.hand_data(m, n=23, seed=2)
    m._predict_ctx = ctx = LooCtx()
    r = m.loo_scores(d, max_goals=7, bins=5)
    assert len(ctx.calls) == (len(np.unique(d["gameweek"])) if kind == "dynamic" else 1) and sum(ctx.calls) == 23
    assert set(r) == KEYS
    assert r["kind"] == "scores" and r["n"] == 23
    assert r["outcome"].dtype == np.uint8 and r["outcome"].shape == (23,)
    np.testing.assert_array_equal(r["outcome"], SR.outcome_of(d["home_goals"], d["away_goals"]))
    for k in ("outcome_proba", "outcome_proba_in_sample"):
        assert r[k].shape == (23, 3) and r[k].dtype == np.float64, k
    for k in ("pit_home", "pit_away"):
        assert r[k].shape == (23, 2) and r[k].dtype == np.float64, k
    for name in ("log_score", "brier", "rps"):
        assert r[f"{name}_i"].shape == (23,) and r[f"{name}_i"].dtype == np.float64
        assert isinstance(r[name], float) and isinstance(r[f"{name}_se"], float)
        assert isinstance(r["in_sample"][name], float)
    assert set(r["in_sample"]) == {"log_score", "brier", "rps"}
    for k in ("elpd_loo_i", "pareto_k", "ess"):
        assert r[k].shape == (23,) and r[k].dtype == np.float64, k
    assert r["tail_len"].shape == (23,) and r["tail_len"].dtype == np.int32
    assert r["reliable"].shape == (23,) and r["reliable"].dtype == np.bool_
    assert isinstance(r["elpd_loo"], float) and isinstance(r["warning"], bool)
    cal = r["calibration"]
    assert cal["bin_edges"].shape == (6,) and cal["count"].shape == (3, 5) and (cal["count"].sum(axis=1) == 23).all()
    # the host side scatters the groups back into fixture order and adds the rules: nothing else
    ref = OR.scores(m, d, 7)
    o = SR.outcome_of(d["home_goals"], d["away_goals"])
    for mine, theirs in (("outcome_proba", "proba"), ("outcome_proba_in_sample", "proba_in_sample"),
                         ("elpd_loo_i", "elpd_loo"), ("pareto_k", "pareto_k"), ("ess", "ess")):
        np.testing.assert_allclose(r[mine], ref[theirs], rtol=1e-12, atol=1e-14, err_msg=mine)
    np.testing.assert_array_equal(r["tail_len"], ref["tail_len"])
    np.testing.assert_allclose(r["pit_home"], ref["pit"][:, :2], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(r["pit_away"], ref["pit"][:, 2:], rtol=1e-12, atol=1e-14)
    log, brier, rps = SR.rules(ref["proba"], o)
    for name, want in (("log_score", log), ("brier", brier), ("rps", rps)):
        np.testing.assert_allclose(r[f"{name}_i"], want, rtol=1e-12, atol=1e-14, err_msg=name)
        assert abs(r[name] - want.mean()) < 1e-13
        assert abs(r[f"{name}_se"] - np.std(want, ddof=1) / math.sqrt(23)) < 1e-13
    for name, want in zip(("log_score", "brier", "rps"), SR.rules(ref["proba_in_sample"], o)):
        assert abs(r["in_sample"][name] - want.mean()) < 1e-13
    assert abs(r["elpd_loo"] - ref["elpd_loo"].sum()) < 1e-12
    np.testing.assert_array_equal(r["reliable"], ref["pareto_k"] <= 0.7)
    assert r["warning"] == bool((ref["pareto_k"] > 0.7).any())
    # S = 40 has a tail of 8 draws: the weights are smoothed and not uniform
    assert (r["tail_len"] > 4).all() and (r["ess"] < 40).all() and (r["ess"] >= 1).all()
    # leaving a match out costs skill on it: the in-sample log score is the better one
    assert r["in_sample"]["log_score"] > r["log_score"]


def test_k_threshold_moves_the_flags():
    m = LR.hand_model("basic", S=40, T=6, seed=1)
    d = LR.hand_data(m, n=12, seed=2)
    m._predict_ctx = LooCtx()
    k = m.loo_scores(d)["pareto_k"]
    low = m.loo_scores(d, k_threshold=float(k.min()) - 1.0)
    assert not low["reliable"].any() and low["warning"] is True
    high = m.loo_scores(d, k_threshold=float(k.max()))
    assert high["reliable"].all() and high["warning"] is False


@pytest.mark.parametrize("kind", LR.KINDS)
def test_compare_scores_takes_it_next_to_forecast_scores(kind):
    m = LR.hand_model(kind, S=20, T=6, seed=3)
    d = LR.hand_data(m, n=15, seed=4)
    m._predict_ctx = LooCtx()
    loo, fit = m.loo_scores(d, max_goals=9), m.forecast_scores(d, max_goals=9)
    np.testing.assert_allclose(loo["outcome_proba_in_sample"], fit["outcome_proba"], rtol=0, atol=1e-14)
    for rule in ("rps", "brier", "log_score"):
        out = compare_scores({"in_sample": fit, "loo": loo}, rule=rule)
        assert set(out) == {"in_sample", "loo"} and sorted(v["rank"] for v in out.values()) == [0, 1]
        assert out["loo"]["score"] == loo[rule] and out["in_sample"]["score"] == fit[rule]
        assert abs(loo["in_sample"][rule] - fit[rule]) < 1e-14


def _raises(m, data, **kwargs):
    m._predict_ctx = FailCtx()
    with pytest.raises(ValueError):
        m.loo_scores(data, **kwargs)


@pytest.mark.parametrize("kind", LR.KINDS)
def test_argument_checks_run_on_the_host(kind):
    m = LR.hand_model(kind, S=16)
    good = LR.hand_data(m, n=6)
    _raises(m, {k: [] for k in good})                       # no fixture
    for r in (None, 0, -1.0, math.inf, math.nan, "1", True):
        _raises(m, good, r_eff=r)
    for g in (-1, 64, 2.0, True, None, "15"):
        _raises(m, good, max_goals=g)
    for b in (0, 1001, -5, 10.0, True, None):
        _raises(m, good, bins=b)
    for t in (math.inf, -math.inf, math.nan, None, "0.7", True):
        _raises(m, good, k_threshold=t)
    _raises(m, dict(good, home_team=["nope"] + list(good["home_team"][1:])))
    _raises(m, dict(good, away_goals=list(good["away_goals"][:-1])))
    _raises(m, dict(good, home_goals=[256] + list(good["home_goals"][1:])))
    _raises(m, dict(good, away_goals=[-1] + list(good["away_goals"][1:])))
    d = dict(good)
    d.pop("home_goals")
    _raises(m, d)
    if kind in ("neutral", "wc", "dynamic"):
        _raises(m, dict(good, neutral_venue=[2] + list(good["neutral_venue"][1:])))
    if kind == "wc":
        _raises(m, dict(good, home_conf=["nope"] + list(good["home_conf"][1:])))


def test_draw_and_tail_limits_run_on_the_host():
    big = LR.hand_model("neutral", S=65537, T=2)
    _raises(big, LR.hand_data(big, n=2))
    wide = LR.hand_model("basic", S=6000, T=2)              # 0.2 S = 1200 draws in the tail at a small r_eff
    _raises(wide, LR.hand_data(wide, n=2), r_eff=0.01)


# ---- the PIT histogram
def test_pit_histogram_by_hand():
    # one fixture whose transform covers [0.2, 0.6]: bins [.2, .4) and [.4, .6) hold half each
    np.testing.assert_allclose(pit_histogram([[0.2, 0.6]], bins=5), [0.0, 0.5, 0.5, 0.0, 0.0], rtol=0, atol=1e-15)
    # a degenerate pair is a step at lower: all of it falls into the bin whose right edge first reaches it
    np.testing.assert_array_equal(pit_histogram([[0.35, 0.35]], bins=4), [0.0, 1.0, 0.0, 0.0])
    np.testing.assert_array_equal(pit_histogram([[0.5, 0.5]], bins=4), [0.0, 1.0, 0.0, 0.0])     # on an edge: u >= lower
    # the mean of the two above, with another width
    got = pit_histogram([[0.2, 0.6], [0.35, 0.35]], bins=5)
    np.testing.assert_allclose(got, [0.0, 0.25 + 0.5, 0.25, 0.0, 0.0], rtol=0, atol=1e-15)
    # one bin holds everything; the default is ten bins
    np.testing.assert_array_equal(pit_histogram([[0.1, 0.9], [0.0, 1.0]], bins=1), [1.0])
    h = pit_histogram([[0.0, 1.0]])
    assert h.shape == (10,) and h.dtype == np.float64
    np.testing.assert_allclose(h, np.full(10, 0.1), rtol=0, atol=1e-15)                         # uniform: flat


def test_pit_histogram_sums_to_one_and_checks_its_arguments():
    rs = np.random.RandomState(0)
    lower = rs.uniform(0.0, 0.9, 200)
    pit = np.stack([lower, lower + rs.uniform(0.0, 1.0, 200) * (1.0 - lower)], axis=1)
    pit[::17, 1] = pit[::17, 0]                              # some degenerate pairs, all with lower > 0
    pit[:, 0] = np.maximum(pit[:, 0], 1e-3)
    pit[:, 1] = np.maximum(pit[:, 1], pit[:, 0])
    for bins in (1, 7, 10, 1000):
        h = pit_histogram(pit, bins=bins)
        assert h.shape == (bins,) and (h >= 0).all() and abs(h.sum() - 1.0) < 1e-12
    # mass beyond the forecast grid is missing when an upper exceeds 1: never more than 1
    assert pit_histogram([[0.5, 1.5]], bins=2).sum() == 0.5
    for bad in ([0.2, 0.6], [[0.2, 0.6, 0.7]], np.zeros((0, 2)), [[0.6, 0.2]], [[0.1, math.nan]], [[-math.inf, 0.5]]):
        with pytest.raises(ValueError):
            pit_histogram(bad)
    for bins in (0, 1001, 2.0, True, None):
        with pytest.raises(ValueError):
            pit_histogram([[0.2, 0.6]], bins=bins)


# ---- identities of the restatement
@pytest.mark.parametrize("kind", LR.KINDS)
@pytest.mark.parametrize("S", [2, 10, 64, 100, 700])
def test_restatement_runs_for_every_class_without_nan(kind, S):
    tails = {2: 1, 10: 2, 64: 13, 100: 20, 700: 80}
    for spread in ("wide", "narrow"):
        m = LR.hand_model(kind, S=S, T=8, seed=5)
        if spread == "narrow":
            OR.narrow(m)
        d = LR.hand_data(m, n=8, seed=6)
        ref = OR.scores(m, d, 6)
        for k, v in ref.items():
            assert not np.isnan(v).any(), (spread, k)
        assert (ref["tail_len"] == tails[S]).all(), ref["tail_len"]
        assert (ref["pit"][:, 0] <= ref["pit"][:, 1]).all() and (ref["pit"][:, 2] <= ref["pit"][:, 3]).all()
        assert (ref["pit"] >= 0).all() and (ref["pit"] <= 1 + 1e-12).all()
        assert (ref["ess"] >= 1 - 1e-12).all() and (ref["ess"] <= S + 1e-9).all()
        if S >= 64:
            assert np.isfinite(ref["pareto_k"]).all()
            if spread == "narrow":
                assert np.median(ref["pareto_k"]) < 0.7, ref["pareto_k"]     # the regime loo calls reliable
        else:
            assert (ref["pareto_k"] == np.inf).all()        # a tail of at most 4 draws is not smoothed


def test_restatement_transform_telescopes_to_the_weighted_mass():
    G = 5
    m = LR.hand_model("neutral", S=64, T=6, seed=7)
    d = LR.hand_data(m, n=1, seed=8)
    lh, la = SR.rates(m, d)
    rho = np.asarray(m.corr_coef)
    total_h = total_a = 0.0
    for x in range(G + 1):                                   # a hypothetical score x - x for the same fixture
        dx = dict(d, home_goals=np.array([x]), away_goals=np.array([x]))
        ll = LR.ll_matrix(m, d)                              # (the weights of the actual result throughout)
        part = OR.device_part(ll, lh, la, rho, dx["home_goals"], dx["away_goals"], G)
        total_h += part["pit"][0, 1] - part["pit"][0, 0]
        total_a += part["pit"][0, 3] - part["pit"][0, 2]
    w = OR.weights(LR.ll_matrix(m, d)[:, 0])[0]
    mass = float(w @ SR.grid(lh, la, rho, G)[:, 0].sum(axis=(1, 2)))
    assert abs(total_h - mass) < 1e-14 and abs(total_a - mass) < 1e-14
    # a score above the grid: lower = upper = that mass; the outcome probabilities add up to it as well
    over = OR.device_part(LR.ll_matrix(m, d), lh, la, rho, np.array([G + 1]), np.array([200]), G)
    np.testing.assert_allclose(over["pit"][0], mass, rtol=0, atol=1e-14)
    assert abs(over["proba"][0].sum() - mass) < 1e-14


def test_restatement_identical_draws_give_uniform_weights():
    m = LR.hand_model("wc", S=1, T=6, seed=9)
    for name in ("attack", "defence", "home_attack", "away_attack", "home_defence", "away_defence",
                 "confederation_strength"):
        setattr(m, name, np.repeat(getattr(m, name), 64, axis=0))
    m.corr_coef = np.repeat(m.corr_coef, 64)
    d = LR.hand_data(m, n=5, seed=10)
    ref = OR.scores(m, d, 8)
    np.testing.assert_allclose(ref["ess"], 64.0, rtol=1e-12)
    np.testing.assert_allclose(ref["proba"], ref["proba_in_sample"], rtol=0, atol=1e-14)
    np.testing.assert_allclose(ref["elpd_loo"], LR.ll_matrix(m, d)[0], rtol=1e-12)


def test_restatement_takes_the_limit_at_a_clipped_tau():
    m = LR.hand_model("basic", S=20, T=4, seed=11)
    m.corr_coef = np.asarray(m.corr_coef).copy()
    m.corr_coef[::7] = 1.5                                   # draws 0, 7, 14: tau(1, 1) = 1 - rho < 0
    d = {"home_team": ["t00", "t01"], "away_team": ["t01", "t02"], "home_goals": [1, 2], "away_goals": [1, 2]}
    ref = OR.scores(m, d, 6)
    assert ref["elpd_loo"][0] == -np.inf and ref["pareto_k"][0] == np.inf and ref["tail_len"][0] == 0
    assert ref["ess"][0] == 3.0 and np.isfinite(ref["elpd_loo"][1])
    lh, la = SR.rates(m, d)
    p = SR.draw_probs(lh, la, np.asarray(m.corr_coef), 6)
    np.testing.assert_allclose(ref["proba"][0], p[::7, 0].mean(axis=0), rtol=0, atol=1e-15)
    assert all(np.isfinite(v).all() for k, v in ref.items() if k not in ("elpd_loo", "pareto_k"))


# ---- the C ABI
def test_the_new_symbol_is_declared_as_the_header_says():
    header = open(os.path.join(ROOT, "include", "bplhip.h")).read()
    decl = re.search(r"int bplhip_loo_scores\((.*?)\);", header, re.S).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    assert params == ["bplhip_ctx* ctx", "const bplhip_fixtures* q", "double r_eff", "int32_t max_goals",
                      "double* elpd_loo", "double* pareto_k", "int32_t* tail_len", "double* ess", "double* proba",
                      "double* proba_in_sample", "double* pit", "void* stream"]
    restype, argtypes = _ffi._SIGNATURES["bplhip_loo_scores"]
    assert restype is C.c_int and len(argtypes) == len(params)
    assert argtypes[1] is _ffi._SIGNATURES["bplhip_loglik_summary"][1][1]       # the fixtures record
    pointer = [a is C.c_void_p or a is argtypes[1] for a in argtypes]
    assert pointer == ["*" in p for p in params]
    scalar = {"double": C.c_double, "int32_t": C.c_int32}
    assert [a for a, p in zip(argtypes, params) if "*" not in p] == [scalar[p.split()[0]] for p in params if "*" not in p]
    assert "bplhip_loo_scores" in _ffi.ABI_SYMBOLS
    assert int(re.search(r"#define BPLHIP_ABI_VERSION (\d+)", header).group(1)) == 2 == _ffi.ABI_VERSION
    fn = _ffi.load_library().bplhip_loo_scores
    assert fn(None, None, 1.0, 15, *([None] * 8)) == -1      # EINVAL: no context, before anything touches a GPU
