"""tournament_scenarios without a GPU: the new argument checks (all before any device call), the result's keys, shapes
and floats through a stand-in device in the manner of tests/test_paths_host.py's PathsCtx, bpl.scenarios' helpers on
such a result, and the header's new symbol."""
import os
import re

import numpy as np
import pytest

import tournament_ref as R
import tournament_scenarios_ref as S
from bpl import NeutralDixonColesMatchPredictorWC, _ffi, scenarios
from bpl.base import _prng_key
from fake_ctx import FakePredictCtx
from test_paths_host import _cpu_case
from test_tournament_host import conf_of, hand_posterior

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 400


class ScenariosCtx(FakePredictCtx):
    """TEST-ONLY stand-in for HipContext.tournament_scenarios: records the call and answers with the restatement's
    records (tests/tournament_scenarios_ref.py) cross-tabulated into the raw tables the device returns."""

    def __init__(self, model, inp, seed):
        self.model, self.inp, self.seed, self.calls = model, inp, seed, []

    def tournament_scenarios(self, team_idx, bracket, n_sims, key, return_records=False, key_fixture=(), key_cap=(),
                             **kwargs):
        self.calls.append(dict(kwargs, team_idx=team_idx, bracket=bracket, n_sims=n_sims, key=key,
                               return_records=return_records, key_fixture=key_fixture, key_cap=key_cap))
        inp = self.inp
        assert tuple(key) == tuple(_prng_key(self.seed)) and n_sims == inp["num_simulations"]
        rec = S.simulate(R.model_tables(self.model), inp, key, key_fixture, key_cap,
                         head_to_head=kwargs.get("head_to_head", False))
        c = S.counts(rec, inp, key_fixture, key_cap)
        raw = {"scenario": c["scenario_count"].astype(np.uint64), "joint": c["joint_count"].astype(np.uint64)}
        if "decided" in rec:
            Rr = inp["rounds"]
            k0, dc = 0, np.zeros((Rr, 4), dtype=np.uint64)
            for r in range(Rr):
                M = (1 << Rr) >> (r + 1)
                dc[r] = np.bincount(rec["decided"][:, k0:k0 + M].ravel(), minlength=4)
                k0 += M
            raw["decided_counts"] = dc
        if return_records:
            raw["sim_scenario"], raw["sim_tset"] = rec["scenario"], rec["target_set"]
        self.records = rec
        return raw


def _raises(m, *args, **kwargs):
    with pytest.raises(ValueError):
        m.tournament_scenarios(*args, **kwargs)
    assert m._predict_ctx is None   # no device context was ever made


def test_new_argument_errors_come_before_the_device():
    m = hand_posterior()
    t = list(m.teams)
    euro = R.euro_24(t)
    groups, ko = euro["groups"], euro["knockout"]
    kw = dict(groups=groups, advance=2, best_of_rest=4, num_simulations=10)   # 6 groups of 4: 36 fixtures
    # nothing to key on: no groups; an empty group-fixture list
    _raises(m, t[:4], [0])
    _raises(m, t[:4], [0], num_simulations=10, margin_cap=1)
    _raises(m, ko, [0], group_fixtures=[], **kw)
    # positions
    for bad in ([], [36], [-1], [0, 0], [True], [1.0], [0.5], ["0"], 3, None, list(range(9))):
        _raises(m, ko, bad, **kw)
    _raises(m, ko, [2], group_fixtures=[("t00", "t01"), ("t02", "t03")], **kw)   # the given list has 2 fixtures
    # caps
    for bad in (0, 4, -1, True, 1.0, [1], [1, 2, 3], [1, 4], [1, None], "1"):
        _raises(m, ko, [0, 1], margin_cap=bad, **kw)
    # more than 6561 scenarios: 7^5 = 16807, 3^7 x 5 = 10935; 3^8 = 6561 itself is allowed (checked below)
    _raises(m, ko, [0, 1, 2, 3, 4], margin_cap=3, **kw)
    _raises(m, ko, list(range(8)), margin_cap=[1] * 7 + [2], **kw)
    # return_records
    for bad in (1, 0, "yes", None):
        _raises(m, ko, [0], return_records=bad, **kw)
    # simulate_tournament's own errors, through the same code
    _raises(m, ko, [0], groups=groups, advance=2, best_of_rest=2, num_simulations=10)
    _raises(m, ko, [0], tiebreak="coin", **kw)
    _raises(m, ko, [0], legs=2, **kw)
    _raises(m, ko, [0], team_conf=conf_of(m), **kw)
    w = hand_posterior(NeutralDixonColesMatchPredictorWC)
    _raises(w, ko, [0], **kw)                                                  # the World-Cup class needs team_conf
    # 3^8 scenarios pass every check: the call reaches the device
    inp = m._tournament_inputs(ko, groups, 2, 4, None, None, None, (3, 1, 0), 10, None)
    m._predict_ctx = ScenariosCtx(m, inp, 1)
    m._uploaded = None
    res = m.tournament_scenarios(ko, list(range(8)), random_state=1, **kw)
    assert res["scenario_count"].shape == (6561,) and res["scenario_count"].sum() == 10
    m._predict_ctx = None


def _run(m, kw, inp, keys, caps, seed=5, hosts=("t01",), **extra):
    m._predict_ctx = ctx = ScenariosCtx(m, inp, seed)
    m._uploaded = None
    res = m.tournament_scenarios(fixtures=keys, margin_cap=caps, num_simulations=N, random_state=seed,
                                 hosts=list(hosts), **kw, **extra)
    m._predict_ctx = None
    return res, ctx


@pytest.fixture(scope="module")
def case():
    # 3 groups of 4, the two best thirds, R = 3; t01 is a host, listed second in fixture 0 (t00 v t01)
    m, kw, inp = _cpu_case(hosts=["t01"])
    keys, caps = [0, 7, 17], [2, 1, 3]
    res, ctx = _run(m, kw, inp, keys, caps, return_records=True)
    return m, kw, inp, keys, caps, res, ctx


def test_keys_shapes_and_the_device_call(case):
    m, kw, inp, keys, caps, res, ctx = case
    call = ctx.calls[0]
    assert call["return_records"] is True and call["advance"] == 2 and call["best_of_rest"] == 2
    np.testing.assert_array_equal(call["key_fixture"], keys)
    np.testing.assert_array_equal(call["key_cap"], caps)
    np.testing.assert_array_equal(call["fix_p"], inp["fix_p"])
    n, Rr, k, M = 12, 3, 3, 5 * 3 * 7
    K = Rr + 2
    shapes = {"teams": (n,), "targets": (K,), "fixtures": (k,), "home": (k,), "away": (k,), "margin_cap": (k,),
              "margins": (M, k), "scenario_count": (M,), "scenario_proba": (M,), "joint_count": (M, n, K),
              "target_count": (n, K), "target_proba": (n, K), "conditional_proba": (M, n, K),
              "conditional_se": (M, n, K), "settled": (M, n, K), "leverage": (n, K), "round_proba": (n, Rr + 1),
              "scenario": (N,), "target_set": (N, n)}
    assert {k_: np.shape(v) for k_, v in res.items() if k_ != "shape"} == shapes
    assert res["shape"] == (5, 3, 7)
    assert list(res["targets"]) == ["round_0", "round_1", "round_2", "winner", "group_winner"]
    assert list(res["teams"]) == list(inp["teams"])
    # "home" / "away" read first- / second-listed, also for the host listed second
    fixtures = kw["group_fixtures"]
    assert list(res["home"]) == [fixtures[f][0] for f in keys] and list(res["away"]) == [fixtures[f][1] for f in keys]
    assert res["away"][0] == "t01"
    for name in ("scenario_count", "joint_count", "target_count", "fixtures", "margin_cap", "margins"):
        assert res[name].dtype == np.int64, name
    assert res["settled"].dtype == np.int8 and res["scenario"].dtype == np.uint32 and res["target_set"].dtype == np.uint8
    # without records, and under the extra-time rule
    rule = dict(knockout_rule="extra_time", legs=(2, 1, 1))
    _, _, inp_et = _cpu_case(rule, hosts=["t01"])
    bare, _ = _run(m, kw, inp_et, keys, caps, **rule)
    assert set(bare) == (set(res) - {"scenario", "target_set"}) | {"decided_proba"}
    assert bare["decided_proba"].shape == (Rr, 4)
    np.testing.assert_allclose(bare["decided_proba"].sum(axis=1), 1.0, atol=1e-12)


def test_floats_against_the_formulas(case):
    m, kw, inp, keys, caps, res, ctx = case
    rec = ctx.records
    sc, jc = res["scenario_count"], res["joint_count"]
    M, n, K = jc.shape
    Rr = inp["rounds"]
    # the tables are the records' cross-tabulation; the records are the restatement's
    np.testing.assert_array_equal(res["scenario"], rec["scenario"])
    np.testing.assert_array_equal(res["target_set"], rec["target_set"])
    for m_ in (0, 17, M - 1):
        hit = rec["scenario"] == m_
        assert sc[m_] == hit.sum()
        np.testing.assert_array_equal(jc[m_], ((rec["target_set"][hit][:, :, None] >> np.arange(K)) & 1).sum(axis=0))
    assert sc.sum() == N
    # the margins of a scenario are those of its simulations, in the listed orientation
    margin = S.key_margins(R.model_tables(m), inp, _prng_key(5), keys)
    np.testing.assert_array_equal(res["margins"][rec["scenario"]], np.clip(margin, -np.array(caps), np.array(caps)))
    # targets: stage and first place
    stage, pos = rec["stage"].astype(int), rec["position"].astype(int)
    for k in range(Rr + 1):
        np.testing.assert_array_equal(res["target_count"][:, k], (stage >= k + 1).sum(axis=0))
    np.testing.assert_array_equal(res["target_count"][:, Rr + 1], (pos == 0).sum(axis=0))
    assert res["target_count"][:, Rr + 1].sum() == 3 * N       # one winner per group
    # the floats, one operation per cell
    np.testing.assert_array_equal(res["scenario_proba"], sc / N)
    np.testing.assert_array_equal(res["target_count"], jc.sum(axis=0))
    np.testing.assert_array_equal(res["target_proba"], jc.sum(axis=0) / N)
    np.testing.assert_array_equal(res["round_proba"], jc.sum(axis=0)[:, :Rr + 1] / N)
    seen = sc > 0
    assert 1 < seen.sum() < M                                   # some scenarios never occurred
    assert np.isnan(res["conditional_proba"][~seen]).all() and np.isnan(res["conditional_se"][~seen]).all()
    assert not np.isnan(res["conditional_proba"][seen]).any()
    p = jc[seen] / sc[seen][:, None, None]
    np.testing.assert_array_equal(res["conditional_proba"][seen], p)
    np.testing.assert_array_equal(res["conditional_se"][seen], np.sqrt(p * (1.0 - p) / sc[seen][:, None, None]))
    want = np.zeros((M, n, K), dtype=np.int8)
    want[seen] =np.where(jc[seen] == sc[seen][:, None, None], 1, np.where(jc[seen] == 0, -1, 0))
    np.testing.assert_array_equal(res["settled"], want)
    assert (res["settled"][~seen] == 0).all()
    lev = np.zeros((n, K))
    for m_ in range(M):
        if sc[m_]:
            lev = lev + (sc[m_] / N) * np.abs(jc[m_] / sc[m_] - jc.sum(axis=0) / N)
    np.testing.assert_allclose(res["leverage"], lev, rtol=0, atol=1e-15)


def test_marginal_and_coarsen_equal_the_narrower_calls(case):
    m, kw, inp, keys, caps, res, _ = case
    tables = ("scenario_count", "joint_count", "target_count")
    same = tables + ("scenario_proba", "target_proba", "conditional_proba", "conditional_se", "settled", "leverage",
                     "margins", "fixtures", "home", "away", "margin_cap")
    for keep in ([1], [2, 0], [0, 1, 2]):
        narrow, _ = _run(m, kw, inp, [keys[q] for q in keep], [caps[q] for q in keep])
        got = scenarios.marginal(res, keep)
        assert got["shape"] == narrow["shape"]
        for name in same:
            np.testing.assert_array_equal(got[name], narrow[name], err_msg=f"{name} keep {keep}")
    for new in (1, [1, 1, 2], [2, 1, 3]):
        coarse, _ = _run(m, kw, inp, keys, new)
        got = scenarios.coarsen(res, new)
        assert got["shape"] == coarse["shape"]
        for name in same:
            np.testing.assert_array_equal(got[name], coarse[name], err_msg=f"{name} caps {new}")


def test_requirements_and_format_table_take_the_result(case):
    *_, res, _ = case
    for target in ("round_0", "group_winner"):
        rows = scenarios.requirements(res, "t00", target, level=1.0)
        assert rows.ndim == 2 and rows.shape[1] == 3
        t, k = list(res["teams"]).index("t00"), list(res["targets"]).index(target)
        np.testing.assert_array_equal(rows, res["margins"][res["settled"][:, t, k] == 1])
        text = scenarios.format_table(res, "t00", target)
        lines = text.splitlines()
        assert lines[0].startswith(f"t00: {target} ") and "t00 v t01" in lines[1]
        assert len(lines) == 2 + int((res["scenario_count"] > 0).sum())
    assert len(scenarios.requirements(res, "t00", "round_0", level=0.5)) >= len(
        scenarios.requirements(res, "t00", "round_0", level=1.0))
    with pytest.raises(ValueError):
        scenarios.requirements(res, "t00", "semi_final")


def test_header_declares_the_new_symbol():
    header = open(os.path.join(ROOT, "include", "bplhip.h")).read()
    declared = set(re.findall(r"\b(bplhip_[a-z_0-9]+)\s*\(", header)) - {"bplhip_ctx"}
    assert "bplhip_tournament_scenarios" in declared and declared == set(_ffi.ABI_SYMBOLS)
    decl = re.search(r"int bplhip_tournament_scenarios\((.*?)\);", header, re.S).group(1)
    params = [p.strip() for p in decl.split(",")]
    restype, argtypes = _ffi._SIGNATURES["bplhip_tournament_scenarios"]
    assert len(params) == len(argtypes) == 40
    assert [a is _ffi._vp for a in argtypes] == ["*" in p for p in params]
    base = re.search(r"int bplhip_simulate_tournament\((.*?)\);", header, re.S).group(1)
    theirs = [p.strip().split()[-1].lstrip("*") for p in base.split(",")]
    ours = [p.split()[-1].lstrip("*") for p in params]
    assert theirs[22] == "key_lo" and ours[:23] == theirs[:23]
    assert ours[23:] == ["stream", "pair_init", "head_to_head", "extra_time", "legs_mask", "extra_time_scale",
                         "away_goals", "strength", "decided_counts", "chunk_sims", "n_key", "key_fixture", "key_cap",
                         "scenario", "joint", "sim_scenario", "sim_tset"]
    assert _ffi.load_library().bplhip_tournament_scenarios is not None
    assert int(re.search(r"#define BPLHIP_ABI_VERSION (\d+)", header).group(1)) == 2 == _ffi.ABI_VERSION
