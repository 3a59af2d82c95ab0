"""tournament_points on the device (csrc/dc_group_points.hip.h): every integer table against the numpy restatement
(tests/tournament_points_ref.py) and against a cross-tabulation of tournament_paths' own records, in all four modes;
its identity with simulate_tournament and tournament_scenarios under one random_state; the independence of the chunk;
designed cases (deterministic groups, goal-difference clipping, unequal groups, a host listed second, the World-Cup
class, played matches under the head-to-head order); the sums; and the context and argument errors.  Every comparison
is exact: the tables are integers, and the floats come from one host function fed equal integers.

Every case's seed and shape were run through the restatement on the CPU first: it flags none of their simulations
(a flag marks a comparison within 1e-12 of its boundary, where exp's last bit could change a scoreline), and the tests
assert that before they compare."""
import functools

import numpy as np
import pytest

import tournament_points_ref as G
import tournament_ref as R
from bpl import NeutralDixonColesMatchPredictorWC, group_points
from bpl._ffi import BPLHIP_EINVAL, BPLHIP_ESTATE, BplHipError, HipContext
from bpl.base import _prng_key, points_axis
from bpl.neutral_dixon_coles import points_result
from test_tournament_host import conf_of, hand_posterior

pytestmark = pytest.mark.gpu
SEED, DRAWS = 2468, 7
MODE_IDS = ["overall-redraw", "h2h-redraw", "overall-extra_time", "h2h-extra_time"]
FORMATS = ["2x3", "3x3", "euro24", "wc48"]
TABLES = ("team_points_count", "team_target_count", "team_place_count", "place_points_count", "place_gap_count")
REST = ("rest_count", "rest_through_count", "rest_rank_count")
RAW = ("team_points", "team_target", "team_place", "place_points", "place_gap", "rest_count", "rest_through", "rest_rank")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def mode(name, rounds):
    """(tiebreak, the knockout rule's keywords) of a mode for a bracket of `rounds` rounds."""
    tiebreak = "head_to_head" if name.startswith("h2h") else "overall"
    if name.endswith("redraw"):
        return tiebreak, {}
    if tiebreak == "overall":
        return tiebreak, dict(knockout_rule="extra_time", legs=tuple(2 - r % 2 for r in range(rounds)), away_goals=True,
                              shootout={"t01": 0.8, "t04": -0.4})
    return tiebreak, dict(knockout_rule="extra_time", legs=tuple(1 + r % 2 for r in range(rounds)), shootout={"t03": 1.5})


def shape(name):
    """(model, simulate_tournament kwargs, hosts, N) of a case."""
    if name == "2x3":
        # 2 groups of 3, the winners meet: R = 1, no best of the rest; N mod DRAWS != 0
        m = hand_posterior(T=6, S=DRAWS, seed=41)
        return m, R.group_format(list(m.teams), 2, 3, 0, seed=1, advance=1), None, 1501
    if name == "3x3":
        # 3 groups of 3, the winners and the best second: R = 2
        m = hand_posterior(T=9, S=DRAWS, seed=42)
        return m, R.group_format(list(m.teams), 3, 3, 1, seed=2, advance=1), None, 1501
    if name == "euro24":
        m = hand_posterior(T=24, S=DRAWS, seed=43)
        return m, R.euro_24(list(m.teams), seed=3), None, 1501
    if name == "wc48":
        m = hand_posterior(T=48, S=DRAWS, seed=44)
        return m, R.world_cup_48(list(m.teams), seed=4), None, 2000
    if name == "unequal":
        # groups of 4, 4, 3, 3, 3 with advance 3: only two groups have a fourth place (B = 2 < Gn = 5), the better of
        # the two fourths goes on; 15 + 1 qualifiers, R = 4
        m = hand_posterior(T=17, S=DRAWS, seed=45)
        t = list(m.teams)
        groups = {"A": t[0:4], "B": t[4:8], "C": t[8:11], "D": t[11:14], "E": t[14:17]}
        entries = [(g, p) for g in groups for p in (1, 2, 3)] + [("best", 1)]
        order = np.random.RandomState(8).permutation(16)
        return m, {"groups": groups, "advance": 3, "best_of_rest": 1, "knockout": [entries[i] for i in order]}, None, 1201
    if name == "host_second":
        # t01 is a host and listed second in the first fixture of the default round robin (t00 v t01)
        m = hand_posterior(T=8, S=DRAWS, seed=46)
        kw = {"groups": {"A": list(m.teams[:4]), "B": list(m.teams[4:])}, "advance": 2,
              "knockout": [("A", 1), ("B", 2), ("B", 1), ("A", 2)]}
        return m, kw, ["t01"], 1201
    if name == "wc_class":
        # the World-Cup class: confederation strengths in every rate; 3 groups of 4 and the two best thirds, R = 3
        m = hand_posterior(NeutralDixonColesMatchPredictorWC, T=12, S=DRAWS, seed=47)
        return m, R.group_format(list(m.teams), 3, 4, 2, seed=5), ["t06"], 1201
    if name == "played_h2h":
        # two matchdays played (they fill the table and the head-to-head records), the last pair of fixtures left
        m = hand_posterior(T=8, S=DRAWS, seed=48)
        kw = {"groups": {"A": list(m.teams[:4]), "B": list(m.teams[4:])}, "advance": 2,
              "knockout": [("A", 1), ("B", 2), ("B", 1), ("A", 2)]}
        home = ["t00", "t02", "t00", "t01", "t04", "t06", "t04", "t05"]
        away = ["t01", "t03", "t02", "t03", "t05", "t07", "t06", "t07"]
        kw["played"] = {"home_team": home, "away_team": away, "home_goals": [1, 0, 2, 1, 0, 1, 1, 0],
                        "away_goals": [1, 0, 1, 0, 2, 1, 1, 0]}
        kw["group_fixtures"] = [("t00", "t03"), ("t01", "t02"), ("t04", "t07"), ("t05", "t06")]
        return m, kw, ["t03"], 1201
    raise KeyError(name)


def _call(m, kw, hosts, tiebreak, rule, n_sims, seed=SEED):
    """(the public call's keywords, the checked inputs, the head-to-head records or None), the last two as the public
    call itself forms them."""
    conf = conf_of(m) if isinstance(m, NeutralDixonColesMatchPredictorWC) else None
    common = dict(num_simulations=n_sims, random_state=seed, hosts=hosts, team_conf=conf, tiebreak=tiebreak, **kw, **rule)
    inp, call = m._tournament_call(kw["knockout"], kw.get("groups"), kw.get("advance", 2), kw.get("best_of_rest", 0),
                                   kw.get("group_fixtures"), kw.get("current_table"), hosts, (3, 1, 0), n_sims, seed,
                                   conf, tiebreak, kw.get("played"), rule.get("knockout_rule", "redraw"),
                                   rule.get("legs"), rule.get("extra_time_scale", 1 / 3), rule.get("shootout"),
                                   rule.get("away_goals", False))
    return common, inp, call


@functools.lru_cache(maxsize=None)
def device(name, mode_id):
    """One device run per (case, mode), shared by the tests and left unchanged: (model, keywords, inputs, result)."""
    m, kw, hosts, n_sims = shape(name)
    rounds = len(kw["knockout"]).bit_length() - 1
    tiebreak, rule = mode(mode_id, rounds)
    common, inp, call = _call(m, kw, hosts, tiebreak, rule, n_sims)
    return m, common, inp, call, m.tournament_points(**common)


def _check_sums(res, inp):
    N, best = inp["num_simulations"], inp["best_of_rest"]
    sizes = np.bincount(inp["group"])
    np.testing.assert_array_equal(res["team_points_count"].sum(axis=1), N)
    np.testing.assert_array_equal(res["team_target_count"].sum(axis=1), res["target_count"])
    np.testing.assert_array_equal(res["team_place_count"].sum(axis=2), res["team_points_count"])
    np.testing.assert_array_equal(res["place_points_count"].sum(axis=2), N * (np.arange(inp["group_size"])[None, :] < sizes[:, None]))
    np.testing.assert_array_equal(res["place_gap_count"].sum(axis=2), N * (np.arange(1, inp["group_size"])[None, :] < sizes[:, None]))
    if best > 0:
        B = int((sizes > inp["advance"]).sum())
        assert res["rest_rank_count"].shape[0] == B
        assert res["rest_count"].sum() == N * B and res["rest_through_count"].sum() == N * best
        np.testing.assert_array_equal(res["rest_rank_count"].sum(axis=(1, 2)), N)
        np.testing.assert_array_equal(res["rest_rank_count"].sum(axis=0), res["rest_count"])
        np.testing.assert_array_equal(res["rest_rank_count"][:best].sum(axis=0), res["rest_through_count"])
    else:
        assert not any(k in res for k in REST)


def _check_against_restatement(name, mode_id):
    m, common, inp, call, res = device(name, mode_id)
    ref = G.simulate(R.model_tables(m), inp, _prng_key(SEED), head_to_head=common["tiebreak"] == "head_to_head",
                     pair_init=call["kwargs"].get("pair_init"))
    assert ref["flagged"].sum() == 0, ref["flagged"].sum()
    points_min, n_bins = int(res["points"][0]), res["points"].size
    want = G.counts(ref, inp, points_min, n_bins, gd_cap=3)
    assert set(want) == {k for k in TABLES + REST if k in res}
    for k, v in want.items():
        assert res[k].dtype == np.int64 and res[k].shape == v.shape, k
        np.testing.assert_array_equal(res[k], v, err_msg=k)
    _check_sums(res, inp)
    return m, common, inp, res, ref


# ---- 1. every integer table against the restatement, and against tournament_paths' own records: H2H x ET
@pytest.mark.parametrize("mode_id", MODE_IDS)
@pytest.mark.parametrize("name", FORMATS)
def test_tables_against_restatement(name, mode_id):
    m, common, inp, res, _ = _check_against_restatement(name, mode_id)
    Rr = inp["rounds"]
    assert list(res["targets"]) == [f"round_{r}" for r in range(Rr)] + ["winner", "group_winner"]
    assert list(res["teams"]) == list(inp["teams"]) and list(res["groups"]) == inp["group_names"]
    assert ("decided_proba" in res) == ("knockout_rule" in common)
    if name == "wc48":
        assert res["rest_rank_count"].shape == (12, 10, 7) and res["team_target_count"].shape == (48, 10, 7)


@pytest.mark.parametrize("mode_id", MODE_IDS)
@pytest.mark.parametrize("name", FORMATS)
def test_tables_against_tournament_paths_records(name, mode_id):
    m, common, inp, _, res = device(name, mode_id)
    paths = m.tournament_paths(return_records=True, **common)
    rec = G.records_from_paths(paths, inp)
    want = G.counts(rec, inp, int(res["points"][0]), res["points"].size)
    assert set(want) == set(TABLES)
    for k, v in want.items():
        np.testing.assert_array_equal(res[k], v, err_msg=k)


# ---- 2. equalities with the existing methods, under one random_state
@pytest.mark.parametrize("mode_id", MODE_IDS)
def test_equalities_with_simulate_tournament_and_scenarios(mode_id):
    m, common, inp, _, res = device("3x3", mode_id)
    Rr = inp["rounds"]
    sim = m.simulate_tournament(**common)
    for k in ("round_proba", "group_position_proba") + (("decided_proba",) if "knockout_rule" in common else ()):
        assert res[k].dtype == sim[k].dtype and res[k].shape == sim[k].shape, k
        np.testing.assert_array_equal(res[k], sim[k], err_msg=k)
    assert ("decided_proba" in res) == ("decided_proba" in sim)
    scen = m.tournament_scenarios(fixtures=[0], margin_cap=1, **common)
    np.testing.assert_array_equal(res["target_count"][:, Rr:], scen["target_count"][:, Rr:])
    np.testing.assert_array_equal(res["target_count"], scen["target_count"])


# ---- 3. chunking and determinism
def test_chunking_and_determinism():
    m, kw, hosts, _ = shape("3x3")
    tiebreak, rule = mode("h2h-extra_time", 2)
    N = 203          # no multiple of 7 or 64
    _, inp, call = _call(m, kw, hosts, tiebreak, rule, N)
    pmin, bins = points_axis(inp["table"][:, 0], inp["fix_p"], inp["fix_q"], inp["points"])
    ctx = m._device()
    extra = dict(points_min=pmin, n_bins=bins, gd_cap=2)
    first = ctx.tournament_points(*call["args"], chunk_sims=0, **extra, **call["kwargs"])
    assert set(first) == set(RAW) | {"decided_counts"}
    assert first["team_points"].sum() == 9 * N and first["decided_counts"].sum() == 3 * N
    for chunk in (0, 1, 7, 64):        # 0 again: two runs are bit-identical
        again = ctx.tournament_points(*call["args"], chunk_sims=chunk, **extra, **call["kwargs"])
        assert set(again) == set(first)
        for k in first:
            np.testing.assert_array_equal(again[k], first[k], err_msg=f"{k} chunk {chunk}")


def test_one_simulation():
    m, kw, hosts, _ = shape("3x3")
    common, inp, _ = _call(m, kw, hosts, "overall", {}, 1)
    res = m.tournament_points(**common)
    _check_sums(res, inp)
    assert res["team_points_count"].sum() == 9 and res["rest_through_count"].sum() == 1
    np.testing.assert_array_equal(res["round_proba"], m.simulate_tournament(**common)["round_proba"])


# ---- 4. designed cases
def test_deterministic_groups():
    # no group fixture left: the current table IS the group stage.  Groups A and C are level on points between the
    # first two places (goal difference decides), the thirds have 3 / 3 / 2 points and goal differences -1 / -3 / 0
    m = hand_posterior(T=12, S=DRAWS, seed=49)
    kw = R.group_format(list(m.teams), 3, 4, 2, seed=6)
    t = list(m.teams)
    rows = [(7, 5, 2), (7, 4, 2), (3, 2, 3), (0, 1, 5),      # A: level at the top, third 3 points, -1
            (9, 6, 1), (6, 4, 3), (3, 2, 5), (0, 2, 5),      # B: third 3 points, -3
            (5, 3, 1), (5, 2, 1), (2, 2, 2), (2, 1, 4)]      # C: level at the top and at the bottom, third 2 points, 0
    kw["current_table"] = {t[i]: rows[i] for i in range(12)}
    kw["group_fixtures"] = []
    N = 301
    for tiebreak in ("overall", "head_to_head"):
        common, inp, _ = _call(m, kw, None, tiebreak, {}, N)
        res = m.tournament_points(gd_cap=2, **common)
        _check_sums(res, inp)
        pts = np.array([r[0] for r in rows])
        np.testing.assert_array_equal(res["points"], np.arange(0, 10))
        # every group table has one cell, with count N
        want = np.zeros((12, 10), dtype=np.int64)
        want[np.arange(12), pts] = N
        np.testing.assert_array_equal(res["team_points_count"], want)
        place = np.array([0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3])
        assert (res["team_place_count"][np.arange(12), pts, place] == N).all() and res["team_place_count"].sum() == 12 * N
        assert (res["place_points_count"][np.repeat(np.arange(3), 4), place, pts] == N).all()
        gaps = np.array([[0, 4, 3], [3, 3, 3], [0, 3, 0]])
        for g in range(3):
            for z in range(3):
                assert res["place_gap_count"][g, z, gaps[g, z]] == N and res["place_gap_count"][g, z].sum() == N
        np.testing.assert_array_equal(res["level_proba"], (gaps == 0).astype(np.float64))
        # the thirds: (3, -1) best, (3, -3 -> clipped to -2) second, (2, 0) out
        rest = np.zeros((10, 5), dtype=np.int64)
        rest[3, 1], rest[3, 0], rest[2, 2] = N, N, N
        np.testing.assert_array_equal(res["rest_count"], rest)
        rest[2, 2] = 0
        np.testing.assert_array_equal(res["rest_through_count"], rest)
        for k, cell in enumerate([(3, 1), (3, 0), (2, 2)]):
            assert res["rest_rank_count"][k][cell] == N
        assert group_points.cut_line(res) == (3, -2, 1.0)
        # two of the three thirds go through whatever they have; all of those with at least 3 points do
        np.testing.assert_array_equal(res["rest_proba_given_at_least"][:4], [2 / 3, 2 / 3, 2 / 3, 1.0])
        np.testing.assert_array_equal(res["rest_points_needed"], [0.0, 3.0, 3.0])


def _coarsen(table, c_from, c_to):
    """A [..., 2 c_from + 1] goal-difference table re-summed to the narrower cap c_to."""
    d = np.clip(np.arange(-c_from, c_from + 1), -c_to, c_to) + c_to
    out = np.zeros(table.shape[:-1] + (2 * c_to + 1,), dtype=table.dtype)
    np.add.at(out, (Ellipsis, d), table)
    return out


def test_goal_difference_clipping():
    # t00 and t04 score freely: their group rivals' goal differences pass -8, their own pass +8
    m = hand_posterior(T=12, S=DRAWS, seed=50)
    m.attack[:, [0, 4]] += 2.2
    kw = R.group_format(list(m.teams), 3, 4, 2, seed=7)
    common, inp, _ = _call(m, kw, None, "overall", {}, 1201)
    res = {c: m.tournament_points(gd_cap=c, **common) for c in (0, 1, 8)}
    for c, r in res.items():
        _check_sums(r, inp)
        assert r["rest_count"].shape == (10, 2 * c + 1) and list(r["goal_difference"]) == list(range(-c, c + 1))
        for k in TABLES:
            np.testing.assert_array_equal(r[k], res[8][k], err_msg=k)
    assert res[8]["rest_count"][:, 0].sum() > 0          # a third-placed team at -8 or worse: the clip is exercised
    for c in (0, 1):
        for k in REST:
            np.testing.assert_array_equal(_coarsen(res[8][k], 8, c), res[c][k], err_msg=f"{k} cap {c}")


@pytest.mark.parametrize("mode_id", ["overall-redraw", "h2h-extra_time"])
def test_unequal_groups(mode_id):
    m, common, inp, res, _ = _check_against_restatement("unequal", mode_id)
    assert res["place_points_count"].shape == (5, 4, 10) and res["rest_rank_count"].shape == (2, 10, 7)
    np.testing.assert_array_equal(res["place_points_quantile"][:, 2:, 3], -1)
    assert (res["place_points_quantile"][:, :2] >= 0).all() and (res["place_points_quantile"][:, 2:, :3] >= 0).all()
    assert np.isnan(res["place_points_mean"][2:, 3]).all() and not np.isnan(res["place_points_mean"][:2]).any()
    assert not res["place_gap_count"][2:, 2].any() and not res["place_points_count"][2:, 3].any()
    # the rest are the two fourths: slots of groups A and B only
    assert res["rest_count"].sum() == 2 * inp["num_simulations"]


@pytest.mark.parametrize("name,mode_id", [("host_second", "overall-extra_time"), ("wc_class", "overall-redraw"),
                                          ("wc_class", "h2h-extra_time"), ("played_h2h", "h2h-redraw")])
def test_designed_shapes(name, mode_id):
    m, common, inp, res, ref = _check_against_restatement(name, mode_id)
    if name == "host_second":
        # the host listed second plays at home: without the flag the tables differ
        plain = m.tournament_points(**dict(common, hosts=None))
        assert not np.array_equal(plain["team_points_count"], res["team_points_count"])
    if name == "wc_class":
        assert inp["conf"] is not None and res["rest_rank_count"].shape[0] == 3
    if name == "played_h2h":
        np.testing.assert_array_equal(inp["table"][:4], [[4, 3, 2], [4, 2, 1], [1, 1, 2], [1, 0, 1]])
        assert res["points"][0] == 1 and res["points"][-1] == 7


def test_floats_come_from_the_integers():
    m, common, inp, _, res = device("euro24", "overall-extra_time")
    raw = {k: res[f"{k}_count"] for k in ("team_points", "team_target", "team_place", "place_points", "place_gap")}
    raw.update(rest_count=res["rest_count"], rest_through=res["rest_through_count"], rest_rank=res["rest_rank_count"])
    again = points_result(inp, raw, int(res["points"][0]), res["levels"])
    for k, v in again.items():
        np.testing.assert_array_equal(res[k], v, err_msg=k)
    text = group_points.format_table(res, "t05")
    assert text.splitlines()[0] == "t05" and "group_winner" in text
    p, d, share = group_points.cut_line(res)
    assert share == res["cut_proba"].max() and res["cut_proba"][p - int(res["points"][0]), d + 3] == share


# ---- 5. errors
def test_context_state_and_argument_errors():
    ctx = HipContext(0)
    try:
        grp = dict(team_idx=[0, 1, 2, 3], team_group=[0, 0, 1, 1], bracket=[0x0001, 0x0101], n_sims=10, key=(0, 1),
                   fix_p=[0, 2], fix_q=[1, 3], advance=1, points_min=0, n_bins=4)
        with pytest.raises(BplHipError) as e:        # no posterior
            ctx.tournament_points(**grp)
        assert e.value.code == BPLHIP_ESTATE
        S_, T = 4, 8
        ctx.predict_set_posterior(np.zeros((S_, T)), np.zeros((S_, T)), np.zeros(S_), np.zeros(S_))
        with pytest.raises(BplHipError) as e:        # a plain posterior
            ctx.tournament_points(**grp)
        assert e.value.code == BPLHIP_ESTATE
        ctx.predict_set_posterior_venue(*[np.zeros((S_, T)) for _ in range(6)], np.zeros(S_))
        out = ctx.tournament_points(**grp)
        assert set(out) == set(RAW[:5]) and out["team_points"].shape == (4, 4) and out["team_points"].sum() == 40
        assert out["place_gap"].shape == (2, 1, 4) and out["place_gap"].sum() == 20
        none = ctx.tournament_points(**dict(grp, fix_p=[], fix_q=[], n_bins=1))      # no fixtures: allowed
        assert none["team_points"].sum() == 40 and none["place_gap"][:, :, 0].sum() == 20
        ko = dict(team_idx=[0, 1, 2, 3], bracket=[0, 1, 2, 3], n_sims=10, key=(0, 1), points_min=0, n_bins=4)
        rule = {"legs_mask": 0, "scale": 1 / 3, "away_goals": 0, "strength": None}
        bad = [
            ko,                                              # no groups: no group points
            dict(grp, n_bins=3),                             # a win leaves the axis at the top
            dict(grp, points_min=1),                         # a defeat leaves it at the bottom
            dict(grp, n_bins=0),
            dict(grp, n_bins=257),
            dict(grp, gd_cap=-1),
            dict(grp, gd_cap=9),
            dict(grp, chunk_sims=-1),
            dict(grp, n_sims=0),
            dict(grp, team_idx=[0, 1, 2, 9]),
            dict(grp, points=(3, -1, 0)),
            dict(grp, knockout=dict(rule, scale=0.0)),
        ]
        for kwargs in bad:
            with pytest.raises(BplHipError) as e:
                ctx.tournament_points(**kwargs)
            assert e.value.code == BPLHIP_EINVAL, kwargs
        again = ctx.tournament_points(**grp)         # the context stays usable, and the run repeats
        for k in out:
            np.testing.assert_array_equal(again[k], out[k], err_msg=k)
    finally:
        ctx.close()
