"""CPU: every case of tests/sim_edge_cases.py still sits on the edge it was built for, and the numpy
restatements flag none of its simulations or replications, so that tests/test_gpu_season_edges.py,
tests/test_gpu_tournament_edges.py and tests/test_gpu_ppc_edges.py compare every one of them exactly."""
import numpy as np
import pytest

import ppc_ref as PR
import sim_edge_cases as E
import tournament_ref as TR

SEASON = {c.name: c for c in E.season_cases()}
TOURNAMENT = {c.name: c for c in E.tournament_cases()}
PPC = {c.name: c for c in E.ppc_cases() + [E.ppc_fixture_ids()]}


def _python_positions(pts, gd, gf, words):
    """Positions of one simulation from Python's own integers and tuple order: points, goal difference,
    goals for and the word descending, then the slot ascending."""
    n = len(pts)
    order = sorted(range(n), key=lambda i: (-int(pts[i]), -int(gd[i]), -int(gf[i]), -int(words[i]), i))
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.arange(n)
    return pos


# ------------------------------------------------------------------------------------ season
@pytest.mark.parametrize("name", list(SEASON))
def test_season_case_is_unflagged_and_ranked(name):
    c = SEASON[name]
    ref, table_idx = E.season_reference(c)
    N, n = ref["points"].shape
    assert N == c.call["num_simulations"] and n == table_idx.size
    assert ref["flagged"].sum() <= 1e-4 * N and not ref["flagged"].any()
    np.testing.assert_array_equal(np.sort(ref["position"].astype(np.int64), axis=1), np.tile(np.arange(n), (N, 1)))
    # the restatement's order is the order of Python's integers
    pts, gd, gf = E.season_keys(c)
    words = E.tiebreak_words(c.call["random_state"], N, n)
    for j in range(0, N, max(1, N // 16)):
        np.testing.assert_array_equal(ref["position"][j], _python_positions(pts[j], gd[j], gf[j], words[j]))


@pytest.mark.parametrize("shape", E.SEASON_SHAPES)
def test_season_shape(shape):
    T, n, nf, N, S = shape
    c = SEASON["shape_T%d_n%d_nf%d_N%d_S%d" % shape]
    ref, table_idx = E.season_reference(c)
    m = c.model
    assert m.attack.shape == (S, T) and len(m.teams) == T
    assert ref["points"].shape == (N, n) and ref["home_goals"].shape == (N, nf)
    assert np.all(np.diff(table_idx.astype(np.int64)) > 0)              # the public call's table is in model order
    if T > 64:
        assert m.home_advantage.shape == (S, T)                        # per-team home advantage: ha_stride = T
        listed = c.facts["listed"].astype(np.int64)
        assert sorted(listed.tolist()) == table_idx.tolist() and (np.diff(listed) < 0).any()
        assert table_idx.max() > 64 and len(c.facts["idle"]) >= 5
        assert set(c.facts["idle"]) <= set(table_idx.tolist())
        ref2, tab2 = E.season_reference_in_order(c, c.facts["listed"])
        # the same seasons with the slots renumbered: every slot draws another tie-break word, the points do not move
        back = np.argsort(listed)
        np.testing.assert_array_equal(ref2["points"][:, back], ref["points"])
        np.testing.assert_array_equal(ref2["home_goals"], ref["home_goals"])
        assert tab2.shape == (n, 3)


def test_season_shapes_cover_the_strides():
    shapes = E.SEASON_SHAPES
    assert {s[1] for s in shapes} >= {2, 3, 64}                        # n < 4; every lane a slot
    assert {s[2] for s in shapes} >= {1, 63, 64, 65, 129}              # nf around the 64-lane stride
    assert any(s[3] < 4 for s in shapes) and any(s[3] % 4 for s in shapes)   # below one workgroup's four waves, off it
    assert any(s[4] == 1 for s in shapes) and any(s[4] > s[3] for s in shapes)


@pytest.mark.parametrize("kind", E.RHO_KINDS)
def test_season_ladder(kind):
    c = SEASON["ladder_" + kind]
    ref, _ = E.season_reference(c)
    f = c.facts
    x, y = ref["home_goals"].astype(np.int64), ref["away_goals"].astype(np.int64)
    assert c.model.attack.shape[0] == 1                                 # one draw
    rungs = sorted(set(np.round(f["log_home"], 12).tolist()))
    assert len(rungs) == 10 and rungs[0] == -40.0 and rungs[-1] == 6.5 and rungs == sorted(set(np.round(f["log_away"], 12).tolist()))
    assert {(a, b) for a, b in zip(f["log_home"].tolist(), f["log_away"].tolist())} == \
        {(a, b) for a in E.LADDER_LOG for b in E.LADDER_LOG}
    lo, hi = f["bounds"]
    if kind.startswith("clip"):
        assert f["clipped"] > 0 and not lo <= f["rho"] <= hi
    else:
        assert f["clipped"] == 0 and lo < f["rho"] < hi and (kind == "zero" or min(f["rho"] - lo, hi - f["rho"]) < 1.01e-6)
    for g, log_rate in ((x, f["log_home"]), (y, f["log_away"])):
        assert g.min() == 0 and g.max() == 255
        assert ((g > 63) & (g < 255)).any()                             # walks longer than a wave is wide, short of the cap
        for rung in (float(np.log(300.0)), 6.5):
            assert (g[:, log_rate == rung] == 255).any(), rung
        assert (g[:, log_rate == -40.0] == 0).all()
    # 255 goals are booked: the top rung's teams (9 and 19) carry them into the table
    gd = ref["expected_goal_difference"]
    assert gd[9] > 255 and gd[19] > 255 and ref["points"].max() > 3 * 10


@pytest.mark.parametrize("name", [n for n in SEASON if n.startswith("level_")])
def test_season_level_tables(name):
    c = SEASON[name]
    ref, _ = E.season_reference(c)
    assert np.exp(-np.exp(E.LEVEL_LOG)) == 1.0 and (c.model.attack == E.LEVEL_LOG).all()
    assert not ref["home_goals"].any() and not ref["away_goals"].any()
    pts, gd, gf = E.season_keys(c)
    for key in (pts, gd, gf):
        assert (key == key[:, :1]).all()                                # every simulation: fully tied keys
    N, n = pts.shape
    words = E.tiebreak_words(c.call["random_state"], N, n)
    # the word decides: position = number of larger words (+ equal words at a lower slot)
    ahead = (words[:, :, None] > words[:, None, :]) | ((words[:, :, None] == words[:, None, :])
                                                       & (np.arange(n)[:, None] < np.arange(n)[None, :]))
    np.testing.assert_array_equal(ref["position"], ahead.sum(axis=1))
    assert len({tuple(p) for p in ref["position"].tolist()}) == N         # no two simulations in the same order


def test_season_equal_words():
    c = SEASON["level_equal_words"]
    ref, _ = E.season_reference(c)
    a, b = c.facts["equal_slots"]
    words = E.tiebreak_words(c.call["random_state"], 3, 64)
    assert a < b and words[0, a] == words[0, b]
    assert np.unique(words[0]).size == 63                               # the only coincidence of simulation 0
    assert ref["position"][0, b] == ref["position"][0, a] + 1           # the lower slot is ahead, nothing between


def test_season_sparse_ties():
    c = SEASON["sparse_8"]
    pts, gd, gf = E.season_keys(c)
    N, n = pts.shape
    assert all(np.unique(pts[j]).size < n for j in range(N))            # level on points in every simulation
    full = sum(len({(pts[j, i], gd[j, i], gf[j, i]) for i in range(n)}) < n for j in range(N))
    # a drawn match leaves its two teams level on all three keys: P(some draw in four matches) > 0.5 at these rates
    assert full >= 0.4 * N, full


@pytest.mark.parametrize("points", [(1000, 1, 0), (0, 0, 0)])
def test_season_limits(points):
    c = SEASON["limits_%d_%d_%d" % points]
    ref, _ = E.season_reference(c)
    rows = np.array(c.facts["rows"], dtype=np.int64)
    assert len(rows) == 27 and rows.max() == 1 << 24 and ((1 << 24) - 1 in rows) and rows.min() == 0
    gd0 = rows[:, 1] - rows[:, 2]
    assert gd0.min() == -(1 << 24) and gd0.max() == 1 << 24
    pts, gd, gf = E.season_keys(c)
    assert gd.min() < -(1 << 24) + 300 and gd.max() > (1 << 24) - 300
    if points == (0, 0, 0):
        np.testing.assert_array_equal(pts, np.tile(rows[:, 0], (pts.shape[0], 1)))
    else:
        assert pts.max() >= (1 << 24) + 1000 or (pts - rows[:, 0]).max() >= 1000


# ------------------------------------------------------------------------------------ tournament
@pytest.mark.parametrize("name", list(TOURNAMENT))
def test_tournament_case_is_unflagged(name):
    c = TOURNAMENT[name]
    inp, ref, want = E.tournament_reference(c)
    N, n, R = inp["num_simulations"], len(inp["teams"]), inp["rounds"]
    assert ref["flagged"].sum() <= 1e-3 * N and not ref["flagged"].any()
    assert ref["stage"].shape == (N, n) and want["round_proba"].shape == (n, R + 1)
    stage = ref["stage"].astype(np.int64)
    for r in range(R + 1):
        np.testing.assert_array_equal((stage >= r + 1).sum(axis=1), 2 ** (R - r))


@pytest.mark.parametrize("fmt", E.TOURNAMENT_FORMATS)
@pytest.mark.parametrize("counts", E.TOURNAMENT_COUNTS)
def test_tournament_format(fmt, counts):
    g, size, adv, best, nb = fmt
    N, S = counts
    c = TOURNAMENT["format_%dx%d_adv%d_best%d_ko%d_N%d_S%d" % (fmt + counts)]
    inp, ref, want = E.tournament_reference(c)
    assert c.model.attack.shape[0] == S and inp["num_simulations"] == N
    assert len(inp["teams"]) == g * size and inp["group_size"] == size and len(inp["group_names"]) == g
    assert inp["advance"] == adv and inp["best_of_rest"] == best and 1 << inp["rounds"] == nb == g * adv + best
    assert inp["fix_p"].size == g * size * (size - 1) // 2
    assert want["group_position_proba"].shape == (g * size, size)
    np.testing.assert_array_equal(ref["position_counts"][:, :size].sum(axis=0), np.full(size, N * g))
    assert not ref["position_counts"][:, size:].any()
    if size == 8 and N == 257:
        assert g * size == 64 and inp["fix_p"].size == 224
        assert (ref["position_counts"] > 0).any(axis=0).all()           # all eight places of hist_pos are used


def test_group_format_keeps_its_dicts():
    teams = ["t%02d" % i for i in range(64)]
    for kw in (TR.world_cup_48(teams, seed=1), TR.euro_24(teams, seed=2), TR.group_format(teams, 4, 4, 0, seed=3)):
        assert kw["advance"] == 2 and set(kw) == {"groups", "advance", "best_of_rest", "knockout"}
        names = list(kw["groups"])
        entries = [(g, p) for g in names for p in (1, 2)] + [("best", k) for k in range(1, kw["best_of_rest"] + 1)]
        assert sorted(kw["knockout"]) == sorted(entries)
    # the shuffle is the one the formats always had: the permutation of the entries under the seed
    kw = TR.euro_24(teams, seed=2)
    entries = [(g, p) for g in "ABCDEF" for p in (1, 2)] + [("best", k) for k in range(1, 5)]
    assert kw["knockout"] == [entries[i] for i in np.random.RandomState(2).permutation(16)]
    one = TR.group_format(teams, 4, 3, 0, seed=0, advance=1)
    assert sorted(one["knockout"]) == [(g, 1) for g in "ABCD"] and one["advance"] == 1


@pytest.mark.parametrize("nb", E.KNOCKOUT_BRACKETS)
def test_tournament_knockouts(nb):
    for N, S in E.TOURNAMENT_COUNTS:
        inp, ref, _ = E.tournament_reference(TOURNAMENT["knockout_%d_N%d_S%d" % (nb, N, S)])
        assert inp["group"] is None and 1 << inp["rounds"] == nb and len(inp["teams"]) == nb
        assert (ref["position"] == -1).all() and ref["stage"].min() >= 1


def test_tournament_hosts_swap():
    for name in ("hosts_knockout_8", "hosts_groups_4x4"):
        inp, ref, _ = E.tournament_reference(TOURNAMENT[name])
        host = inp["host"]
        assert host.sum() == 2
        if inp["group"] is None:
            p, q = np.arange(0, 8, 2), np.arange(1, 8, 2)
        else:
            p, q = inp["fix_p"].astype(np.int64), inp["fix_q"].astype(np.int64)
        hs, _, on = TR.venue(p, q, host)
        assert (hs != p).any()                       # a host listed second: swapped into the home side
        assert ((hs == p) & on).any()                # a host listed first
        assert (~on).any()                           # and neutral matches
    # the host of the knockout reaches round two in some simulations: later rounds meet it too
    inp, ref, _ = E.tournament_reference(TOURNAMENT["hosts_knockout_8"])
    assert (ref["stage"][:, 1] >= 2).any() and (ref["stage"][:, 6] >= 2).any()


def _level(m):
    return (np.exp(-np.exp(E.LEVEL_LOG)) == 1.0 and (m.attack == E.LEVEL_LOG).all() and not m.defence.any()
            and not m.home_attack.any() and not m.away_attack.any() and not m.home_defence.any()
            and not m.away_defence.any() and not m.corr_coef.any())


@pytest.mark.parametrize("nb", [2, 8, 64])
def test_tournament_level_knockout_takes_all_attempts(nb):
    c = TOURNAMENT["level_knockout_%d" % nb]
    inp, ref, _ = E.tournament_reference(c)
    assert _level(c.model)                           # every attempt of every pairing is 0-0: 32 attempts, then the rule
    assert inp["host"][1] == 1 and inp["host"][0] == 0   # entry 0's opponent is a host: the home side is listed second
    np.testing.assert_array_equal(ref["stage"], np.tile(E.level_knockout_stage(nb), (inp["num_simulations"], 1)))
    assert ref["stage"][0, 0] == inp["rounds"] + 1
    for r in range(inp["rounds"]):
        assert ref["stage"][0, 1 << r] == r + 1      # entry 2^r goes out in round r


@pytest.mark.parametrize("name", ["level_groups_3x5_empty", "level_groups_3x5_table"])
def test_tournament_level_groups(name):
    c = TOURNAMENT[name]
    inp, ref, _ = E.tournament_reference(c)
    assert _level(c.model) and (inp["table"] == inp["table"][0]).all() and inp["best_of_rest"] == 2
    N, n = ref["position"].shape
    words = E.tiebreak_words(c.call["random_state"], N, n)
    group = inp["group"].astype(np.int64)
    ahead = (words[:, :, None] > words[:, None, :]) & (group[:, None] == group[None, :])[None]
    np.testing.assert_array_equal(ref["position"], ahead.sum(axis=1))   # the words alone order every group
    assert np.unique(words).size == words.size
    # ... and the thirds: the two with the larger words go through
    third = ref["position"] == 2
    for j in range(N):
        t = np.nonzero(third[j])[0]
        assert t.size == 3
        through = t[np.argsort(-words[j, t])][:2]
        assert (ref["stage"][j, through] >= 1).all() and ref["stage"][j, t].astype(bool).sum() == 2
    assert len({tuple(p) for p in ref["position"].tolist()}) > N // 2


def test_tournament_equal_words():
    c = TOURNAMENT["level_groups_8x8_equal_words"]
    inp, ref, _ = E.tournament_reference(c)
    a, b = c.facts["equal_slots"]
    words = E.tiebreak_words(c.call["random_state"], 3, 64)
    assert _level(c.model) and not inp["table"].any()
    assert a < b and words[0, a] == words[0, b] and inp["group"][a] == inp["group"][b]
    assert ref["position"][0, b] == ref["position"][0, a] + 1           # the lower slot is ahead, nothing between


@pytest.mark.parametrize("points", [(1000, 1, 0), (0, 0, 0)])
def test_tournament_limits(points):
    c = TOURNAMENT["limits_%d_%d_%d" % points]
    inp, _, _ = E.tournament_reference(c)
    tab = inp["table"]
    assert sorted(map(tuple, tab.tolist()))[5:] == sorted(E.limit_rows()) and inp["points"] == points
    gd = tab[:, 1] - tab[:, 2]
    assert gd.min() == -(1 << 24) and gd.max() == 1 << 24 and tab[:, 0].max() == 1 << 24
    assert inp["fix_p"].size == 16
    # extreme rows meet inside groups: some group holds both a row at 2^24 and one at 2^24 - 1 in the same column
    group = inp["group"]
    assert any(((tab[group == g] == 1 << 24).any(axis=0) & (tab[group == g] == (1 << 24) - 1).any(axis=0)).any()
               for g in range(8))


# ------------------------------------------------------------------------------------ ppc
@pytest.mark.parametrize("name", list(PPC))
def test_ppc_case_is_unflagged(name):
    c = PPC[name]
    x, y, flagged = E.ppc_reference(c)
    R, n = c.call["num_replications"], len(c.call["data"]["home_team"])
    assert x.shape == y.shape == (R, n)
    assert (~flagged).mean() >= 0.9 and not flagged.any()


def test_ppc_shapes_are_the_ones_asked_for():
    for kind in ("basic", "wc"):
        for n in E.PPC_FIXTURE_COUNTS:
            c = PPC["fixtures_%s_%d" % (kind, n)]
            assert len(c.call["data"]["home_team"]) == n and c.call["num_replications"] == 3
    assert 1025 > 4 * 256 and {255, 256, 257} <= set(E.PPC_FIXTURE_COUNTS)   # 1, 2 and 5 trips of the 256-thread stride
    for name, k, T in (("slots_2", 2, 2), ("slots_130", 130, 130)):
        c = PPC[name]
        idx, hs, as_ = PR.slots(c.model, c.call["data"])
        assert idx.size == k and len(c.model.teams) == T
    for R, S in E.PPC_COUNTS:
        c = PPC["counts_R%d_S%d" % (R, S)]
        assert c.call["num_replications"] == R and c.model.attack.shape[0] == S
    assert PPC["depth_1"].call["max_goals"] == 1 and PPC["depth_15"].call["max_goals"] == 15


def _beyond(x, y, G):
    return {"x": bool(((x > G) & (y <= G)).any()), "y": bool(((x <= G) & (y > G)).any()), "both": bool(((x > G) & (y > G)).any()),
            "inside": bool(((x <= G) & (y <= G)).any())}


@pytest.mark.parametrize("G", [1, 15])
def test_ppc_grid_depths(G):
    c = PPC["ladder_G%d" % G]
    assert c.call["max_goals"] == G and c.model.attack.shape[0] == 1
    d = c.call["data"]
    x, y, _ = E.ppc_reference(c)
    every = {"x": True, "y": True, "both": True, "inside": True}
    assert _beyond(np.asarray(d["home_goals"]), np.asarray(d["away_goals"]), G) == every
    assert _beyond(x, y, G) == every
    assert max(d["home_goals"]) == 255 and max(d["away_goals"]) == 255
    assert x.min() == 0 and y.min() == 0 and ((x == 255) & (y == 255)).any()   # x y = 65025 inside the sums
    assert ((x > 63) & (x < 255)).any() and ((y > 63) & (y < 255)).any()
    idx, hs, as_ = PR.slots(c.model, d)
    raw = PR.raw_tallies(x, y, hs, as_, idx.size, G)
    assert raw["team"][:, 9, 0].min() >= 255 * 10 and raw["sums"][:, 4].min() >= 65025   # the cap in a team's goals, in sum x y
    assert raw["score"][:, G, G].min() >= 4                             # the last bin takes everything beyond
    # the ordinary posterior at depth 1: most scorelines are beyond the grid on some axis
    c1 = PPC["depth_1"]
    x1, y1, _ = E.ppc_reference(c1)
    assert _beyond(x1, y1, 1) == every


def test_ppc_fixture_ids():
    c = PPC["fixture_ids"]
    fid = c.facts["fixture_id"]
    assert fid.max() == (1 << 32) - 1 and fid.min() == 0 and (np.diff(np.sort(fid)) > 1000).sum() >= fid.size - 3
    x, y, _ = E.ppc_reference(c)
    kw = c.call
    from bpl.base import _prng_key
    x0, y0, _ = PR.replicate(c.model, kw["data"], kw["num_replications"], _prng_key(kw["random_state"]))
    assert not np.array_equal(x, x0)                                     # the counters matter
    # the fixtures whose id is their position draw what they draw without ids
    same = np.nonzero(fid == np.arange(fid.size))[0]
    assert same.tolist() == [7]
    np.testing.assert_array_equal(x[:, same], x0[:, same])
    x1, y1, _ = PR.replicate(c.model, kw["data"], kw["num_replications"], _prng_key(kw["random_state"]),
                             fixture_id=np.arange(fid.size))
    np.testing.assert_array_equal(x1, x0)
    np.testing.assert_array_equal(y1, y0)
