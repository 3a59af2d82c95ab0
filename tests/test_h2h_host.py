"""The head-to-head tie-break without a GPU (bpl/base.py, tests/h2h_ref.py): the restated rule on hand-built
tables, `pair_records` (packing, orientation, a pair meeting twice, every ValueError), the current table
derived from `played`, the routing of the keywords through a stand-in backend and the three new C symbols."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest

import h2h_ref as H
from bpl import NeutralDixonColesMatchPredictor, _ffi
from bpl.base import check_tiebreak, pair_records, played_matches, remaining_meetings, table_from_played
from test_leverage_host import _hand_posterior
from test_tournament_host import hand_posterior as neutral_posterior

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTS = (3, 1, 0)
A, B, C_, D, E = "t00", "t01", "t02", "t03", "t04"


def _played(matches):
    """[(home, away, home goals, away goals), ...] -> the `played` dict."""
    return {"home_team": [m[0] for m in matches], "away_team": [m[1] for m in matches],
            "home_goals": [m[2] for m in matches], "away_goals": [m[3] for m in matches]}


# Every case: the matches played and the hand-derived order, top to bottom (None: decided by the tie-break word).
HAND_CASES = {
    # A, B, C beat each other in a cycle and each lost to D: 3 points each.  Among the three: GD +2 (A), -1 (B),
    # -1 (C), goals 2 (B) v 1 (C) -> A, B, C.  Overall: GD -3 (A), -2 (B), -2 (C), GF 2 (B) v 1 (C) -> B, C, A.
    "cycle": ([(A, B, 3, 0), (B, C_, 2, 0), (C_, A, 1, 0), (D, A, 5, 0), (D, B, 1, 0), (D, C_, 1, 0)], [D, A, B, C_]),
    # A, B, C on 6 points; among them A took 6, B 3, C 0 -> A, B, C.  Overall GD: -2 (A), +5 (B), +8 (C): the opposite.
    "points": ([(A, B, 1, 0), (A, C_, 1, 0), (B, C_, 1, 0), (D, A, 4, 0), (B, D, 5, 0), (C_, D, 5, 0), (C_, E, 5, 0)],
               [A, B, C_, D, E]),
    # {A, B} on 6 and {C, D} on 3.  A beat B and C beat D; B's big wins over C and D and D's over E count for
    # nothing inside their own sets (a mini-table over the union {A, B, C, D} would put B first).
    "two_sets": ([(A, B, 1, 0), (A, C_, 1, 0), (B, C_, 5, 0), (B, D, 5, 0), (C_, D, 1, 0), (D, E, 9, 0)],
                 [A, B, C_, D, E]),
    # A and B drew with each other: level on keys 2-4.  B's overall GD is better.
    "overall_gd": ([(A, B, 1, 1), (A, C_, 1, 0), (B, C_, 3, 0)], [B, A, C_]),
    # ... the same GD, B scored more
    "overall_gf": ([(A, B, 1, 1), (A, C_, 1, 0), (B, C_, 3, 2)], [B, A, C_]),
    # ... level on everything: the tie-break word, then the slot
    "all_equal": ([(A, B, 1, 1), (A, C_, 1, 0), (B, C_, 1, 0)], None),
}


def hand_case(name):
    """(played dict, teams in slot order, expected order of team names or None)."""
    matches, order = HAND_CASES[name]
    teams = sorted({t for m in matches for t in m[:2]})
    return _played(matches), teams, order


def _order(played, teams, words=None, head_to_head=True):
    slot_of = {t: i for i, t in enumerate(teams)}
    n = len(teams)
    table = table_from_played(played, slot_of, n, POINTS)
    pair = pair_records(played, slot_of, n, POINTS)
    words = np.zeros((1, n), dtype=np.int64) if words is None else np.asarray(words)[None, :]
    pts, gf, ga = (table[None, :, c] for c in range(3))
    if head_to_head:
        pos = H.rank(pts, gf, ga, pair, words)[0]
    else:
        pos = H.overall_ahead(pts, gf, ga, words).sum(axis=1)[0]
    assert sorted(pos) == list(range(n))
    return [teams[i] for i in np.argsort(pos)]


def test_three_way_cycle_is_decided_by_the_head_to_head_goal_difference():
    played, teams, order = hand_case("cycle")
    assert _order(played, teams) == order == [D, A, B, C_]
    assert _order(played, teams, head_to_head=False) == [D, B, C_, A]
    slot_of = {t: i for i, t in enumerate(teams)}
    table = table_from_played(played, slot_of, 4, POINTS)
    hp, hgd, hgf = H.h2h_keys(table[None, :, 0], pair_records(played, slot_of, 4, POINTS))
    np.testing.assert_array_equal(hp[0], [3, 3, 3, 0])
    np.testing.assert_array_equal(hgd[0], [2, -1, -1, 0])
    np.testing.assert_array_equal(hgf[0], [3, 2, 1, 0])


def test_three_way_tie_on_head_to_head_points_against_the_overall_goal_difference():
    played, teams, order = hand_case("points")
    assert _order(played, teams) == order
    assert _order(played, teams, head_to_head=False) == [C_, B, A, D, E]


def test_two_disjoint_tied_sets_and_a_team_level_with_nobody():
    played, teams, order = hand_case("two_sets")
    assert _order(played, teams) == order
    assert _order(played, teams, head_to_head=False) == [B, A, D, C_, E]
    slot_of = {t: i for i, t in enumerate(teams)}
    table = table_from_played(played, slot_of, 5, POINTS)
    np.testing.assert_array_equal(table[:, 0], [6, 6, 3, 3, 0])
    hp, hgd, hgf = H.h2h_keys(table[None, :, 0], pair_records(played, slot_of, 5, POINTS))
    np.testing.assert_array_equal(hp[0], [3, 0, 3, 0, 0])      # only the match inside the own set counts
    np.testing.assert_array_equal(hgd[0], [1, -1, 1, -1, 0])
    np.testing.assert_array_equal(hgf[0], [1, 0, 1, 0, 0])     # E is level with nobody: an empty mini-table


def test_level_on_the_head_to_head_keys_falls_to_gd_gf_word_slot():
    for name in ("overall_gd", "overall_gf"):
        played, teams, order = hand_case(name)
        assert _order(played, teams) == order, name
        assert _order(played, teams, words=[9, 0, 0]) == order, name     # the word comes after GD and GF
    played, teams, order = hand_case("all_equal")
    assert order is None
    assert _order(played, teams, words=[5, 9, 0]) == [B, A, C_]
    assert _order(played, teams, words=[9, 5, 0]) == [A, B, C_]
    assert _order(played, teams, words=[7, 7, 0]) == [A, B, C_]            # the slot, ascending


def test_rank_is_vectorised_and_grouped():
    """Two simulations with different pair records; with groups a slot is compared with its own group only."""
    pts = np.array([[3, 3, 3, 3], [3, 3, 3, 3]])
    zero = np.zeros_like(pts)
    pair = np.zeros((2, 4, 4), dtype=np.int64)
    pair[0, 1, 0] = 3 << 16 | 1           # simulation 0: slot 1 beat slot 0
    pair[1, 0, 1] = 3 << 16 | 1           # simulation 1: slot 0 beat slot 1
    pair[:, 3, 0] = 3 << 16 | 4           # slot 3 beat slot 0 (another group below)
    pair[:, 2, 3] = 3 << 16 | 2           # slot 2 beat slot 3
    pos = H.rank(pts, zero, zero, pair, zero, group=[0, 0, 1, 1])
    np.testing.assert_array_equal(pos, [[1, 0, 0, 1], [0, 1, 0, 1]])
    pos = H.rank(pts, zero, zero, pair, zero)
    assert sorted(pos[0]) == [0, 1, 2, 3] and pos[0, 0] == 3   # slot 0 lost twice and won nothing


# ---------------------------------------------------------------- pair_records
def test_pair_records_packing_orientation_and_a_pair_meeting_twice():
    slot_of = {A: 0, B: 1, C_: 2}
    played = _played([(A, B, 2, 0), (B, A, 1, 1), (C_, A, 4, 3)])
    pair = pair_records(played, slot_of, 3, POINTS)
    assert pair.dtype == np.uint32 and pair.shape == (3, 3)
    assert pair[0, 1] == (3 + 1) << 16 | (2 + 1)      # A against B: a home win 2-0 and an away draw 1-1
    assert pair[1, 0] == (0 + 1) << 16 | (0 + 1)
    assert pair[2, 0] == 3 << 16 | 4 and pair[0, 2] == 0 << 16 | 3
    assert pair[1, 2] == 0 and pair[2, 1] == 0 and (np.diag(pair) == 0).all()
    assert pair_records(played, slot_of, 3, (2, 1, 0))[0, 1] == (2 + 1) << 16 | 3
    np.testing.assert_array_equal(pair_records(None, None, 3, POINTS), np.zeros((3, 3), dtype=np.uint32))
    # a slot order other than the names' order
    np.testing.assert_array_equal(pair_records(played, {A: 2, B: 0, C_: 1}, 3, POINTS),
                                  pair[np.ix_([1, 2, 0], [1, 2, 0])])


def test_pair_records_errors():
    slot_of = {A: 0, B: 1}
    ok = _played([(A, B, 1, 0)])
    pair_records(ok, slot_of, 2, POINTS)
    bad = [
        _played([(A, "nope", 1, 0)]),                     # an unknown name
        _played([(A, C_, 1, 0)]),                         # a team outside the table
        _played([(A, A, 1, 0)]),                          # a team playing itself
        dict(ok, home_goals=[1, 2]),                      # unequal lengths
        _played([(A, B, 1.5, 0)]),                        # non-integer goals
        _played([(A, B, 1, -1)]),                         # negative goals
        _played([(A, B, True, 0)]),
        _played([(A, B, "1", 0)]),
        {"home_team": [A], "away_team": [B], "home_goals": [1]},   # a missing column
    ]
    for played in bad:
        with pytest.raises(ValueError):
            pair_records(played, slot_of, 2, POINTS)
    with pytest.raises(ValueError):
        pair_records(ok, slot_of, 2, (3, 1))
    assert pair_records(_played([(A, B, 2.0, np.int64(1))]), slot_of, 2, POINTS)[0, 1] == 3 << 16 | 2


def test_pair_records_sixteen_bit_bound():
    slot_of = {A: 0, B: 1}
    assert pair_records(_played([(A, B, 65535, 0)]), slot_of, 2, POINTS)[0, 1] == 3 << 16 | 65535
    with pytest.raises(ValueError):
        pair_records(_played([(A, B, 65536, 0)]), slot_of, 2, POINTS)          # goals played alone
    meet = remaining_meetings([0], [1], 2)
    np.testing.assert_array_equal(meet, [[0, 1], [1, 0]])
    assert pair_records(_played([(A, B, 65280, 0)]), slot_of, 2, POINTS, remaining=meet)[0, 1] & 0xFFFF == 65280
    with pytest.raises(ValueError):
        pair_records(_played([(A, B, 65281, 0)]), slot_of, 2, POINTS, remaining=meet)   # + 255 to come
    # points: 65 wins of 1000 are 65000; one more meeting can bring 1000
    wins = _played([(A, B, 1, 0)] * 65)
    with pytest.raises(ValueError):
        pair_records(wins, slot_of, 2, (1000, 1, 0), remaining=meet)
    assert pair_records(wins, slot_of, 2, (1000, 1, 0))[0, 1] >> 16 == 65000
    # without anything played: 258 meetings of up to 255 goals pass 16 bits, 257 do not
    with pytest.raises(ValueError):
        pair_records(None, None, 2, POINTS, remaining=258 * meet)
    pair_records(None, None, 2, POINTS, remaining=257 * meet)


def test_tiebreak_names():
    assert check_tiebreak("overall") is False and check_tiebreak("head_to_head") is True
    for bad in ("h2h", None, 1, "Head_to_head"):
        with pytest.raises(ValueError):
            check_tiebreak(bad)


# ---------------------------------------------------------------- the keywords, through stand-in backends
class OldSurfaceCtx:
    """Stands in for bpl._ffi.HipContext with the signatures it had BEFORE the head-to-head keywords: a default
    call that passed `pair_init` or `head_to_head` on would be a TypeError."""

    def __init__(self):
        self.calls = []

    def predict_set_posterior(self, *arrays):
        pass

    def predict_set_posterior_venue(self, *arrays, **kw):
        pass

    def simulate_season(self, home_idx, away_idx, table_idx, table, points, n_sims, key, return_tables=False,
                        return_scores=False):
        self.calls.append(("simulate_season", np.asarray(table_idx), np.asarray(table)))
        n = len(table_idx)
        return {"counts": np.zeros((n, n), np.uint64), "points_sum": np.zeros(n, np.int64), "gd_sum": np.zeros(n, np.int64)}

    def match_leverage(self, home_idx, away_idx, table_idx, table, points, n_sims, key, target_masks, chunk_sims=0):
        self.calls.append(("match_leverage", np.asarray(table_idx), np.asarray(table)))
        n, k, nf = len(table_idx), len(target_masks), len(home_idx)
        return {"outcome": np.zeros((nf, 3), np.uint64), "target": np.zeros((n, k), np.uint64),
                "joint": np.zeros((nf, 3, n, k), np.uint64)}

    def simulate_tournament(self, team_idx, bracket, n_sims, key, team_conf=None, team_host=None, team_group=None,
                            table=None, fix_p=(), fix_q=(), advance=2, best_of_rest=0, points=(3, 1, 0),
                            return_stages=False):
        self.calls.append(("simulate_tournament", np.asarray(team_idx), np.asarray(table)))
        n, r = len(team_idx), len(bracket).bit_length() - 1
        return {"stage_counts": np.zeros((n, r + 2), np.uint64), "position_counts": np.zeros((n, 8), np.uint64)}


class NewSurfaceCtx(OldSurfaceCtx):
    """... and with the new keywords, recorded."""

    def simulate_season(self, *args, pair_init=None, head_to_head=False, **kw):
        self.h2h = (head_to_head, pair_init)
        return super().simulate_season(*args, **kw)

    def match_leverage(self, *args, pair_init=None, head_to_head=False, **kw):
        self.h2h = (head_to_head, pair_init)
        return super().match_leverage(*args, **kw)

    def simulate_tournament(self, *args, pair_init=None, head_to_head=False, **kw):
        self.h2h = (head_to_head, pair_init)
        return super().simulate_tournament(*args, **kw)


def test_default_keywords_never_reach_a_head_to_head_entry_point():
    m = _hand_posterior()
    m._predict_ctx = ctx = OldSurfaceCtx()
    H_, A_ = ["t00", "t01", "t02"], ["t01", "t02", "t00"]
    m.simulate_season(H_, A_, num_simulations=10, random_state=1)
    m.simulate_season(H_, A_, num_simulations=10, random_state=1, tiebreak="overall")
    m.match_leverage(H_, A_, num_simulations=10, random_state=1)
    m.match_leverage(H_, A_, num_simulations=10, random_state=1, tiebreak="overall", played=_played([(A, B, 1, 0)]))
    assert [c[0] for c in ctx.calls] == ["simulate_season"] * 2 + ["match_leverage"] * 2
    with pytest.raises(TypeError):
        m.simulate_season(H_, A_, num_simulations=10, random_state=1, tiebreak="head_to_head")
    nm = neutral_posterior(NeutralDixonColesMatchPredictor, T=8)
    nm._predict_ctx = nctx = OldSurfaceCtx()
    groups = {"A": list(nm.teams[:4]), "B": list(nm.teams[4:8])}
    ko = [("A", 1), ("B", 2), ("B", 1), ("A", 2)]
    nm.simulate_tournament(ko, groups, num_simulations=10, random_state=1)
    assert [c[0] for c in nctx.calls] == ["simulate_tournament"]
    with pytest.raises(TypeError):
        nm.simulate_tournament(ko, groups, num_simulations=10, random_state=1, tiebreak="head_to_head")


class _RecordingLib:
    """Stands in for the loaded library: every bplhip_* call is recorded by name and succeeds."""

    def __init__(self):
        self.called = []

    def __getattr__(self, name):
        if not name.startswith("bplhip_"):
            raise AttributeError(name)

        def call(*args):
            self.called.append((name, len(args)))
            return 0
        return call


class _NoTorch:
    class cuda:
        device = staticmethod(lambda device: contextlib.nullcontext())


def _hollow_context():
    ctx = _ffi.HipContext.__new__(_ffi.HipContext)
    ctx._lib, ctx._torch, ctx._h, ctx.device = _RecordingLib(), _NoTorch, None, None
    ctx._stream = lambda: None
    return ctx


def test_hip_context_routes_to_the_new_symbols_only_when_asked():
    ctx = _hollow_context()
    season = ([0, 1], [1, 0], [0, 1], np.zeros((2, 3)), (3, 1, 0), 10, (0, 1))
    ctx.simulate_season(*season)
    ctx.simulate_season(*season, pair_init=np.ones((2, 2)))       # not read without head_to_head
    ctx.match_leverage(*season, [1])
    ko = dict(team_idx=[0, 1, 2, 3], team_group=[0, 0, 1, 1], bracket=[0x0001, 0x0101], n_sims=10, key=(0, 1),
              fix_p=[0, 2], fix_q=[1, 3], advance=1)
    ctx.simulate_tournament(**ko)
    names = [c[0] for c in ctx._lib.called]
    assert names == ["bplhip_simulate_season"] * 2 + ["bplhip_match_leverage", "bplhip_simulate_tournament"]
    counts = dict(ctx._lib.called)
    ctx._lib.called.clear()
    ctx.simulate_season(*season, head_to_head=True)
    ctx.match_leverage(*season, [1], head_to_head=True, pair_init=np.zeros((2, 2)))
    ctx.simulate_tournament(**ko, head_to_head=True)
    assert [c[0] for c in ctx._lib.called] == ["bplhip_simulate_season_h2h", "bplhip_match_leverage_h2h",
                                               "bplhip_simulate_tournament_h2h"]
    for name, nargs in ctx._lib.called:       # the counterpart's arguments plus pair_init
        assert nargs == counts[name[:-4]] + 1 == len(_ffi._SIGNATURES[name][1])
    with pytest.raises(ValueError):
        ctx.simulate_season(*season, head_to_head=True, pair_init=np.zeros((3, 3)))
    ctx._h = None


class _KeepingLib:
    """Like _RecordingLib, but keeps the arguments of every call, not only their number."""

    def __init__(self):
        self.args = []

    def __getattr__(self, name):
        if not name.startswith("bplhip_"):
            raise AttributeError(name)
        return lambda *args: self.args.append((name, args)) or 0


def test_hip_context_gives_every_season_entry_point_the_same_head():
    ctx = _hollow_context()
    ctx._lib = _KeepingLib()
    season = ([0, 1, 0], [1, 0, 1], [0, 1], [[1, 2, 3], [4, 5, 6]], (3, 1, 0), 10, (7, 9))
    ctx.simulate_season(*season)
    ctx.simulate_season_live(*season)
    ctx.match_leverage(*season, [1])
    ctx.season_points(*season, [1], 0, 8)
    ctx.season_trajectory(*season, [1], 0, 8, [0, 1, 2], [3])
    assert [name for name, _ in ctx._lib.args] == ["bplhip_simulate_season", "bplhip_simulate_season_live",
                                                   "bplhip_match_leverage", "bplhip_season_points",
                                                   "bplhip_season_trajectory"]
    pointers = (2, 3, 5, 6, 7, 8)       # home_idx, away_idx, table_idx, init_points, init_gf, init_ga
    for name, args in ctx._lib.args:
        assert len(args) == len(_ffi._SIGNATURES[name][1]), name
        head = [a for i, a in enumerate(args[:15]) if i not in pointers]
        assert head == [None, 3, 2, 3, 1, 0, 10, 7, 9], name    # context, n_fixtures, n_table, points, n_sims, key
        assert all(isinstance(args[i], C.c_void_p) and args[i].value for i in pointers), name
    ctx._h = None


def test_head_to_head_keywords_reach_the_backend_with_the_pair_records():
    m = _hand_posterior()
    m._predict_ctx = ctx = NewSurfaceCtx()
    played, teams, _ = hand_case("cycle")
    res = m.simulate_season([A], [B], num_simulations=10, random_state=1, tiebreak="head_to_head", played=played)
    assert list(res["teams"]) == teams
    head_to_head, pair = ctx.h2h
    slot_of = {t: i for i, t in enumerate(teams)}
    assert head_to_head is True
    np.testing.assert_array_equal(pair, pair_records(played, slot_of, 4, POINTS))
    # the current table is what `played` adds up to ...
    np.testing.assert_array_equal(ctx.calls[-1][2], table_from_played(played, slot_of, 4, POINTS))
    np.testing.assert_array_equal(ctx.calls[-1][2], [[3, 3, 6], [3, 2, 4], [3, 1, 3], [9, 7, 0]])
    # ... also without the head-to-head order, and a given current_table wins over it
    m.simulate_season([A], [B], num_simulations=10, random_state=1, played=played)
    np.testing.assert_array_equal(ctx.calls[-1][2], [[3, 3, 6], [3, 2, 4], [3, 1, 3], [9, 7, 0]])
    own = {A: (1, 2, 3), B: (0, 0, 0), C_: (0, 0, 0), D: (5, 5, 5)}
    m.match_leverage([A], [B], num_simulations=10, random_state=1, tiebreak="head_to_head", played=played,
                     current_table=own, targets={"title": (0,)})
    np.testing.assert_array_equal(ctx.calls[-1][2], [[1, 2, 3], [0, 0, 0], [0, 0, 0], [5, 5, 5]])
    np.testing.assert_array_equal(ctx.h2h[1], pair_records(played, slot_of, 4, POINTS))
    # without `played` the records are zero
    m.simulate_season([A], [B], num_simulations=10, random_state=1, tiebreak="head_to_head")
    np.testing.assert_array_equal(ctx.h2h[1], np.zeros((2, 2), dtype=np.uint32))


def test_season_argument_errors_are_raised_on_the_host():
    m = _hand_posterior()
    kw = dict(num_simulations=10, random_state=1)
    bad = [
        dict(tiebreak="h2h"),
        dict(played=_played([(A, "nope", 1, 0)])),
        dict(played=_played([(A, A, 1, 0)])),
        dict(played=_played([(A, B, 1, -2)])),
        dict(played=_played([(A, B, 0.5, 0)])),
        dict(played=dict(_played([(A, B, 1, 0)]), away_goals=[])),
        dict(played=_played([(A, C_, 1, 0)]), current_table={A: (0, 0, 0)}),    # C is outside the table
        dict(played=_played([(A, C_, 1, 0)]), teams=[A, B]),
        dict(played=_played([(A, B, 65300, 0)]), tiebreak="head_to_head"),       # + 255 for the meeting to come
    ]
    for extra in bad:
        for method in (m.simulate_season, m.match_leverage):
            with pytest.raises(ValueError):
                method([A], [B], **kw, **extra)
            assert m._predict_ctx is None, extra   # no device context was ever made
    # 258 remaining meetings of one pair
    with pytest.raises(ValueError):
        m.simulate_season([A] * 258, [B] * 258, tiebreak="head_to_head", **kw)
    assert m._predict_ctx is None


def test_tournament_keywords_played_and_errors():
    m = neutral_posterior(NeutralDixonColesMatchPredictor, T=8)
    t = list(m.teams)
    groups = {"A": t[:4], "B": t[4:8]}
    ko = [("A", 1), ("B", 2), ("B", 1), ("A", 2)]
    kw = dict(num_simulations=10, random_state=1)
    played = _played([(t[0], t[1], 2, 1), (t[5], t[4], 0, 0)])
    for extra in (dict(tiebreak="nope"), dict(played=_played([(t[0], t[4], 1, 0)])),       # two groups
                  dict(played=_played([(t[0], "nope", 1, 0)])), dict(played=_played([(t[0], t[0], 1, 0)])),
                  dict(played=_played([(t[0], t[1], -1, 0)])), dict(played=dict(played, home_team=[t[0]])),
                  dict(played=_played([(t[0], t[1], 65400, 0)]), tiebreak="head_to_head")):
        with pytest.raises(ValueError):
            m.simulate_tournament(ko, groups, **kw, **extra)
        assert m._predict_ctx is None
    with pytest.raises(ValueError):
        m.simulate_tournament(t[:4], played=played, **kw)                                   # played needs groups
    m._predict_ctx = ctx = NewSurfaceCtx()
    m.simulate_tournament(ko, groups, tiebreak="head_to_head", played=played, **kw)
    head_to_head, pair = ctx.h2h
    assert head_to_head is True and pair.shape == (8, 8)
    assert pair[0, 1] == 3 << 16 | 2 and pair[1, 0] == 1 and pair[5, 4] == 1 << 16 and pair[4, 5] == 1 << 16
    assert np.count_nonzero(pair) == 4
    want = np.zeros((8, 3), dtype=np.int64)
    want[0], want[1], want[4], want[5] = (3, 2, 1), (0, 1, 2), (1, 0, 0), (1, 0, 0)
    np.testing.assert_array_equal(ctx.calls[-1][2], want)
    m.simulate_tournament(ko, groups, tiebreak="head_to_head", played=played,
                          current_table={t[0]: (7, 7, 7)}, **kw)
    assert ctx.calls[-1][2][0].tolist() == [7, 7, 7] and ctx.calls[-1][2][1:].sum() == 0
    np.testing.assert_array_equal(ctx.h2h[1], pair)


# ---------------------------------------------------------------- the C ABI
COUNTERPART = {"bplhip_simulate_season_h2h": "bplhip_simulate_season", "bplhip_match_leverage_h2h": "bplhip_match_leverage",
               "bplhip_simulate_tournament_h2h": "bplhip_simulate_tournament"}


def _params(header, name):
    decl = re.search(rf"int {name}\((.*?)\);", header, re.S).group(1)
    return [" ".join(p.split()) for p in decl.split(",")]


@pytest.mark.parametrize("name", sorted(COUNTERPART))
def test_new_symbols_are_declared_as_the_header_says(name):
    header = open(os.path.join(ROOT, "include", "bplhip.h")).read()
    params, old = _params(header, name), _params(header, COUNTERPART[name])
    assert params == old + ["const uint32_t* pair_init"]
    restype, argtypes = _ffi._SIGNATURES[name]
    old_restype, old_argtypes = _ffi._SIGNATURES[COUNTERPART[name]]
    assert restype is C.c_int is old_restype and argtypes == old_argtypes + [C.c_void_p]
    assert len(argtypes) == len(params)
    assert [a is C.c_void_p for a in argtypes] == ["*" in p for p in params]
    scalar = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32}
    assert [a for a, p in zip(argtypes, params) if "*" not in p] == [scalar[p.split()[0]] for p in params if "*" not in p]
    fn = getattr(_ffi.load_library(), name)
    assert fn(*([None] * len(argtypes[:1])), *[0 if "*" not in p else None for p in params[1:]]) == -1   # EINVAL: no context


def test_played_matches_resolves_slots():
    hs, as_, x, y = played_matches(_played([(B, A, 2, 1), (A, C_, 0, 0)]), {A: 0, B: 1, C_: 2})
    assert (hs.tolist(), as_.tolist(), x.tolist(), y.tolist()) == ([1, 0], [0, 2], [2, 0], [1, 0])
