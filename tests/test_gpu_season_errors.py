"""The argument errors of the season family's eight entry points (bplhip_simulate_season, _h2h, _playoff, _live,
bplhip_match_leverage, _h2h, bplhip_season_points, bplhip_season_trajectory): the code and the whole message of
each, and with two faults in one call the one that is reported.  The checks run in a fixed order on the host
("The season family's shared host path"); no case reaches a kernel.

A case goes through HipContext where its method can express the fault, and through the loaded library's symbol
where it cannot (a null output, a flag the method never passes)."""
import ctypes as C

import numpy as np
import pytest

from bpl._ffi import BPLHIP_EINVAL, BPLHIP_ESTATE, BplHipError, HipContext, _np_ptr

pytestmark = pytest.mark.gpu
S, T, N, NF, SIMS = 4, 6, 4, 2, 10       # draws, model teams, table rows, fixtures, simulations
OVER = np.zeros((N, N), dtype=np.uint32)
OVER[0, 1] = 0xFFFF << 16                # slot 0 has 65535 head-to-head points against slot 1, and meets it again


@pytest.fixture(scope="module")
def contexts():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    bare, ready = HipContext(0), HipContext(0)
    ready.predict_set_posterior(np.zeros((S, T)), np.zeros((S, T)), np.zeros(S), np.zeros(S))
    yield {False: bare, True: ready}
    bare.close()
    ready.close()


def _season(**over):
    """The keywords every HipContext method of the family takes: slots 0..3 are model teams 0..3, 0 plays 1 and 2
    plays 3, nobody has a point."""
    return dict(dict(home_idx=[0, 2], away_idx=[1, 3], table_idx=[0, 1, 2, 3], table=np.zeros((N, 3)), points=(3, 1, 0),
                     n_sims=SIMS, key=(0, 1)), **over)


# what the methods take beyond _season(): one target (the top two places), an axis that holds 0..3 points, one matchday
TARGETS = dict(target_masks=[0b0011])
AXIS = dict(TARGETS, points_min=0, n_bins=4)
ROUNDS = dict(AXIS, fix_id=[0, 1], round_end=[2])
IN_PLAY = ([1], [2], [0], [0], [0.5])      # slot 1 against slot 2, goalless at half time


def _raw(ctx, name, over):
    """The arguments of the symbol `name`, all valid, as an ordered dict by parameter name with `over` applied; the
    arrays they point into ride along under "_keep"."""
    u16, i32, u64 = (lambda v: np.ascontiguousarray(v, dtype=np.uint16)), np.int32, np.uint64
    keep = dict(h=u16([0, 2]), a=u16([1, 3]), ti=u16([0, 1, 2, 3]), init=[np.zeros(N, dtype=i32) for _ in range(3)],
                counts=np.zeros((N, N), dtype=u64), sums=[np.zeros(N, dtype=np.int64) for _ in range(2)],
                masks=np.array([0b0011], dtype=u64), big=[np.zeros(4096, dtype=u64) for _ in range(8)],
                guests=u16([4, 5]), bracket=u16([0, 0x8001, 0x8000, 3]), live=[u16([1]), u16([2])],
                goals=[np.zeros(1, dtype=np.uint8) for _ in range(2)], elapsed=np.array([0.5]),
                stats=[C.c_double(0.0), C.c_double(0.0)], ends=np.array([2], dtype=i32), ids=np.array([0, 1], dtype=i32))
    big = [_np_ptr(b) for b in keep["big"]]
    a = dict(ctx=ctx._h, n_fixtures=NF, home_idx=_np_ptr(keep["h"]), away_idx=_np_ptr(keep["a"]), n_table=N,
             table_idx=_np_ptr(keep["ti"]), init_points=_np_ptr(keep["init"][0]), init_gf=_np_ptr(keep["init"][1]),
             init_ga=_np_ptr(keep["init"][2]), win=3, draw=1, loss=0, n_sims=SIMS, key_hi=0, key_lo=1)
    if name.startswith("bplhip_simulate_season"):
        a.update(position_counts=_np_ptr(keep["counts"]), points_sum=_np_ptr(keep["sums"][0]),
                 gd_sum=_np_ptr(keep["sums"][1]), sim_points=None, sim_position=None, home_goals=None, away_goals=None,
                 stream=None)
        if name != "bplhip_simulate_season":
            a.update(pair_init=None)
        if name.endswith("_playoff"):
            a.update(head_to_head=0, n_guests=2, guest_idx=_np_ptr(keep["guests"]), bracket=_np_ptr(keep["bracket"]),
                     rounds=2, legs_mask=0b01, neutral_mask=0b10, extra_time_scale=1 / 3, away_goals_rule=1, strength=None,
                     stage_counts=big[0], decided_counts=big[1], sim_stage=None, sim_decided=None)
        if name.endswith("_live"):
            a.update(head_to_head=0, n_in_play=1, in_play_home_idx=_np_ptr(keep["live"][0]),
                     in_play_away_idx=_np_ptr(keep["live"][1]), in_play_home_goals=_np_ptr(keep["goals"][0]),
                     in_play_away_goals=_np_ptr(keep["goals"][1]), in_play_elapsed=_np_ptr(keep["elapsed"]), reweight=1,
                     log_weights=None, ess=C.cast(C.pointer(keep["stats"][0]), C.c_void_p),
                     log_evidence=C.cast(C.pointer(keep["stats"][1]), C.c_void_p), sim_draw=None, draw_log_weights=None,
                     draw_log_evidence=None)
    else:
        a.update(n_targets=1, target_mask=_np_ptr(keep["masks"]), chunk_sims=0)
        if name.startswith("bplhip_match_leverage"):
            a.update(outcome_counts=big[0], target_counts=big[1], joint_counts=big[2], stream=None)
            if name.endswith("_h2h"):
                a.update(pair_init=None)
        else:
            a.update(points_min=0, n_bins=4)
            if name == "bplhip_season_points":
                a.update(team_points=big[0], team_target=big[1], position_points=big[2], gap=big[3])
            else:
                a.update(n_rounds=1, round_end=_np_ptr(keep["ends"]), fix_id=_np_ptr(keep["ids"]),
                         **{f"out{i}": big[i] for i in range(8)})
            a.update(stream=None, pair_init=None)
    assert set(over) <= set(a), set(over) - set(a)
    a.update(over)
    a["_keep"] = keep
    return a


# (id, the context has a posterior, method or symbol, keywords or overrides, code, message)
CASES = [
    # -- two faults at once: the one that is reported
    ("leverage_no_posterior_and_no_targets", False, "match_leverage", _season(target_masks=[]),
     BPLHIP_ESTATE, "match_leverage: no posterior set"),
    ("points_no_posterior_and_no_targets", False, "season_points", _season(**dict(AXIS, target_masks=[])),
     BPLHIP_ESTATE, "season_points: no posterior set"),
    ("trajectory_no_posterior_and_no_targets", False, "season_trajectory", _season(**dict(ROUNDS, target_masks=[])),
     BPLHIP_ESTATE, "season_trajectory: no posterior set"),
    ("live_no_posterior_and_elapsed_one", False, "simulate_season_live", _season(in_play=IN_PLAY[:4] + ([1.0],)),
     BPLHIP_EINVAL, "simulate_season_live: elapsed 1 of in-play match 0 outside [0, 1)"),
    ("live_no_posterior_and_flag_two", False, "bplhip_simulate_season_live", dict(head_to_head=2),
     BPLHIP_EINVAL, "simulate_season_live: head_to_head is 0 / 1"),
    ("leverage_bad_mask_and_null_output", True, "bplhip_match_leverage", dict(target_mask="mask_outside", joint_counts=None),
     BPLHIP_EINVAL, "match_leverage: target 0 has no position, or one outside the table"),
    ("leverage_h2h_negative_chunk_and_null_output", True, "bplhip_match_leverage_h2h", dict(chunk_sims=-1, outcome_counts=None),
     BPLHIP_EINVAL, "match_leverage: chunk_sims=-1 is negative"),
    ("points_bad_mask_and_null_output", True, "bplhip_season_points", dict(target_mask="mask_empty", team_points=None),
     BPLHIP_EINVAL, "season_points: target 0 has no position, or one outside the table"),
    ("trajectory_bad_mask_and_null_output", True, "bplhip_season_trajectory", dict(target_mask="mask_outside", out7=None),
     BPLHIP_EINVAL, "season_trajectory: target 0 has no position, or one outside the table"),
    ("points_no_bins_and_axis_too_short", True, "season_points", _season(**dict(AXIS, n_bins=0)),
     BPLHIP_EINVAL, "season_points: n_bins=0 out of range [1,1024]"),
    ("trajectory_no_bins_and_axis_too_short", True, "season_trajectory", _season(**dict(ROUNDS, n_bins=0)),
     BPLHIP_EINVAL, "season_trajectory: n_bins=0 out of range [1,1024]"),
    ("trajectory_round_end_short_and_fix_id_repeated", True, "season_trajectory",
     _season(**dict(ROUNDS, round_end=[1], fix_id=[0, 0])),
     BPLHIP_EINVAL, "season_trajectory: round_end ends at 1, not at n_fixtures=2"),
    ("trajectory_round_end_falls_and_fix_id_repeated", True, "season_trajectory",
     _season(**dict(ROUNDS, round_end=[2, 1], fix_id=[0, 0])),
     BPLHIP_EINVAL, "season_trajectory: round_end[1]=1 is not non-decreasing within the fixtures"),
    ("trajectory_fix_id_repeated_and_axis_too_short", True, "season_trajectory", _season(**dict(ROUNDS, fix_id=[1, 1], n_bins=3)),
     BPLHIP_EINVAL, "season_trajectory: fix_id is not a permutation of the fixtures (entry 1)"),
    ("points_pair_overflow_and_axis_holds", True, "season_points", _season(**AXIS, head_to_head=True, pair_init=OVER),
     BPLHIP_EINVAL, "season_points: the pair record of slots 0 and 1 can pass 16 bits"),
    ("points_pair_overflow_and_axis_too_short", True, "season_points",
     _season(**dict(AXIS, n_bins=3), head_to_head=True, pair_init=OVER),
     BPLHIP_EINVAL, "season_points: slot 0 can end on 0..3 points, outside [0,3)"),
    ("trajectory_pair_overflow_and_axis_holds", True, "season_trajectory", _season(**ROUNDS, head_to_head=True, pair_init=OVER),
     BPLHIP_EINVAL, "season_trajectory: the pair record of slots 0 and 1 can pass 16 bits"),
    ("trajectory_pair_overflow_and_axis_starts_late", True, "season_trajectory",
     _season(**dict(ROUNDS, points_min=1), head_to_head=True, pair_init=OVER),
     BPLHIP_EINVAL, "season_trajectory: slot 0 can stand on 0..3 points, outside [1,5)"),
    ("season_null_output_and_bad_bracket", True, "bplhip_simulate_season_playoff", dict(gd_sum=None, rounds=0),
     BPLHIP_EINVAL, "simulate_season: null required output"),
    ("playoff_goals_apart_and_flag_two", True, "bplhip_simulate_season_playoff", dict(home_goals="some", head_to_head=2),
     BPLHIP_EINVAL, "simulate_season: home_goals and away_goals go together"),
    ("playoff_flag_two_and_pair_overflow", True, "bplhip_simulate_season_playoff", dict(head_to_head=2, pair_init="over"),
     BPLHIP_EINVAL, "simulate_season_playoff: head_to_head is 0 / 1"),
    ("live_log_weight_and_pair_overflow", True, "simulate_season_live",
     _season(in_play=IN_PLAY, log_weights=[0.0, np.inf, 0.0, 0.0], head_to_head=True, pair_init=OVER),
     BPLHIP_EINVAL, "simulate_season_live: log weight 1 is not finite"),
    ("live_null_output_and_log_weight", True, "bplhip_simulate_season_live", dict(position_counts=None, log_weights="nan"),
     BPLHIP_EINVAL, "simulate_season_live: null required output"),
    # -- one fault: every entry point's own name at the front of a shared check's message
    ("season_fixture_outside_table", True, "simulate_season", _season(away_idx=[1, 5]),
     BPLHIP_EINVAL, "simulate_season: fixture 1 has a team outside the table"),
    ("season_h2h_pair_overflow", True, "simulate_season", _season(head_to_head=True, pair_init=OVER),
     BPLHIP_EINVAL, "simulate_season: the pair record of slots 0 and 1 can pass 16 bits"),
    ("playoff_pair_overflow", True, "bplhip_simulate_season_playoff", dict(head_to_head=1, pair_init="over"),
     BPLHIP_EINVAL, "simulate_season: the pair record of slots 0 and 1 can pass 16 bits"),
    ("live_pair_overflow", True, "simulate_season_live", _season(in_play=IN_PLAY, head_to_head=True, pair_init=OVER),
     BPLHIP_EINVAL, "simulate_season_live: the pair record of slots 0 and 1 can pass 16 bits"),
    ("live_in_play_team_outside_table", True, "simulate_season_live", _season(in_play=([1], [5]) + IN_PLAY[2:]),
     BPLHIP_EINVAL, "simulate_season_live: fixture 2 has a team outside the table"),
    ("leverage_h2h_pair_overflow", True, "match_leverage", _season(**TARGETS, head_to_head=True, pair_init=OVER),
     BPLHIP_EINVAL, "match_leverage: the pair record of slots 0 and 1 can pass 16 bits"),
    ("leverage_too_many_targets", True, "match_leverage", _season(target_masks=[1] * 9),
     BPLHIP_EINVAL, "match_leverage: n_targets=9 out of range [1,8] or null masks"),
    ("leverage_team_repeated", True, "match_leverage", _season(**TARGETS, table_idx=[0, 1, 2, 2]),
     BPLHIP_EINVAL, "match_leverage: table team 2 out of range or repeated"),
    ("points_null_gap", True, "bplhip_season_points", dict(gap=None),
     BPLHIP_EINVAL, "season_points: null required output"),
    ("points_bad_points", True, "season_points", _season(**AXIS, points=(3, 1, -1)),
     BPLHIP_EINVAL, "season_points: bad points"),
    ("trajectory_no_rounds", True, "season_trajectory", _season(**dict(ROUNDS, round_end=[])),
     BPLHIP_EINVAL, "season_trajectory: n_rounds=0 out of range [1,256], or null round_end / fix_id"),
    ("trajectory_no_sims", True, "season_trajectory", _season(**ROUNDS, n_sims=0),
     BPLHIP_EINVAL, "season_trajectory: n_sims=0 out of range [1,2^31)"),
]


@pytest.mark.parametrize("posterior,entry,args,code,message", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_bad_call_reports(contexts, posterior, entry, args, code, message):
    ctx = contexts[posterior]
    if not entry.startswith("bplhip_"):
        with pytest.raises(BplHipError) as e:
            getattr(ctx, entry)(**args)
        assert (e.value.code, str(e.value)) == (code, f"libbplhip error {code}: {message}")
        return
    special = {"mask_outside": np.array([1 << N], dtype=np.uint64), "mask_empty": np.zeros(1, dtype=np.uint64),
               "some": np.zeros((SIMS, NF), dtype=np.uint8), "over": OVER, "nan": np.array([0.0, np.nan, 0.0, 0.0])}
    over = {k: _np_ptr(special[v]) if isinstance(v, str) else v for k, v in args.items()}
    a = _raw(ctx, entry, over)
    keep = a.pop("_keep")
    assert len(a) == len(getattr(ctx._lib, entry).argtypes)
    rc = getattr(ctx._lib, entry)(*a.values())
    assert (rc, ctx._lib.bplhip_last_error(ctx._h).decode()) == (code, message)
    del keep

