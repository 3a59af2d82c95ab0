"""The order of the checks of the live entry points that tests/test_gpu_season_errors.py and
tests/test_gpu_tournament_errors.py do not reach: bplhip_match_leverage_live, bplhip_season_points_live,
bplhip_season_scenarios_live, bplhip_simulate_tournament_live, bplhip_tournament_paths_live,
bplhip_tournament_scenarios_live and bplhip_tournament_points_live.  In their manner: the loaded library's symbol,
the return code and the whole text of bplhip_last_error, every call wrong in two ways so that the earlier check is
the one reported.  A live call checks, in this order: the two lists and the states; the family's shared checks
(a posterior, the table or the slots, the fixtures over the concatenated list); the entry's own arguments and
outputs; the log weights; the pair records.  The tournament entries check "matches in play need groups" and "the
final scores come as a pair" between the states and the shared checks.  No case reaches a kernel.

bplhip_simulate_tournament_live has no argument of its own kind (no axis, key or chunk), so its call across "own
argument / null output" is n_sims = 0 against a null stage_counts; bplhip_tournament_points_live takes no final
scores, so its two calls around them pair "without groups" with no posterior only.

Season: 4 draws, a 6-row table of an 8-team model, 3 fixtures to kick off (0-1, 2-3, 4-5) and 2 in play (0-2, 3-4).
Tournament: 8 slots in 2 groups of 4, the first two of each into a bracket of 4, 2 group fixtures to kick off (0-1,
4-5) and 2 in play (0-2, 4-6).  A win is 3 points, so a slot with a fixture and a match in play ends on 0..6."""
import ctypes as C

import numpy as np
import pytest

from bpl._ffi import BPLHIP_EINVAL, BPLHIP_ESTATE, HipContext, _np_ptr

pytestmark = pytest.mark.gpu
S, T, SIMS, F, L = 4, 8, 10, 3, 2        # draws, model teams, simulations; the season's fixtures and matches in play
N = 6                                    # the season's table rows
CN, CF = 8, 2                            # the tournament's slots and group fixtures to kick off
SEASON = {"leverage": "bplhip_match_leverage_live", "points": "bplhip_season_points_live",
          "scenarios": "bplhip_season_scenarios_live"}
CUP = {"cup": "bplhip_simulate_tournament_live", "paths": "bplhip_tournament_paths_live",
       "cup_scenarios": "bplhip_tournament_scenarios_live", "cup_points": "bplhip_tournament_points_live"}
SYMBOLS = dict(SEASON, **CUP)
# the name at the front of the live checks' messages, and of the entry's own checks
LIVE = {tag: SYMBOLS[tag][len("bplhip_"):] for tag in SYMBOLS}
OWN = dict({tag: LIVE[tag] for tag in SEASON}, cup="simulate_tournament", paths="tournament_paths",
           cup_scenarios="tournament_scenarios", cup_points="tournament_points")


def _over(n):
    """Slot 0 has 65535 head-to-head points against slot 1, and meets it again."""
    pair = np.zeros((n, n), dtype=np.uint32)
    pair[0, 1] = 0xFFFF << 16
    return pair


SPECIAL = {"elapsed_one": np.array([0.5, 1.0]), "nan": np.array([0.0, np.nan, 0.0, 0.0]),
           "mask_outside": np.array([1 << N], dtype=np.uint64), "away_outside": np.array([2, 7], dtype=np.uint16),
           "key_season": np.array([F + L], dtype=np.int32), "key_cup": np.array([CF + L], dtype=np.int32),
           "over_season": _over(N), "over_cup": _over(CN), "some": np.zeros((SIMS, L), dtype=np.uint8)}


@pytest.fixture(scope="module")
def contexts():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    made = {(family, posterior): HipContext(0) for family in ("season", "cup") for posterior in (False, True)}
    made["season", True].predict_set_posterior(np.zeros((S, T)), np.zeros((S, T)), np.zeros(S), np.zeros(S))
    made["cup", True].predict_set_posterior_venue(*(np.zeros((S, T)) for _ in range(6)), np.zeros(S))
    yield made
    for ctx in made.values():
        ctx.close()


def _live(keep, dtype, p, q, sides):
    """The live request, n_in_play to log_evidence, the two sides under the parameter names `p` and `q`."""
    keep.update(sides=[np.array(v, dtype=dtype) for v in sides], goals=[np.zeros(L, dtype=np.uint8) for _ in range(2)],
                elapsed=np.array([0.5, 0.25]), stats=[C.c_double(0.0), C.c_double(0.0)])
    return {"n_in_play": L, p: _np_ptr(keep["sides"][0]), q: _np_ptr(keep["sides"][1]),
            "in_play_home_goals": _np_ptr(keep["goals"][0]), "in_play_away_goals": _np_ptr(keep["goals"][1]),
            "in_play_elapsed": _np_ptr(keep["elapsed"]), "reweight": 1, "log_weights": None,
            "ess": C.cast(C.pointer(keep["stats"][0]), C.c_void_p),
            "log_evidence": C.cast(C.pointer(keep["stats"][1]), C.c_void_p)}


def _raw(ctx, tag, over):
    """The arguments of the symbol of `tag`, all valid, as an ordered dict by parameter name with `over` applied; the
    arrays they point into ride along under "_keep"."""
    u8, u16, i32, u64 = np.uint8, np.uint16, np.int32, np.uint64
    keep = dict(big=[np.zeros(4096, dtype=u64) for _ in range(9)], kf=np.array([0], dtype=i32), kc=np.array([1], dtype=i32))
    big = [_np_ptr(b) for b in keep["big"]]
    if tag in SEASON:
        keep.update(h=np.array([0, 2, 4], dtype=u16), a=np.array([1, 3, 5], dtype=u16), ti=np.arange(N, dtype=u16),
                    init=[np.zeros(N, dtype=i32) for _ in range(3)], masks=np.array([0b000011], dtype=u64))
        a = dict(ctx=ctx._h, n_fixtures=F, home_idx=_np_ptr(keep["h"]), away_idx=_np_ptr(keep["a"]), n_table=N,
                 table_idx=_np_ptr(keep["ti"]), init_points=_np_ptr(keep["init"][0]), init_gf=_np_ptr(keep["init"][1]),
                 init_ga=_np_ptr(keep["init"][2]), win=3, draw=1, loss=0, n_sims=SIMS, key_hi=0, key_lo=1, n_targets=1,
                 target_mask=_np_ptr(keep["masks"]), chunk_sims=0)
        if tag == "leverage":
            a.update(out0=big[0], out1=big[1], out2=big[2])
        elif tag == "points":
            a.update(points_min=0, n_bins=7, out0=big[0], out1=big[1], out2=big[2], out3=big[3])
        else:
            a.update(n_key=1, key_fixture=_np_ptr(keep["kf"]), key_cap=_np_ptr(keep["kc"]), out0=big[0], out1=big[1])
        a.update(stream=None, pair_init=None, **_live(keep, u16, "in_play_home_idx", "in_play_away_idx", ([0, 3], [2, 4])))
    else:
        keep.update(ti=np.arange(CN, dtype=u16), grp=np.array([0, 0, 0, 0, 1, 1, 1, 1], dtype=u8),
                    init=[np.zeros(CN, dtype=i32) for _ in range(3)], fp=np.array([0, 4], dtype=u8),
                    fq=np.array([1, 5], dtype=u8), br=np.array([0x0001, 0x0102, 0x0101, 0x0002], dtype=u16))
        a = dict(ctx=ctx._h, n_teams=CN, team_idx=_np_ptr(keep["ti"]), team_conf=None, team_host=None, n_groups=2,
                 team_group=_np_ptr(keep["grp"]), init_points=_np_ptr(keep["init"][0]), init_gf=_np_ptr(keep["init"][1]),
                 init_ga=_np_ptr(keep["init"][2]), n_fixtures=CF, fix_p=_np_ptr(keep["fp"]), fix_q=_np_ptr(keep["fq"]),
                 advance=2, best_of_rest=0, n_bracket=4, bracket=_np_ptr(keep["br"]), win=3, draw=1, loss=0, n_sims=SIMS,
                 key_hi=0, key_lo=1)
        if tag in ("cup", "paths"):
            a.update(stage_counts=big[0], group_position_counts=big[1], sim_stage=None)
        a.update(stream=None, pair_init=None, head_to_head=0, extra_time=0, legs_mask=0, extra_time_scale=1 / 3,
                 away_goals=0, strength=None, decided_counts=big[2])
        if tag in ("cup", "paths"):
            a.update(sim_decided=None)
        if tag == "cup":
            a.update(slot_counts=None)
        elif tag == "paths":
            a.update(chunk_sims=0, out0=big[3], out1=big[4], out2=big[5], out3=big[6], out4=big[7], sim_position=None,
                     sim_outcome=None, sim_pair=None, sim_winner=None)
        elif tag == "cup_scenarios":
            a.update(chunk_sims=0, n_key=1, key_fixture=_np_ptr(keep["kf"]), key_cap=_np_ptr(keep["kc"]), out0=big[3],
                     out1=big[4], sim_scenario=None, sim_tset=None)
        else:
            a.update(chunk_sims=0, points_min=0, n_bins=7, gd_cap=3, **{f"out{i}": big[i + 1] for i in range(8)})
        a.update(_live(keep, u8, "in_play_p", "in_play_q", ([0, 4], [2, 6])))
        if tag != "cup_points":
            a.update(sim_draw=None)
            if tag == "cup":
                a.update(draw_log_weights=None, draw_log_evidence=None)
            a.update(in_play_final_home=None, in_play_final_away=None)
    assert set(over) <= set(a), set(over) - set(a)
    a.update(over)
    a["_keep"] = keep
    return a


# one bad argument of the entry's own, and what its check says after the entry's name
BAD = {"leverage": (dict(chunk_sims=-1), "chunk_sims=-1 is negative"),
       "points": (dict(n_bins=0), "n_bins=0 out of range [1,1024]"),
       "scenarios": (dict(key_fixture="key_season"), "key fixture 0 is 5, outside [0,5)"),
       "cup": (dict(n_sims=0), "n_sims=0 out of range [1,2^31)"),
       "paths": (dict(chunk_sims=-1), "chunk_sims=-1 is negative"),
       "cup_scenarios": (dict(key_fixture="key_cup"), "key fixture 0 is 4, outside [0,4)"),
       "cup_points": (dict(n_bins=0), "n_bins=0 out of range [1,256]")}
# a required output of the entry (its first) and a slot with a fixture and a match in play on an axis of four bins
NULL_OUT = dict(cup="stage_counts")
SHORT = {"points": "season_points_live: slot 0 can end on 0..6 points, outside [0,4)",
         "cup_points": "tournament_points: slot 0 can end on 0..6 points, outside [0,4)"}

# (id, the context has a posterior, tag, overrides, code, message)
CASES = []
for tag in SYMBOLS:
    out = NULL_OUT.get(tag, "out0")
    pair = dict(pair_init="over_season") if tag in SEASON else dict(pair_init="over_cup", head_to_head=1)
    bad, text = BAD[tag]
    CASES += [
        (f"{tag}_elapsed_one_and_no_posterior", False, tag, dict(in_play_elapsed="elapsed_one"), BPLHIP_EINVAL,
         f"{LIVE[tag]}: elapsed 1 of in-play match 1 outside [0, 1)"),
        (f"{tag}_own_argument_and_null_output", True, tag, dict(bad, **{out: None}), BPLHIP_EINVAL, f"{OWN[tag]}: {text}"),
        (f"{tag}_null_output_and_log_weight", True, tag, {out: None, "log_weights": "nan"}, BPLHIP_EINVAL,
         f"{OWN[tag]}: null required output"),
        (f"{tag}_log_weight_and_pair_overflow", True, tag, dict(pair, log_weights="nan"), BPLHIP_EINVAL,
         f"{LIVE[tag]}: log weight 1 is not finite"),
    ]
for tag in SEASON:
    CASES.append((f"{tag}_in_play_team_outside_and_bad_mask", True, tag,
                  dict(in_play_away_idx="away_outside", target_mask="mask_outside"), BPLHIP_EINVAL,
                  f"{LIVE[tag]}: fixture 4 has a team outside the table"))
for tag in ("cup", "paths", "cup_scenarios"):
    CASES += [
        (f"{tag}_no_groups_and_one_final_score", True, tag, dict(n_groups=0, in_play_final_home="some"), BPLHIP_EINVAL,
         f"{LIVE[tag]}: n_in_play=2 without groups"),
        (f"{tag}_one_final_score_and_no_posterior", False, tag, dict(in_play_final_away="some"), BPLHIP_EINVAL,
         f"{LIVE[tag]}: the final scores come as a pair"),
    ]
CASES.append(("cup_points_no_groups_and_no_posterior", False, "cup_points", dict(n_groups=0), BPLHIP_EINVAL,
              "tournament_points_live: n_in_play=2 without groups"))
for tag, text in SHORT.items():
    CASES.append((f"{tag}_axis_too_short_and_log_weight", True, tag, dict(n_bins=4, log_weights="nan"), BPLHIP_EINVAL, text))
# the later check of every pair above is reached once the earlier fault is gone
CASES += [
    ("leverage_no_posterior", False, "leverage", {}, BPLHIP_ESTATE, "match_leverage_live: no posterior set"),
    ("cup_no_posterior", False, "cup", {}, BPLHIP_ESTATE, "simulate_tournament: no posterior set"),
    ("scenarios_pair_overflow", True, "scenarios", dict(pair_init="over_season"), BPLHIP_EINVAL,
     "season_scenarios_live: the pair record of slots 0 and 1 can pass 16 bits"),
    ("cup_pair_overflow", True, "cup", dict(pair_init="over_cup", head_to_head=1), BPLHIP_EINVAL,
     "simulate_tournament: the pair record of slots 0 and 1 can pass 16 bits"),
    ("points_bad_mask", True, "points", dict(target_mask="mask_outside"), BPLHIP_EINVAL,
     "season_points_live: target 0 has no position, or one outside the table"),
    ("cup_points_log_weight", True, "cup_points", dict(log_weights="nan"), BPLHIP_EINVAL,
     "tournament_points_live: log weight 1 is not finite"),
]


@pytest.mark.parametrize("posterior,tag,args,code,message", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_bad_call_reports(contexts, posterior, tag, args, code, message):
    ctx, entry = contexts["season" if tag in SEASON else "cup", posterior], SYMBOLS[tag]
    over = {k: _np_ptr(SPECIAL[v]) if isinstance(v, str) else v for k, v in args.items()}
    a = _raw(ctx, tag, over)
    keep = a.pop("_keep")
    assert len(a) == len(getattr(ctx._lib, entry).argtypes)
    rc = getattr(ctx._lib, entry)(*a.values())
    assert (rc, ctx._lib.bplhip_last_error(ctx._h).decode()) == (code, message)
    del keep
