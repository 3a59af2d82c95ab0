"""The argument errors of the tournament family's six entry points (bplhip_simulate_tournament, _h2h, _knockout,
bplhip_tournament_paths, bplhip_tournament_scenarios, bplhip_tournament_points): the code and the whole message of
each, and with two faults in one call the one that is reported.  The checks run in a fixed order on the host
("The tournament family's shared paths"): the checks every entry shares up to the required outputs, the
knockout rule, the slots, groups, bracket and fixtures, the entry's own arguments in the order of its parameters,
tournament_points' axis, and the pair records last.  No case reaches a kernel.

Every case goes through the loaded library's symbol: a null table or a flag out of range is nothing the HipContext
methods can express.  Four slots in two groups of two, slot 0 meets 1 and 2 meets 3, the group winners play the
final; two posterior draws."""
import numpy as np
import pytest

from bpl._ffi import BPLHIP_EINVAL, BPLHIP_ESTATE, HipContext, _np_ptr

pytestmark = pytest.mark.gpu
S, T, N, NF, SIMS = 2, 6, 4, 2, 10       # draws, model teams, slots, group fixtures, simulations
OVER = np.zeros((N, N), dtype=np.uint32)
OVER[0, 1] = 0xFFFF << 16                # slot 0 has 65535 head-to-head points against slot 1, and meets it again
P = "bplhip_simulate_tournament"
SYMBOLS = {"plain": P, "h2h": P + "_h2h", "knockout": P + "_knockout", "paths": "bplhip_tournament_paths",
           "scenarios": "bplhip_tournament_scenarios", "points": "bplhip_tournament_points"}


@pytest.fixture(scope="module")
def contexts():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    bare, ready = HipContext(0), HipContext(0)
    ready.predict_set_posterior_venue(*(np.zeros((S, T)) for _ in range(6)), np.zeros(S))
    yield {False: bare, True: ready}
    bare.close()
    ready.close()


def _raw(ctx, name, over):
    """The arguments of the symbol `name`, all valid, as an ordered dict by parameter name with `over` applied; the
    arrays they point into ride along under "_keep"."""
    u8, u16, i32, u64 = np.uint8, np.uint16, np.int32, np.uint64
    keep = dict(ti=np.arange(N, dtype=u16), grp=np.array([0, 0, 1, 1], dtype=u8),
                init=[np.zeros(N, dtype=i32) for _ in range(3)], fp=np.array([0, 2], dtype=u8),
                fq=np.array([1, 3], dtype=u8), br=np.array([0x0001, 0x0101], dtype=u16),
                big=[np.zeros(4096, dtype=u64) for _ in range(9)], kf=np.array([0], dtype=i32),
                kc=np.array([1], dtype=i32))
    big = [_np_ptr(b) for b in keep["big"]]
    a = dict(ctx=ctx._h, n_teams=N, team_idx=_np_ptr(keep["ti"]), team_conf=None, team_host=None, n_groups=2,
             team_group=_np_ptr(keep["grp"]), init_points=_np_ptr(keep["init"][0]), init_gf=_np_ptr(keep["init"][1]),
             init_ga=_np_ptr(keep["init"][2]), n_fixtures=NF, fix_p=_np_ptr(keep["fp"]), fix_q=_np_ptr(keep["fq"]),
             advance=1, best_of_rest=0, n_bracket=2, bracket=_np_ptr(keep["br"]), win=3, draw=1, loss=0, n_sims=SIMS,
             key_hi=0, key_lo=1)
    if name in (SYMBOLS["scenarios"], SYMBOLS["points"]):
        a.update(stream=None)
    else:
        a.update(stage_counts=big[0], group_position_counts=big[1], sim_stage=None, stream=None)
    if name != P:
        a.update(pair_init=None)
    if name not in (P, SYMBOLS["h2h"]):
        a.update(head_to_head=0)
        if name != SYMBOLS["knockout"]:
            a.update(extra_time=1)
        a.update(legs_mask=0, extra_time_scale=1 / 3, away_goals=0, strength=None, decided_counts=big[2])
        if name in (SYMBOLS["knockout"], SYMBOLS["paths"]):
            a.update(sim_decided=None)
    if name == SYMBOLS["paths"]:
        a.update(chunk_sims=0, advance_counts=big[3], position_stage_counts=big[4], outcome_counts=big[5],
                 target_counts=big[6], joint_counts=big[7], sim_position=None, sim_outcome=None, sim_pair=None,
                 sim_winner=None)
    if name == SYMBOLS["scenarios"]:
        a.update(chunk_sims=0, n_key=1, key_fixture=_np_ptr(keep["kf"]), key_cap=_np_ptr(keep["kc"]), scenario=big[3],
                 joint=big[4], sim_scenario=None, sim_tset=None)
    if name == SYMBOLS["points"]:
        a.update(chunk_sims=0, points_min=0, n_bins=4, gd_cap=3, **{f"out{i}": big[i] for i in range(1, 9)})
    assert set(over) <= set(a), set(over) - set(a)
    a.update(over)
    a["_keep"] = keep
    return a


NO_POSTERIOR = "simulate_tournament: no posterior set"
BRACKET = "simulate_tournament: the bracket must have 2^R entries, 1 <= R <= 6"
TABLE = "simulate_tournament: n_groups=2 out of range [0,16] or null group table"
SCALE = "simulate_tournament: extra_time_scale=0 outside (0,1]"
AWAY = "simulate_tournament: away_goals is 0 / 1"
PAIR = "simulate_tournament: the pair record of slots 0 and 1 can pass 16 bits"
H2H = dict(head_to_head=1, pair_init="over")
# one bad argument of the entry's own per recording mode, and the message of its check
MODE = {"paths": (dict(chunk_sims=-1), "tournament_paths: chunk_sims=-1 is negative"),
        "scenarios": (dict(key_fixture="key_outside"), "tournament_scenarios: key fixture 0 is 2, outside [0,2)"),
        "points": (dict(n_bins=0), "tournament_points: n_bins=0 out of range [1,256]")}

# (id, the context has a posterior, symbol, overrides, code, message)
CASES = []
for tag in SYMBOLS:
    CASES += [
        (f"{tag}_no_posterior_and_no_sims", False, tag, dict(n_sims=0), BPLHIP_ESTATE, NO_POSTERIOR),
        (f"{tag}_bad_bracket_and_no_sims", True, tag, dict(n_bracket=3, n_sims=0), BPLHIP_EINVAL, BRACKET),
    ]
for tag in ("knockout", "paths", "scenarios", "points"):
    CASES.append((f"{tag}_null_table_and_bad_scale", True, tag, dict(init_gf=None, extra_time_scale=0.0),
                  BPLHIP_EINVAL, SCALE))
for tag, (bad, message) in MODE.items():
    CASES += [
        (f"{tag}_bad_away_goals_and_bad_mode", True, tag, dict(bad, away_goals=2), BPLHIP_EINVAL, AWAY),
        (f"{tag}_bad_mode_and_pair_overflow", True, tag, dict(bad, **H2H), BPLHIP_EINVAL, message),
        (f"{tag}_pair_overflow", True, tag, H2H, BPLHIP_EINVAL, PAIR),
    ]
CASES += [
    ("h2h_null_table_and_pair_overflow", True, "h2h", dict(init_gf=None, pair_init="over"), BPLHIP_EINVAL, TABLE),
    ("h2h_pair_overflow", True, "h2h", dict(pair_init="over"), BPLHIP_EINVAL, PAIR),
    ("knockout_bad_away_goals_and_pair_overflow", True, "knockout", dict(away_goals=2, **H2H), BPLHIP_EINVAL, AWAY),
    ("knockout_null_table_and_pair_overflow", True, "knockout", dict(init_gf=None, **H2H), BPLHIP_EINVAL, TABLE),
    ("knockout_pair_overflow", True, "knockout", H2H, BPLHIP_EINVAL, PAIR),
    ("plain_null_output_and_bad_table", True, "plain", dict(stage_counts=None, init_gf=None),
     BPLHIP_EINVAL, "simulate_tournament: null required output"),
    ("paths_null_output_and_bad_scale", True, "paths", dict(group_position_counts=None, extra_time_scale=0.0),
     BPLHIP_EINVAL, "simulate_tournament: null required output"),
    ("paths_null_paths_output_and_pair_overflow", True, "paths", dict(joint_counts=None, **H2H),
     BPLHIP_EINVAL, "tournament_paths: null required output"),
    ("scenarios_negative_chunk_and_key_outside", True, "scenarios", dict(chunk_sims=-1, key_fixture="key_outside"),
     BPLHIP_EINVAL, "tournament_scenarios: chunk_sims=-1 is negative"),
    ("scenarios_key_outside_and_bad_cap", True, "scenarios", dict(key_fixture="key_outside", key_cap="cap_zero"),
     BPLHIP_EINVAL, "tournament_scenarios: key fixture 0 is 2, outside [0,2)"),
    ("points_no_bins_and_bad_gd_cap", True, "points", dict(n_bins=0, gd_cap=-1),
     BPLHIP_EINVAL, "tournament_points: n_bins=0 out of range [1,256]"),
    ("points_null_output_and_axis_too_short", True, "points", dict(out5=None, n_bins=3),
     BPLHIP_EINVAL, "tournament_points: null required output"),
    ("points_axis_too_short_and_pair_overflow", True, "points", dict(n_bins=3, **H2H),
     BPLHIP_EINVAL, "tournament_points: slot 0 can end on 0..3 points, outside [0,3)"),
    ("points_axis_starts_late_and_pair_overflow", True, "points", dict(points_min=1, **H2H),
     BPLHIP_EINVAL, "tournament_points: slot 0 can end on 0..3 points, outside [1,5)"),
]


@pytest.mark.parametrize("posterior,tag,args,code,message", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_bad_call_reports(contexts, posterior, tag, args, code, message):
    ctx, entry = contexts[posterior], SYMBOLS[tag]
    special = {"over": OVER, "key_outside": np.array([NF], dtype=np.int32), "cap_zero": np.zeros(1, dtype=np.int32)}
    over = {k: _np_ptr(special[v]) if isinstance(v, str) else v for k, v in args.items()}
    a = _raw(ctx, entry, over)
    keep = a.pop("_keep")
    assert len(a) == len(getattr(ctx._lib, entry).argtypes)
    rc = getattr(ctx._lib, entry)(*a.values())
    assert (rc, ctx._lib.bplhip_last_error(ctx._h).decode()) == (code, message)
    del keep
