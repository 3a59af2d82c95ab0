"""The checks of the five summary entry points bplhip_market_summary, bplhip_period_summary, bplhip_inplay_summary,
bplhip_slate_summary and bplhip_team_ratings, in the manner of tests/test_gpu_live_errors.py: the loaded library's
symbol called raw, the return code and the whole text of bplhip_last_error.  Per entry the faults stand below in the
order in which the entry checks them.  One case makes each fault alone (every fail line of the entry's own, and the
lines of the shared query check that the posterior's form, the record and the team columns reach); one more makes it
together with the next fault that fits the same context, and the earlier check is the one reported.  The orders differ
between the five: market checks the weights before the quantiles; period the quantiles, the splits, then the weights
of the readable cells; in-play the weights, the quantiles, the states (per fixture: elapsed, a score beyond the grid,
a score at elapsed = 0), then the log weights; slate and ratings the quantiles after their own lists; the workspace
rule is the last host check of all five.  No case reaches a kernel.

Not reached: the caps on the posterior's draws (65536, in-play 12288), which need an upload of that size; so the
place of "no posterior set" before the cap is not pinned here.

4 teams, 4 draws, 2 fixtures, max_goals 2 (period: 1), 2 markets, 2 quantiles; ratings 3 teams against 3 opponents;
slate 2 slates of one fixture over 2 leg tables that top out at 1.  Contexts: "P" a plain posterior, "V" a venue one
with 2 confederations, "N" none.  The two slate faults that need many legs bring their own fixture list."""
import ctypes as C

import numpy as np
import pytest

from bpl._ffi import BPLHIP_EINVAL, BPLHIP_ESTATE, HipContext, _np_ptr, fixtures

pytestmark = pytest.mark.gpu
S, T, M, K, NQ, R = 4, 4, 2, 2, 2, 3
SYMBOLS = {"market": "bplhip_market_summary", "period": "bplhip_period_summary", "inplay": "bplhip_inplay_summary",
           "slate": "bplhip_slate_summary", "ratings": "bplhip_team_ratings"}
G = {"market": 2, "period": 1, "inplay": 2, "slate": 2, "ratings": 2}
f64, u8, u16, i32 = np.float64, np.uint8, np.uint16, np.int32


@pytest.fixture(scope="module")
def contexts():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    made = {kind: HipContext(0) for kind in "PVN"}
    made["P"].predict_set_posterior(np.zeros((S, T)), np.zeros((S, T)), np.zeros(S), np.zeros(S))
    made["V"].predict_set_posterior_venue(*(np.zeros((S, T)) for _ in range(6)), np.zeros(S), np.zeros((S, 2)))
    yield made
    for ctx in made.values():
        ctx.close()


def _nan_at(shape, at):
    a = np.zeros(shape)
    a.reshape(-1)[at] = np.nan
    return a


def _raw(ctx, kind, tag, over):
    """The arguments of the symbol of `tag`, all valid for a context of `kind`, as an ordered dict by parameter name
    with `over` applied: an array replaces the one behind the pointer, "fx" holds keyword arguments of
    bpl._ffi.fixtures, "m" replaces the record's count.  What the pointers point into rides along under "_keep"."""
    over = dict(over)
    venue = kind == "V"
    fx = dict(home_idx=[0, 2], away_idx=[1, 3], neutral=0 if venue else None, conf=([0, 1], [1, 0]) if venue else None)
    if tag == "inplay":
        fx.update(home_goals=[0, 1], away_goals=[0, 0])
    fx.update(over.pop("fx", {}))
    q = fixtures(**fx)
    q.m = over.pop("m", q.m)
    g1 = G[tag] + 1
    keep = dict(q=q, big=[np.zeros(4096) for _ in range(8)], quantiles=np.array([0.25, 0.75]),
                weights=np.zeros((K, g1 ** (4 if tag == "period" else 2))), split=np.array([0.5, 0.5]),
                elapsed=np.array([0.5, 0.25]), start=np.array([0, 1, 2], dtype=i32),
                tables=np.array([[0] * 8 + [1]] * 2, dtype=u8), leg_table=np.array([0, 1], dtype=i32),
                teams=np.array([0, 1, 2], dtype=u16), opponents=np.array([1, 2, 3], dtype=u16),
                team_conf=np.array([0, 1, 0], dtype=u16), opponent_conf=np.array([1, 0, 1], dtype=u16),
                points=np.array([3.0, 1.0, 0.0]))
    big = [_np_ptr(b) for b in keep["big"]]
    p = {name: _np_ptr(a) for name, a in keep.items() if isinstance(a, np.ndarray)}
    tail = dict(n_quantiles=NQ, quantiles=p["quantiles"], mean=big[0], sd=big[1], quantile=big[2])
    end = dict(draws=None, workspace_bytes=0, stream=None)
    a = dict(ctx=ctx._h, q=C.byref(q))
    if tag == "market":
        a.update(max_goals=G[tag], n_markets=K, weights=p["weights"], **tail, **end)
    elif tag == "period":
        a.update(split=p["split"], max_goals=G[tag], n_markets=K, weights=p["weights"], **tail, **end)
    elif tag == "inplay":
        a.update(elapsed=p["elapsed"], max_goals=G[tag], n_markets=K, weights=p["weights"], n_quantiles=NQ,
                 quantiles=p["quantiles"], reweight=1, log_weights=None, mean=big[0], sd=big[1], quantile=big[2],
                 ess=big[3], log_evidence=big[4], draws=None, draw_log_evidence=None, workspace_bytes=0, stream=None)
    elif tag == "slate":
        a.update(max_goals=G[tag], n_slates=2, start=p["start"], n_tables=2, tables=p["tables"],
                 leg_table=p["leg_table"], **tail, leg_mean=big[3], **end)
    else:
        a = dict(ctx=ctx._h, n_teams=R, teams=p["teams"], team_conf=p["team_conf"] if venue else None, n_opponents=R,
                 opponents=p["opponents"], opponent_conf=p["opponent_conf"] if venue else None, venue=0,
                 max_goals=G[tag], points=p["points"], rank_by=0, **tail, rank_count=big[3], better_count=big[4],
                 matches=big[5], **end)
    assert set(over) <= set(a), set(over) - set(a)
    for name, value in over.items():
        if isinstance(value, np.ndarray):
            keep["over_" + name] = value
            value = _np_ptr(value)
        a[name] = value
    a["_keep"] = keep
    return a


def _arr(values, dtype=f64):
    return np.array(values, dtype=dtype)


# the shared head and tail of the four fixture entries' ladders: (id, context or None for any, overrides, code, text)
def _scalars(tag, markets):
    top = G[tag] == 1 and 31 or 63
    rows = [("max_goals", None, dict(max_goals=top + 1), BPLHIP_EINVAL, f"max_goals={top + 1} out of range [0,{top}]")]
    if markets:
        rows.append(("n_markets", None, dict(n_markets=0), BPLHIP_EINVAL, f"n_markets=0 out of range [1,{markets}]"))
    return rows + [("n_quantiles", None, dict(n_quantiles=17), BPLHIP_EINVAL, "n_quantiles=17 out of range [0,16]")]


QUERY = [("null_record", None, dict(q=None), BPLHIP_EINVAL, "null fixtures record"),
         ("no_posterior", "N", {}, BPLHIP_ESTATE, "no posterior set"),
         ("plain_query_venue_posterior", "V", dict(fx=dict(neutral=None, conf=None)), BPLHIP_ESTATE,
          "the posterior was set with predict_set_posterior_venue"),
         ("venue_query_plain_posterior", "P", dict(fx=dict(neutral=0)), BPLHIP_ESTATE,
          "the posterior was set with predict_set_posterior"),
         ("negative_m", None, dict(m=-1), BPLHIP_EINVAL, "bad argument"),
         ("no_confederations", "V", dict(fx=dict(conf=None)), BPLHIP_EINVAL,
          "neutral_venue is required, confederations exactly when the posterior has them"),
         ("team_outside", None, dict(fx=dict(away_idx=[1, 4])), BPLHIP_EINVAL, "team index out of range at 1"),
         ("confederation_outside", "V", dict(fx=dict(conf=([0, 1], [1, 2]))), BPLHIP_EINVAL,
          "confederation index out of range at 1")]
QUANTILE = ("quantile", None, dict(quantiles=_arr([0.25, 1.5])), BPLHIP_EINVAL, "quantile 1.5 outside [0, 1]")


def _workspace(text):
    return ("workspace", None, dict(workspace_bytes=8), BPLHIP_EINVAL, f"workspace_bytes=8 {text}")


LADDERS = {
    "market": _scalars("market", 64) + QUERY + [
        ("null_argument", None, dict(mean=None), BPLHIP_EINVAL, "m=2 below 1 or a null argument"),
        ("weight", None, dict(weights=_nan_at((K, 9), 13)), BPLHIP_EINVAL, "weight 4 of market 1 is not finite"),
        QUANTILE, _workspace("holds no fixture (64 bytes each)")],
    "period": _scalars("period", 32) + QUERY + [
        ("null_argument", None, dict(split=None), BPLHIP_EINVAL, "m=2 below 1 or a null argument"),
        QUANTILE,
        ("split", None, dict(split=_arr([0.5, 1.5])), BPLHIP_EINVAL, "split 1.5 of fixture 1 outside [0, 1]"),
        ("weight", None, dict(weights=_nan_at((K, 16), 16)), BPLHIP_EINVAL,
         "market 1 has a non-finite weight on a readable cell"),
        _workspace("holds no fixture (64 bytes each)")],
    "inplay": _scalars("inplay", 64) + QUERY + [
        ("null_argument", None, dict(ess=None), BPLHIP_EINVAL, "m=2 below 1 or a null argument"),
        ("weight", None, dict(weights=_nan_at((K, 9), 13)), BPLHIP_EINVAL, "weight 4 of market 1 is not finite"),
        QUANTILE,
        ("elapsed", None, dict(elapsed=_arr([0.5, 1.0])), BPLHIP_EINVAL, "elapsed 1 of fixture 1 outside [0, 1)"),
        ("score_beyond", None, dict(fx=dict(home_goals=[0, 3])), BPLHIP_EINVAL,
         "score 3-0 of fixture 1 beyond max_goals=2"),
        ("score_at_zero", None, dict(elapsed=_arr([0.5, 0.0])), BPLHIP_EINVAL, "score 1-0 of fixture 1 at elapsed = 0"),
        ("log_weight", None, dict(log_weights=_nan_at(S, 1)), BPLHIP_EINVAL, "log weight 1 is not finite"),
        _workspace("holds no fixture (96 bytes each)")],
    "slate": _scalars("slate", 0) + QUERY + [
        ("null_argument", None, dict(leg_mean=None), BPLHIP_EINVAL, "m=2 below 1 or a null argument"),
        ("n_slates", None, dict(n_slates=3), BPLHIP_EINVAL, "n_slates=3 out of range [1,m]"),
        ("n_tables", None, dict(n_tables=0), BPLHIP_EINVAL, "n_tables=0 out of range [1,m]"),
        ("table_value", None, dict(tables=_arr([[0] * 9, [0] * 4 + [8] + [0] * 4], u8)), BPLHIP_EINVAL,
         "value 8 of cell 4 of leg table 1, at most 7"),
        ("leg_table", None, dict(leg_table=_arr([0, 2], i32)), BPLHIP_EINVAL, "leg table index out of range at 1"),
        ("start_cover", None, dict(start=_arr([1, 1, 2], i32)), BPLHIP_EINVAL, "start does not cover the 2 fixtures"),
        ("start_order", None, dict(start=_arr([0, 2, 2], i32)), BPLHIP_EINVAL, "start is not increasing at slate 1"),
        ("legs", "solo", dict(fx=dict(home_idx=[0] * 1026, away_idx=[1] * 1026), leg_table=np.zeros(1026, dtype=i32),
                              start=_arr([0, 1025, 1026], i32)), BPLHIP_EINVAL, "slate 0 has 1025 legs, at most 1024"),
        ("total", "solo", dict(fx=dict(home_idx=[0] * 20, away_idx=[1] * 20), leg_table=np.zeros(20, dtype=i32),
                               tables=_arr([[7] * 9, [0] * 9], u8), start=_arr([0, 1, 20], i32)), BPLHIP_EINVAL,
         "slate 1 can total 133, at most 127"),
        QUANTILE, _workspace("does not hold the largest slate (448 bytes)")],
    "ratings": [
        ("n_teams", None, dict(n_teams=0), BPLHIP_EINVAL, "n_teams=0 or n_opponents=3 out of range [1,1024]"),
        ("venue", None, dict(venue=4), BPLHIP_EINVAL, "venue=4 out of range [0,3]"),
        ("max_goals", None, dict(max_goals=64), BPLHIP_EINVAL, "max_goals=64 out of range [0,63]"),
        ("rank_by", None, dict(rank_by=5), BPLHIP_EINVAL, "rank_by=5 out of range [0,4]"),
        ("n_quantiles", None, dict(n_quantiles=17), BPLHIP_EINVAL, "n_quantiles=17 out of range [0,16]"),
        ("no_posterior", "N", {}, BPLHIP_ESTATE, "no posterior set"),
        ("null_argument", None, dict(matches=None), BPLHIP_EINVAL, "a null argument"),
        ("neutral_plain_posterior", "P", dict(venue=3), BPLHIP_EINVAL,
         "venue 3 (neutral) needs a posterior set with predict_set_posterior_venue"),
        ("confederations_plain_posterior", "P", dict(team_conf=_arr([0, 1, 0], u16)), BPLHIP_EINVAL,
         "confederations exactly when the posterior has them"),
        ("no_confederations", "V", dict(opponent_conf=None), BPLHIP_EINVAL,
         "confederations exactly when the posterior has them"),
        ("team_outside", None, dict(teams=_arr([0, 1, 4], u16)), BPLHIP_EINVAL, "team index out of range at 2"),
        ("confederation_outside", "V", dict(team_conf=_arr([0, 1, 2], u16)), BPLHIP_EINVAL,
         "confederation index out of range at 2"),
        ("duplicate_opponent", None, dict(opponents=_arr([1, 2, 2], u16)), BPLHIP_EINVAL, "duplicate opponent at 2"),
        ("only_itself", None, dict(n_opponents=1, opponents=_arr([0], u16)), BPLHIP_EINVAL,
         "team 0 has no opponent other than itself"),
        ("points", None, dict(points=_arr([3.0, np.nan, 0.0])), BPLHIP_EINVAL, "point value 1 is not finite"),
        QUANTILE, _workspace("holds no team (160 bytes each)")],
}


def _merge(first, second):
    both = dict(first, **second)
    if "fx" in first and "fx" in second:
        both["fx"] = dict(first["fx"], **second["fx"])
    return both


# (id, context, tag, overrides, code, message)
CASES = []
for tag, ladder in LADDERS.items():
    name = SYMBOLS[tag][len("bplhip_"):]
    for i, (fault, kind, over, code, text) in enumerate(ladder):
        CASES.append((f"{tag}_{fault}", "P" if kind in (None, "solo") else kind, tag, over, code, f"{name}: {text}"))
        if kind == "solo":
            continue
        # with the next fault that fits: the same context, another argument
        for later, kind2, over2, _, _ in ladder[i + 1:]:
            if kind2 == "solo" or (kind and kind2 and kind != kind2) or (set(over) & set(over2)) - {"fx"}:
                continue
            if "fx" in over and "fx" in over2 and set(over["fx"]) & set(over2["fx"]):
                continue
            CASES.append((f"{tag}_{fault}_and_{later}", kind or kind2 or "P", tag, _merge(over, over2), code,
                          f"{name}: {text}"))
            break


@pytest.mark.parametrize("kind,tag,over,code,message", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_bad_call_reports(contexts, kind, tag, over, code, message):
    ctx, entry = contexts[kind], SYMBOLS[tag]
    a = _raw(ctx, kind, tag, over)
    keep = a.pop("_keep")
    assert len(a) == len(getattr(ctx._lib, entry).argtypes)
    rc = getattr(ctx._lib, entry)(*a.values())
    assert (rc, ctx._lib.bplhip_last_error(ctx._h).decode()) == (code, message)
    del keep
