"""The weighted-draw scan (live_weights), search (search_scan; csrc/dc_live.hip.h) and weighted quantiles
(inplay_summary; csrc/dc_inplay.hip.h) on the device across the draw counts, weight rows and simulation counts of
tests/live_weight_cases.py, through the eight live entry points and predict_in_play.

With `log_weights` alone (no `in_play`; `reweight=False` for predict_in_play) the device's L is the caller's row.
On a row of 0.0 and -1e4 the weights are exactly 1 and 0, every scan value is an integer and W = K: the draw of
every simulation and every weighted quantile have one right answer, bit for bit.  Those cases take NO tolerance and
excuse NO simulation -- live_ref.resample's and inplay_ref's flags are not consulted for them.  The inexact rows and
the states in force are compared off the flagged simulations, at most 1 % of a case (tests/test_gpu_live.py's cap;
tests/test_live_weight_cases_host.py holds the seeds to it without a GPU), with `ess` and `log_evidence` within that
file's relative 1e-9 and L / L0 within its `_loglik_gate`; mean and sd of predict_in_play within inplay_ref.gates."""
import numpy as np
import pytest

import allocation_cases as AC
import inplay_ref as IR
import live_cases as LC
import live_ref as LR
import live_weight_cases as WC
import loglik_ref as KR
import paths_ref as PR
import tournament_live_cases as TC
import tournament_live_queries_ref as QR
import tournament_points_ref as TP
import tournament_scenarios_ref as TS
from bpl import NeutralDixonColesMatchPredictor
from bpl import markets as MK
from bpl import scenarios as _scenarios
from bpl.base import (_prng_key, check_levels, leverage_from_counts, leverage_targets, points_axis,
                      points_from_counts)
from test_gpu_inplay import _extremes_are_exact, _markets
from test_gpu_live import _loglik_gate
from test_gpu_live_queries import LEVELS, QUERIES, TARGETS, TIEBREAKS, _check, _season
from test_gpu_season import _posterior
from test_tournament_host import hand_posterior

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


_MODELS = {}


def _model(tag, S, make):
    """One posterior per (tag, S) at a time: the tests come grouped by S, the one before is let go."""
    if _MODELS.get(tag, (None, None))[0] != S:
        old = _MODELS.pop(tag, None)
        if old is not None and old[1]._predict_ctx is not None:
            old[1]._predict_ctx.close()
            old[1]._predict_ctx = None
        _MODELS[tag] = (S, make())
    return _MODELS[tag][1]


def _against_the_oracle(tag, draw, ess, log_evidence, name, S, N, seed):
    """The draw of every simulation, ess and log_evidence of a call with the row `name` alone against
    live_ref.weights and live_ref.resample: exact rows bit for bit and whole, inexact rows off the flags."""
    w = WC.weights(name, S)
    s, flagged = LR.resample(w["C"], N, _prng_key(seed))
    assert draw.dtype == np.int32 and draw.shape == (N,)
    if name in WC.EXACT_ROWS:
        K = WC.live_count(name, S)
        differ = int((draw != s).sum())
        print(f"{tag} S={S} {name} N={N}: {differ} of {N} simulations differ (exact, K={K})")
        np.testing.assert_array_equal(draw, s)
        assert ess == float(K) and log_evidence == 0.0, (ess, K, log_evidence)
    else:
        keep = ~flagged
        differ = int((draw[keep] != s[keep]).sum())
        print(f"{tag} S={S} {name} N={N}: {differ} of {N} simulations differ off the flagged, flagged "
              f"{int(flagged.sum())} ({flagged.mean():.4%})")
        assert flagged.sum() <= 0.01 * N
        np.testing.assert_array_equal(draw[keep], s[keep])
        assert abs(ess - w["ess"]) <= 1e-9 * w["ess"] and log_evidence == 0.0, (ess, w["ess"], log_evidence)


# ---- a. the season simulator: every (S, row, N) of the table
@pytest.mark.parametrize("S,name", WC.ROW_CASES, ids=lambda v: str(v))
def test_season_draws_across_the_table(S, name):
    m = _model("three", S, lambda: _posterior("basic", T=3, S=S, seed=6))
    lw = np.array(WC.log_weights(name, S))
    for N in WC.sim_counts(S):
        seed = WC.SEED + N
        res = m.simulate_season(["t00"], ["t01"], num_simulations=N, random_state=seed, log_weights=lw,
                                return_tables=True, return_weights=True)
        _against_the_oracle("season", res["draw"], res["ess"], res["log_evidence"], name, S, N, seed)
        np.testing.assert_array_equal(res["log_weights"], lw - lw.max())     # the device's L is the caller's row
        assert res["points"].shape == (N, 2)


# ---- b. states in force: live_loglik's partial last workgroup, then the scan and the search on the DEVICE's L
STATE_DRAWS = (1, 63, 64, 65, 255, 256, 257, 513, 4161)


@pytest.mark.parametrize("kind", ["basic", "extended"])
@pytest.mark.parametrize("S", STATE_DRAWS)
def test_states_in_force(S, kind):
    N, seed = 4099, WC.SEED
    m = _posterior(kind, T=LC.T, S=S, seed=4)
    home, away = LC.fixtures(m)
    ipr = m._in_play_inputs(LC.in_play(m))
    assert len(LC.STATES) == 6 and ipr[0].size == 6
    n = LC.T
    raw = m._device().simulate_season_live(*m._team_indices(home, away), np.arange(n), np.zeros((n, 3)), (3, 1, 0), N,
                                           _prng_key(seed), in_play=ipr, reweight=True, return_tables=True,
                                           return_weights=True)
    assert raw["L"].shape == raw["L0"].shape == (S,) and raw["draw"].shape == (N,)
    total, gate = _loglik_gate(m, ipr)
    e0 = np.abs(raw["L0"] - total) / gate
    e1 = np.abs(raw["L"] - total) / (gate + IR.EPS * np.abs(total))
    print(f"S={S} {kind}: L0 error / gate {e0.max():.3e}, L error / gate {e1.max():.3e}")
    assert e0.max() <= 1.0 and e1.max() <= 1.0
    np.testing.assert_array_equal(raw["L"], raw["L0"])                       # reweight without log_weights
    # the scan and the search alone: the restatement on the device's own L and L0
    w = LR.weights(raw["L"], raw["L0"])
    s, flagged = LR.resample(w["C"], N, _prng_key(seed))
    keep = ~flagged
    e_ess = abs(float(raw["ess"]) - w["ess"]) / w["ess"]
    e_ev = abs(float(raw["log_evidence"]) - w["log_evidence"]) / abs(w["log_evidence"])
    print(f"S={S} {kind}: {int((raw['draw'][keep] != s[keep]).sum())} of {N} simulations differ off the flagged, "
          f"flagged {int(flagged.sum())}; ess relative error {e_ess:.3e}, log_evidence relative error {e_ev:.3e}")
    assert flagged.sum() <= 0.01 * N
    np.testing.assert_array_equal(raw["draw"][keep], s[keep])
    assert e_ess <= 1e-9 and e_ev <= 1e-9


# ---- c. the other seven entries
ENTRY_DRAWS = (65, 4161)                 # two search passes with a window of one; three passes
ENTRY_ROWS = ("tail_zero", "generic")
ENTRY_N = 4099
CHUNK = 1024                             # five chunks, the last of three simulations: j0 = 1024, ..., 4096
SCEN_KEYS, SCEN_CAPS = (0, 4, 8), (1, 2, 1)


def _season_query_raw(m, which, home, away, N, seed, lw, tiebreak):
    """A season query through the raw binding (the public method's own steps) with CHUNK simulations per pass."""
    ip, lwc, hh, aa = m._live_inputs(home, away, None, lw)
    h, a, table_idx, table, points, n_sims, h2h, pair = m._season_h2h_inputs(hh, aa, N, LC.TABLE, None, (3, 1, 0),
                                                                             tiebreak, None)
    _, masks = leverage_targets(TARGETS, table_idx.size)
    live = dict(in_play=ip, reweight=True, log_weights=lwc, chunk_sims=CHUNK)
    if h2h:
        live.update(pair_init=pair, head_to_head=True)
    ctx = m._device()
    args = (h, a, table_idx, table, points, n_sims, _prng_key(seed), masks)
    if which == "leverage":
        raw = ctx.match_leverage_live(*args, **live)
        out = leverage_from_counts(raw["outcome"], raw["target"], raw["joint"], n_sims)
    elif which == "points":
        slot = np.full(len(m.teams), -1, dtype=np.int64)
        slot[table_idx.astype(np.int64)] = np.arange(table_idx.size)
        points_min, n_bins = points_axis(table[:, 0], slot[h], slot[a], points)
        raw = ctx.season_points_live(*args, points_min, n_bins, **live)
        out = points_from_counts(raw["team_points"], raw["team_target"], raw["position_points"], raw["gap"],
                                 points_min, n_sims, check_levels(LEVELS))
    else:
        keys, caps = _scenarios.check_keys(list(SCEN_KEYS), list(SCEN_CAPS), h.size)
        raw = ctx.season_scenarios_live(*args, keys, caps, **live)
        out = _scenarios.scenario_from_counts(raw["scenario"], raw["joint"], n_sims)
    out.update(ess=float(raw["ess"]), log_evidence=float(raw["log_evidence"]))
    return out


@pytest.mark.parametrize("tiebreak", TIEBREAKS)
@pytest.mark.parametrize("name", ENTRY_ROWS)
@pytest.mark.parametrize("S", ENTRY_DRAWS)
def test_season_queries_are_the_simulator_chunk_by_chunk(S, name, tiebreak):
    m = _model("six", S, lambda: _posterior("basic", T=LC.T, S=S, seed=4))
    home, away = LC.fixtures(m)
    lw = np.array(WC.log_weights(name, S))
    N, seed = ENTRY_N, WC.SEED + ENTRY_N
    kw = dict(num_simulations=N, random_state=seed, current_table=LC.TABLE, tiebreak=tiebreak, log_weights=lw)
    sim, hg, ag = _season(m, home, away, **kw)
    _against_the_oracle(f"season {tiebreak}", sim["draw"], sim["ess"], sim["log_evidence"], name, S, N, seed)
    for which in QUERIES:
        chunked = _season_query_raw(m, which, home, away, N, seed, lw, tiebreak)
        _check(which, chunked, sim, hg, ag, N, keys=SCEN_KEYS, caps=SCEN_CAPS)
    # and the public methods (one chunk) return the same tables
    whole = m.match_leverage(home, away, targets=TARGETS, **kw)
    _check("leverage", whole, sim, hg, ag, N)


def _cup(shape, S, name, mode_id, N, seed):
    """(model, the public keywords, the checked inputs) of tests/tournament_live_cases.py's shape C (knockout only)
    or its shape A without matches in play, rebuilt at S draws, under the row `name` alone."""
    if shape == "C":
        m = _model("cupC", S, lambda: hand_posterior(NeutralDixonColesMatchPredictor, T=8, S=S, seed=73))
        kw, hosts = {"knockout": list(m.teams)}, ["t03"]
    else:
        m = _model("cupA", S, lambda: hand_posterior(NeutralDixonColesMatchPredictor, T=8, S=S, seed=71))
        _, kw, hosts, _, _, _ = TC.shape("A")
    lw = np.array(WC.log_weights(name, S))
    rounds = len(kw["knockout"]).bit_length() - 1
    tiebreak, rule = AC.mode(mode_id, rounds)
    common = dict(num_simulations=N, random_state=seed, hosts=hosts, tiebreak=tiebreak, **kw, **rule)
    if "groups" in kw:
        common["current_table"] = TC.current_table("A")
    inp, _ = m._tournament_call(
        kw["knockout"], kw.get("groups"), kw.get("advance", 2), kw.get("best_of_rest", 0), kw.get("group_fixtures"),
        common.get("current_table"), hosts, (3, 1, 0), N, seed, None, tiebreak, None,
        rule.get("knockout_rule", "redraw"), rule.get("legs"), rule.get("extra_time_scale", 1 / 3), rule.get("shootout"),
        rule.get("away_goals", False), None, None, lw, True)
    return m, dict(common, in_play=None, reweight=True, log_weights=lw), inp


def _same(a, b, keys):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.parametrize("mode_id", ["overall-redraw", "overall-extra_time"])
@pytest.mark.parametrize("name", ENTRY_ROWS)
@pytest.mark.parametrize("S", ENTRY_DRAWS)
def test_knockout_only_tournament_and_its_queries(S, name, mode_id):
    N, seed = ENTRY_N, WC.SEED + ENTRY_N
    m, common, inp = _cup("C", S, name, mode_id, N, seed)
    assert inp["group"] is None and inp["in_play"][0].size == 0
    sim = m.simulate_tournament(return_stages=True, **common)
    _against_the_oracle(f"tournament {mode_id}", sim["draw"], sim["ess"], sim["log_evidence"], name, S, N, seed)
    paths = m.tournament_paths(return_records=True, **common)
    _same(paths, sim, ["round_proba", "ess", "log_evidence", "stage", "draw"]
          + [k for k in ("decided_proba", "decided") if k in sim])
    mine = PR.counts(paths, QR.shown(inp, inp["in_play"]))
    for k in ("stage_count", "advance_count", "meet_count"):
        np.testing.assert_array_equal(paths[k], mine[k], err_msg=k)
    # without groups there is nothing to key on or to count points of: the other two queries say so
    for method, extra in (("tournament_scenarios", {"fixtures": [0]}), ("tournament_points", {})):
        with pytest.raises(ValueError):
            getattr(m, method)(**common, **extra)


CUP_KEYS, CUP_CAPS = (65, 3), (1, 1)     # an ordinary fixture in the second block of 64 and one in the first


@pytest.mark.parametrize("mode_id", ["overall-redraw", "h2h-extra_time"])
@pytest.mark.parametrize("name", ENTRY_ROWS)
@pytest.mark.parametrize("S", ENTRY_DRAWS)
def test_grouped_tournament_queries_are_the_simulator(S, name, mode_id):
    """The knockout-only shape reaches tournament_paths alone; tournament_scenarios and tournament_points need
    groups, so they are held to the simulator on shape A's groups and fixtures without matches in play."""
    N, seed = ENTRY_N, WC.SEED + ENTRY_N
    m, common, inp = _cup("A", S, name, mode_id, N, seed)
    F = inp["fix_p"].size
    assert inp["group"] is not None and F == 66 and inp["in_play"][0].size == 0
    cat = QR.shown(inp, inp["in_play"])
    sim = m.simulate_tournament(return_stages=True, **common)
    _against_the_oracle(f"grouped tournament {mode_id}", sim["draw"], sim["ess"], sim["log_evidence"], name, S, N, seed)
    shared = [k for k in ("round_proba", "group_position_proba", "decided_proba", "ess", "log_evidence") if k in sim]
    paths = m.tournament_paths(return_records=True, **common)
    _same(paths, sim, shared + ["stage", "draw"] + (["decided"] if "decided" in sim else []))
    mine = PR.counts(paths, cat)
    for k in mine:
        if k in paths:
            np.testing.assert_array_equal(paths[k], mine[k], err_msg=k)
    scen = m.tournament_scenarios(return_records=True, fixtures=list(CUP_KEYS), margin_cap=list(CUP_CAPS), **common)
    _same(scen, sim, [k for k in shared if k != "group_position_proba"])
    _same(scen, paths, ["draw"])
    stride, _ = TS.strides(CUP_CAPS)
    want = sum(paths["group_outcome"][:, f].astype(np.int64) * stride[q] for q, f in enumerate(CUP_KEYS))
    np.testing.assert_array_equal(scen["scenario"], want)
    np.testing.assert_array_equal(scen["target_set"], QR.target_set(paths["stage"], paths["position"], inp["rounds"]))
    mine = TS.counts(scen, cat, CUP_KEYS, CUP_CAPS)
    for k in ("scenario_count", "joint_count"):
        np.testing.assert_array_equal(scen[k], mine[k], err_msg=k)
    pts = m.tournament_points(**common)
    _same(pts, sim, shared)
    points_min, n_bins = points_axis(inp["table"][:, 0], cat["fix_p"], cat["fix_q"], inp["points"])
    np.testing.assert_array_equal(pts["points"], points_min + np.arange(n_bins))
    mine = TP.counts(TP.records_from_paths(paths, cat), cat, points_min, n_bins)
    for k in ("team_points_count", "team_target_count", "team_place_count", "place_points_count", "place_gap_count"):
        np.testing.assert_array_equal(pts[k], mine[k], err_msg=k)


# ---- d. predict_in_play with designed weights
QUANTILE_DRAWS = (2, 64, 255, 256, 257, 511, 512, 513, 768, 12288)
QS = (0.0, 0.25, 0.5, 0.75, 1.0, 0.3)
RANK_ROWS = ("head", "tail", "middle", "alternate", "landing", "equal")
THREADS = 256   # csrc/dc_inplay.hip.h INPLAY_THREADS: the scan's segments of the SORTED order


def _live_ranks(row, S):
    """bool [S]: which positions of the sorted order carry weight 1, or None when S has no room for the row.  From
    eight draws on K, the number of live draws, is a multiple of 4, so q K is an integer at q = 0.25, 0.5, 0.75 and the
    crossing C_i >= q W is met with EQUALITY."""
    per = -(-S // THREADS)
    seg = [(lo, min(lo + per, S)) for lo in range(0, S, per)]
    live = np.ones(S, dtype=bool)
    run = per + 1 if S >= per + 5 else 1           # a whole segment of the sorted order and one position more
    if row == "head":
        live[:run] = False
    elif row == "tail":
        live[S - run:] = False
    elif row == "middle":                          # an interior thread's whole segment and a position on each side
        if len(seg) < 5:
            return None
        lo, hi = seg[len(seg) // 2]
        live[lo - 1:hi + 1] = False
    elif row == "alternate":
        live[0::2] = False
    elif row == "landing":
        # m live positions end ON the last position of segment i, segment i + 1 is dead, m live positions follow:
        # at q = 0.5 the target m = C at the end of segment i, and threads i + 1, i + 2 start with before == target
        if len(seg) < 4:
            return None
        i = len(seg) // 2
        end, after = seg[i][1], seg[i + 1][1]
        m = min(end, S - after) // 2 * 2
        if m < 2:
            return None
        live[:] = False
        live[end - m:end] = True
        live[after:after + m] = True
    elif row != "equal":
        raise KeyError(row)
    if row not in ("equal", "landing") and S >= 8:
        # K down to a multiple of 4: the head row grows its dead run, the others lose their top live positions
        extra = int(live.sum()) % 4
        at = np.nonzero(live)[0]
        live[at[:extra] if row == "head" else at[at.size - extra:]] = False
    return live if live.any() else None


def _weighted_inverted_cdf(val, w, qs):
    """The documented rule written out on the values' own stable sort: the first sorted position whose running
    weight reaches q W; q = 1 is the maximum of ALL draws, q = 0 (C_0 >= 0) the minimum of ALL draws."""
    order = np.argsort(val, kind="stable")
    srt, C = val[order], np.cumsum(w[order])
    return np.array([srt[-1] if q >= 1.0 else srt[np.nonzero(C >= q * C[-1])[0][0]] for q in qs])


@pytest.mark.parametrize("S", QUANTILE_DRAWS)
def test_weighted_quantiles_of_designed_rows(S):
    m = KR.hand_model("basic", S=S, T=6, seed=S)
    d = IR.with_states(KR.hand_data(m, n=1, seed=61), 15, seed=62)
    mk = {"over_2.5": MK.total_over(2.5), "goals_home": MK.goals("home")}
    first = m.predict_in_play(d, mk, max_goals=15, quantiles=QS, reweight=False, return_draws=True)
    values = first["draws"][:, :, 0]                                   # [S, 2]
    order = np.argsort(values[:, 0], kind="stable")
    base = IR.predict_in_play(m, d, mk, 15, QS, reweight=False)
    per = -(-S // THREADS)
    done = []
    for row in RANK_ROWS:
        ranks = _live_ranks(row, S)
        if ranks is None:
            continue
        live = np.zeros(S, dtype=bool)
        live[order] = ranks                                            # by sorted rank of the FIRST market
        K = int(live.sum())
        if S >= 8 and row != "equal":
            assert K % 4 == 0
        if row == "landing":
            # the q = 0.5 crossing is the last position of a thread's segment, and a dead segment follows it
            at = np.nonzero(ranks)[0][K // 2 - 1]
            assert (at + 1) % per == 0 and not ranks[at + 1:at + 1 + per].any()
        lw = np.where(live, 0.0, WC.DEAD) if row != "equal" else np.full(S, 3.5)
        got = m.predict_in_play(d, mk, max_goals=15, quantiles=QS, reweight=False, log_weights=lw, return_draws=True)
        assert got["draws"].tobytes() == first["draws"].tobytes()
        w = live.astype(np.float64)
        for k in range(2):
            val = values[:, k]
            want = _weighted_inverted_cdf(val, w, QS)
            # the same answer by numpy's own rule on the live subset; the extremes are those of ALL draws
            inner = np.quantile(val[live], QS, method="inverted_cdf")
            inner[0], inner[4] = val.min(), val.max()
            assert want.tobytes() == inner.tobytes(), (row, k)
            differ = int((got["quantile"][k, :, 0] != want).sum())
            print(f"S={S} {row} K={K} market {k}: {differ} of {len(QS)} quantiles differ")
            assert got["quantile"][k, :, 0].tobytes() == want.tobytes(), (row, k, got["quantile"][k, :, 0], want)
        _extremes_are_exact(got)
        assert got["ess"][0] == float(K), (row, got["ess"][0], K)
        # mean and sd of the live subset, within the in-play gates of this row's weights
        ref = dict(base)
        ref.update(IR.summarise(base["draws"], base["draw_log_evidence"], QS, False, lw))
        gate = IR.gates(ref)
        sub = values[live]
        e_mean = np.abs(got["mean"][:, 0] - sub.mean(axis=0)) / gate["mean"][:, 0]
        e_sd = np.abs(got["sd"][:, 0] - sub.std(axis=0)) / gate["sd"][:, 0]
        print(f"S={S} {row} K={K}: mean error / gate {e_mean.max():.3e}, sd error / gate {e_sd.max():.3e}")
        assert e_mean.max() <= 1.0 and e_sd.max() <= 1.0
        done.append(row)
    # only two draws have no room for the rows built on whole segments
    assert done == (["head", "tail", "alternate", "equal"] if S == 2 else list(RANK_ROWS))


@pytest.mark.parametrize("S", [256, 512])
def test_equal_weights_at_multiples_of_the_workgroup_are_numpys_inverted_cdf(S):
    """tests/test_gpu_inplay.py's equal-weights check at the sizes where every q S is an integer and lands on the
    last position of a thread's segment (per = 1 and 2)."""
    m = KR.hand_model("extended", S=S, T=8, seed=41)
    d = IR.with_states(KR.hand_data(m, n=20, seed=42), 15, seed=43)
    qs = (0.25, 0.5, 0.75)
    for q in qs:
        assert (q * S) % (S // THREADS) == 0
    r = m.predict_in_play(d, _markets(15), quantiles=qs, reweight=False, return_draws=True)
    want = np.quantile(r["draws"], qs, axis=0, method="inverted_cdf").transpose(1, 0, 2)
    print(f"S={S}: {int((r['quantile'] != want).sum())} of {want.size} quantiles differ")
    assert r["quantile"].tobytes() == np.ascontiguousarray(want).tobytes()
    assert (r["ess"] == float(S)).all()
