"""`best_allocation` on the device (csrc/dc_tournament_body.hip.inc and csrc/dc_tournament_sim_play.hip.inc: the
bracket fill by the set of groups the best of the rest come from) against the numpy restatement
(tests/allocation_ref.py), exactly: the smallest discriminating shape in all four modes; the per-simulation records
of tournament_paths with and without a table, derived through the table with numpy alone; the one-row table that is a
rank-free format in disguise; the Euro shape with every one of its 15 rows; masks of 12 and 14 bits with hosts; the
four entry points against each other and against their restatements; and the independence of the chunk.

The shapes, seeds and tables are tests/allocation_cases.py's; tests/test_allocation_host.py shows without a GPU that
the restatement flags no simulation of any of them and that the small tables' rows all occur, so every comparison is
plain equality."""
import numpy as np
import pytest

import allocation_cases as C
import allocation_ref as A
import knockout_ref as K
import tournament_points_ref as G
import tournament_ref as R
import tournament_scenarios_ref as S
from bpl.base import _prng_key, points_axis
from bpl.neutral_dixon_coles import tournament_result

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _against_restatement(name, mode_id):
    """simulate_tournament(return_stages=True) under the case's table against the restatement: every key."""
    m, common, inp, _ = C.call(name, mode_id)
    ref = C.reference(name, mode_id)
    assert not ref["flagged"].any()
    res = m.simulate_tournament(return_stages=True, **common)
    want = tournament_result(inp, ref)
    keys = ["stage", "round_proba", "group_position_proba", "best_slot_count", "best_slot_proba"]
    keys += ["decided_proba", "decided"] if inp["knockout_rule"] == "extra_time" else []
    assert set(res) == set(keys) | {"teams"}
    for k in keys:
        assert res[k].shape == want[k].shape and res[k].dtype == want[k].dtype, k
        np.testing.assert_array_equal(res[k], want[k], err_msg=k)
    groups, best = len(inp["group_names"]), inp["best_of_rest"]
    assert res["best_slot_count"].shape == (groups, best) and res["best_slot_count"].dtype == np.int64
    np.testing.assert_array_equal(res["best_slot_count"].sum(axis=0), inp["num_simulations"])
    return res, ref, inp


# ---- 1. the smallest discriminating shape: 3 groups of 3, 2 of 3 thirds, 3 rows, N = 512
@pytest.mark.parametrize("mode_id", C.MODE_IDS)
def test_smallest_shape_against_restatement(mode_id):
    res, ref, inp = _against_restatement("3x3", mode_id)
    assert inp["num_simulations"] == 512 and len(inp["best_allocation"]) == 3
    assert sorted(np.unique(ref["row"])) == [0, 1, 2]                        # every table row occurs
    assert (C.ranked_first_round("3x3", mode_id) != ref["bracket"]).any()    # and the fill is not the ranked one
    # the device under the table is not the device without it
    m, common, _, _ = C.call("3x3", mode_id, allocated=False)
    plain = m.simulate_tournament(return_stages=True, **common)
    assert "best_slot_count" not in plain and (plain["stage"] != res["stage"]).any()
    np.testing.assert_array_equal(plain["group_position_proba"], res["group_position_proba"])


# ---- 2. the records with and without a table: numpy alone, no restatement
@pytest.mark.parametrize("mode_id", ["overall-redraw", "h2h-extra_time"])
def test_records_differ_only_in_the_allocated_entries(mode_id):
    m, common, inp, _ = C.call("euro24", mode_id, n_sims=1500)
    _, plain_kw, _, _ = C.call("euro24", mode_id, allocated=False, n_sims=1500)
    with_table = m.tournament_paths(return_records=True, **common)
    without = m.tournament_paths(return_records=True, **plain_kw)
    for k in ("position", "group_outcome"):
        np.testing.assert_array_equal(with_table[k], without[k], err_msg=k)
    np.testing.assert_array_equal(with_table["stage"] >= 1, without["stage"] >= 1)      # the same qualifiers
    # the first round through the table, from the DEFAULT run's positions and qualifiers
    N, n, nb = 1500, len(inp["teams"]), 16
    names, group = inp["group_names"], inp["group"].astype(np.int64)
    position, through = without["position"].astype(np.int64), without["stage"] >= 1
    knockout = C.shape("euro24")[1]["knockout"]
    table = inp["best_allocation"]
    want = np.full((N, nb), -1, dtype=np.int64)
    for j in range(N):
        thirds = [t for t in range(n) if position[j, t] == 2 and through[j, t]]
        combo = tuple(sorted(names[group[t]] for t in thirds))
        order = table[combo]
        for b, (ref, place) in enumerate(knockout):
            g = order[place - 1] if ref == "best" else ref
            want[j, b] = next(t for t in range(n) if names[group[t]] == g and
                              position[j, t] == (2 if ref == "best" else place - 1))
    first = with_table["pair"][:, :nb // 2].reshape(N, nb).astype(np.int64)
    np.testing.assert_array_equal(first, want)
    # every non-best entry sits where it sat; the best entries moved in some simulation
    default_first = without["pair"][:, :nb // 2].reshape(N, nb).astype(np.int64)
    fixed = [b for b, e in enumerate(knockout) if e[0] != "best"]
    best = [b for b, e in enumerate(knockout) if e[0] == "best"]
    np.testing.assert_array_equal(first[:, fixed], default_first[:, fixed])
    assert (first[:, best] != default_first[:, best]).any()
    np.testing.assert_array_equal(np.sort(first[:, best], axis=1), np.sort(default_first[:, best], axis=1))


# ---- 3. a one-row table is a format without ranks: all four seconds "best of the rest" = advance 2
@pytest.mark.parametrize("mode_id", C.MODE_IDS)
def test_one_row_table_equals_the_ranked_free_format(mode_id):
    m, common, inp, _ = C.call("one_row", mode_id)
    names = inp["group_names"]
    same = dict(common, advance=2, best_of_rest=0,
                knockout=[(names[e[1] - 1], 2) if e[0] == "best" else e for e in common["knockout"]])
    del same["best_allocation"]
    extra = {"tournament_scenarios": {"fixtures": [0, 7]}}
    for method in ("simulate_tournament", "tournament_paths", "tournament_scenarios", "tournament_points"):
        a = getattr(m, method)(**common, **extra.get(method, {}))
        b = getattr(m, method)(**same, **extra.get(method, {}))
        shared = [k for k in ("round_proba", "group_position_proba", "decided_proba") if k in a]
        assert "round_proba" in shared and [k for k in shared if k in b] == shared
        for k in shared:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{method} {k}")
    sim = m.simulate_tournament(**common)
    np.testing.assert_array_equal(sim["best_slot_count"], inp["num_simulations"] * np.eye(4, dtype=np.int64))


# ---- 4. the Euro shape: 15 rows, every one occurs
def test_euro_shape_against_restatement():
    res, ref, inp = _against_restatement("euro24", "overall-redraw")
    assert inp["num_simulations"] == 4096 and len(np.unique(ref["row"])) == 15
    # a third never takes a slot its group is barred from
    barred = np.array([[g not in C.EURO_ALLOWED[k] for k in range(4)] for g in inp["group_names"]])
    assert (res["best_slot_count"][barred] == 0).all() and (res["best_slot_count"].sum(axis=1) > 0).all()


# ---- 5. wide masks: 12 groups (495 rows) and 14 groups (1001 rows, bits up to 13), with hosts
@pytest.mark.parametrize("name,mode_id", [("wc48", "overall-extra_time"), ("14x3", "h2h-redraw")])
def test_wide_masks_against_restatement(name, mode_id):
    res, ref, inp = _against_restatement(name, mode_id)
    assert inp["host"].sum() == 2 and inp["num_simulations"] == 2000
    assert len(inp["best_allocation"]) == {"wc48": 495, "14x3": 1001}[name]
    assert res["best_slot_count"][-1].sum() > 0            # the last group's bit was part of a mask


# ---- 6. the four entry points under one table
@pytest.mark.parametrize("mode_id", C.MODE_IDS)
def test_four_entry_points_agree_under_a_table(mode_id, monkeypatch):
    name = "3x3"
    m, common, inp, dev = C.call(name, mode_id)
    _, plain, _, _ = C.call(name, mode_id, allocated=False)
    sim = m.simulate_tournament(**common)
    paths = m.tournament_paths(**common)
    keys, caps = [0, 4, 8], [1, 2, 1]
    scen = m.tournament_scenarios(fixtures=keys, margin_cap=caps, return_records=True, **common)
    pts = m.tournament_points(**common)
    for other, what in ((paths, "paths"), (scen, "scenarios"), (pts, "points")):
        np.testing.assert_array_equal(other["round_proba"], sim["round_proba"], err_msg=what)
        assert ("decided_proba" in other) == ("decided_proba" in sim)
        if "decided_proba" in sim:
            np.testing.assert_array_equal(other["decided_proba"], sim["decided_proba"], err_msg=what)
    np.testing.assert_array_equal(paths["group_position_proba"], sim["group_position_proba"])
    np.testing.assert_array_equal(pts["group_position_proba"], sim["group_position_proba"])
    # the rest tables rank the thirds: the table does not touch them, nor the group tables
    pts_plain = m.tournament_points(**plain)
    for k in ("rest_count", "rest_through_count", "rest_rank_count", "team_points_count", "team_place_count",
              "place_points_count", "place_gap_count"):
        np.testing.assert_array_equal(pts[k], pts_plain[k], err_msg=k)
    assert (pts["team_target_count"] != pts_plain["team_target_count"]).any()
    if inp["knockout_rule"] != "extra_time":
        return
    # under extra time the restatements of the two run on knockout_ref.first_round: substituted, they are
    # allocation restatements
    monkeypatch.setattr(K, "first_round", A.first_round)
    tables, key = R.model_tables(m), _prng_key(C.SEED)
    h2h, pair = common["tiebreak"] == "head_to_head", dev["kwargs"].get("pair_init")
    sref = S.simulate(tables, inp, key, np.asarray(keys), caps, head_to_head=h2h, pair_init=pair)
    assert not sref["flagged"].any()
    np.testing.assert_array_equal(scen["scenario"], sref["scenario"])
    np.testing.assert_array_equal(scen["target_set"], sref["target_set"])
    for k, v in S.counts(sref, inp, keys, caps).items():
        np.testing.assert_array_equal(scen[k], v, err_msg=k)
    pref = G.simulate(tables, inp, key, head_to_head=h2h, pair_init=pair)
    assert not pref["flagged"].any()
    for k, v in G.counts(pref, inp, int(pts["points"][0]), pts["points"].size, gd_cap=3).items():
        np.testing.assert_array_equal(pts[k], v, err_msg=k)


# ---- 7. the chunk: integer tables, best_slot_count included, do not depend on it, nor on the run
def test_chunking_and_determinism():
    m, common, inp, dev = C.call("3x3", "h2h-extra_time", n_sims=203)         # no multiple of 7 or 64
    ctx = m._device()
    first = ctx.simulate_tournament(*dev["args"], **dev["kwargs"])
    again = ctx.simulate_tournament(*dev["args"], **dev["kwargs"])
    assert first["slot_counts"].sum() == 2 * 203
    for k in first:
        np.testing.assert_array_equal(again[k], first[k], err_msg=k)
    pmin, bins = points_axis(inp["table"][:, 0], inp["fix_p"], inp["fix_q"], inp["points"])
    runs = {"tournament_paths": {}, "tournament_scenarios": dict(key_fixture=[0, 4], key_cap=[1, 2]),
            "tournament_points": dict(points_min=pmin, n_bins=bins, gd_cap=2)}
    for method, extra in runs.items():
        one = getattr(ctx, method)(*dev["args"], chunk_sims=0, **extra, **dev["kwargs"])
        np.testing.assert_array_equal(one["decided_counts"], first["decided_counts"], err_msg=method)
        if "stage_counts" in one:
            np.testing.assert_array_equal(one["stage_counts"], first["stage_counts"], err_msg=method)
        for chunk in (1, 7, 64):
            other = getattr(ctx, method)(*dev["args"], chunk_sims=chunk, **extra, **dev["kwargs"])
            assert set(other) == set(one)
            for k in one:
                np.testing.assert_array_equal(other[k], one[k], err_msg=f"{method} {k} chunk {chunk}")
    # the table is gone from the context after each call: a call without one is the ranked fill again
    plain = {k: v for k, v in dev["kwargs"].items() if k != "allocation"}
    ranked = ctx.simulate_tournament(*dev["args"], **plain)
    assert "slot_counts" not in ranked and (ranked["stage_counts"] != first["stage_counts"]).any()
