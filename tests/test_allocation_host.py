"""`best_allocation` on the host (bpl/allocation.py, bpl/neutral_dixon_coles.py), no GPU: every argument error by its
message and before any device call; `from_constraints` on Euro-shaped and World-Cup-shaped constraint sets, on an
unsatisfiable one and twice over; `check` on its output and on keys in any order and form; the keyword's way to the
device call through a stand-in backend; and the facts the GPU tests (tests/test_gpu_allocation.py) rely on, shown by
the restatement alone: it flags no simulation of their cases, every row of the small tables occurs, and the allocated
first round differs from the rank-seeded one."""
from itertools import combinations
from math import comb

import numpy as np
import pytest

import allocation_cases as C
import tournament_ref as R
from bpl import allocation
from test_tournament_host import hand_posterior

EURO_GROUPS = list("ABCDEF")


def euro(m=None):
    m = hand_posterior() if m is None else m
    kw = R.euro_24(list(m.teams))
    kw["best_allocation"] = allocation.from_constraints(kw["groups"], C.EURO_ALLOWED)
    return m, kw


def _raises(match, m, kw, **change):
    with pytest.raises(ValueError, match=match):
        m.simulate_tournament(**{**kw, "num_simulations": 10, **change})
    assert m._predict_ctx is None   # no device context was ever made


def test_argument_errors_by_message():
    m, kw = euro()
    table = kw["best_allocation"]
    some = ("A", "B", "C", "D")
    _raises("best_allocation needs groups and best_of_rest > 0", m, {"knockout": list(m.teams[:8])}, best_allocation=table)
    twos = R.group_format(list(m.teams), 4, 4, 0)
    _raises("best_allocation needs groups and best_of_rest > 0", m, twos, best_allocation=table)
    _raises("best_allocation must be a mapping", m, kw, best_allocation=list(table.items()))
    _raises("best_allocation must be a mapping", m, kw, best_allocation="ABCD")
    _raises("unknown group 'Z'", m, kw, best_allocation={**table, ("A", "B", "C", "Z"): some})
    _raises("unknown group 'Z'", m, kw, best_allocation={**table, some: ("A", "B", "C", "Z")})
    _raises("must name 4 distinct groups", m, kw, best_allocation={**table, ("A", "B", "C"): ("A", "B", "C")})
    _raises("must name 4 distinct groups", m, kw, best_allocation={**table, ("A", "B", "C", "C"): some})
    _raises("is not a permutation of its key", m, kw, best_allocation={**table, some: ("A", "B", "C", "E")})
    _raises("is not a permutation of its key", m, kw, best_allocation={**table, some: ("A", "B", "C", "C")})
    _raises("is not a permutation of its key", m, kw, best_allocation={**table, some: ("A", "B", "C")})
    missing = {k: v for k, v in table.items() if k != some}
    _raises(r"the combination \('A', 'B', 'C', 'D'\) is missing \(14 of 15 rows\)", m, kw, best_allocation=missing)
    _raises(r"the combination \('A', 'B', 'C', 'D'\) appears twice", m, kw,
            best_allocation={**table, ("B", "A", "C", "D"): some})
    _raises("must map a tuple or frozenset of groups", m, kw, best_allocation={**table, "ABCD": some})
    # a group without a place advance + 1: group F has two teams, so five groups have a third place
    t = list(m.teams)
    groups = {**kw["groups"], "F": t[20:22]}
    entries = [(g, p) for g in groups for p in (1, 2)] + [("best", k) for k in range(1, 5)]
    small = {"groups": groups, "advance": 2, "best_of_rest": 4, "knockout": entries}
    five = allocation.from_constraints(groups, [EURO_GROUPS] * 4)
    assert len(five) == 5 and all("F" not in k for k in five)
    _raises("group 'F' has no place 3", m, small, best_allocation={**five, ("A", "B", "C", "F"): ("A", "B", "C", "F")})
    # the table is read by all four methods, and by the World-Cup class, through the one host path
    for method, extra in (("tournament_paths", {}), ("tournament_scenarios", {"fixtures": [0]}), ("tournament_points", {})):
        with pytest.raises(ValueError, match="is missing"):
            getattr(m, method)(**{**kw, "num_simulations": 10, "best_allocation": missing}, **extra)
        assert m._predict_ctx is None


def test_check_returns_one_form_for_any_key_order_and_type():
    groups = {g: [g + str(i) for i in range(4)] for g in EURO_GROUPS}
    table = allocation.from_constraints(groups, C.EURO_ALLOWED)
    assert allocation.check(table, groups, 4) == table and list(allocation.check(table, groups, 4)) == list(table)
    assert list(table) == list(combinations(EURO_GROUPS, 4))
    shuffled = {}
    for i, (k, v) in enumerate(reversed(list(table.items()))):
        shuffled[frozenset(k) if i % 2 else tuple(reversed(k))] = list(v)
    assert allocation.check(shuffled, groups, 4) == table
    assert allocation.check(shuffled, EURO_GROUPS, 4) == table            # a plain sequence of names
    # B == G' is one row
    assert allocation.check({tuple("DCBA"): tuple("BADC")}, list("ABCD"), 4) == {tuple("ABCD"): tuple("BADC")}
    with pytest.raises(ValueError, match="best_of_rest in \\[1, 6\\]"):
        allocation.check(table, groups, 7)
    text = allocation.format_table(table)
    assert len(text.splitlines()) == 16 and "best 4" in text.splitlines()[0] and text.splitlines()[1].startswith("A B C D")


def test_from_constraints_euro_shaped():
    table = allocation.from_constraints(EURO_GROUPS, C.EURO_ALLOWED)
    assert len(table) == comb(6, 4) == 15
    for key, value in table.items():
        assert sorted(value) == sorted(key)
        assert all(g in C.EURO_ALLOWED[k] for k, g in enumerate(value))
    # the lexicographically first matching, slot by slot in group order: worked by hand for two combinations
    assert table[("A", "B", "C", "D")] == ("C", "D", "A", "B")
    assert table[("C", "D", "E", "F")] == ("C", "D", "F", "E")
    # not all rows are the same permutation of their sorted key
    assert len({tuple(sorted(k).index(g) for g in v) for k, v in table.items()}) > 1
    # a second Euro-shaped set: the same rule with the winners met in another order
    turned = allocation.from_constraints(EURO_GROUPS, C.EURO_ALLOWED[::-1])
    assert all(turned[k] == _first_matching(k, C.EURO_ALLOWED[::-1]) for k in turned)


def _first_matching(combo, allowed):
    """The lexicographically first perfect matching by brute force over the permutations in group order."""
    from itertools import permutations

    for perm in permutations(combo):
        if all(g in allowed[k] for k, g in enumerate(perm)):
            return perm
    return None


def test_from_constraints_twelve_groups_eight_slots():
    names = list("ABCDEFGHIJKL")
    allowed = C.cyclic_allowed(names, 8, 12)
    table = allocation.from_constraints(names, allowed)
    assert len(table) == comb(12, 8) == 495 and list(table) == list(combinations(names, 8))
    assert allocation.check(table, names, 8) == table
    for key, value in table.items():
        assert sorted(value) == list(key) and all(g in allowed[k] for k, g in enumerate(value))
    for key in list(table)[::37]:                       # 14 rows against the brute force
        assert table[key] == _first_matching(key, allowed)
    arrays = allocation.device_tables(table, names)
    assert arrays["row_of_mask"].shape == (4096,) and arrays["slots"].shape == (495, 12) and arrays["best"] == 8
    for r, (key, value) in enumerate(table.items()):
        mask = sum(1 << names.index(g) for g in key)
        assert arrays["row_of_mask"][mask] == r
        assert [names[g] for g in np.argsort(arrays["slots"][r])[:8]] == list(value)
        assert (arrays["slots"][r] == 0xFF).sum() == 4


def test_from_constraints_names_the_first_unsatisfiable_combination():
    allowed = [("A", "B", "C", "D", "E"), ("A", "B", "C", "D", "E"), ("A", "B", "F"), ("A", "B", "F")]
    # (A, B, C, D) can be matched; (A, C, D, E) is the first combination whose slots 3 and 4 have only A between them
    with pytest.raises(ValueError, match=r"the combination \('A', 'C', 'D', 'E'\) has no perfect matching"):
        allocation.from_constraints(EURO_GROUPS, allowed)
    with pytest.raises(ValueError, match="unknown group 'Z'"):
        allocation.from_constraints(EURO_GROUPS, [("A", "Z")] * 4)
    with pytest.raises(ValueError, match="at most 12870"):
        allocation.from_constraints(list(range(20)), [list(range(20))] * 10)


def test_from_constraints_is_deterministic():
    names = list("ABCDEFGHIJKLMN")
    allowed = C.cyclic_allowed(names, 4, 4)
    first = allocation.from_constraints(names, allowed)
    again = allocation.from_constraints(tuple(names), [set(a) for a in allowed])
    assert len(first) == comb(14, 4) == 1001
    assert list(first.items()) == list(again.items())


class _Recorder:
    """A stand-in for the device context: records every call's keywords, returns zeros of the right shapes."""

    def __init__(self):
        self.calls = []

    def simulate_tournament(self, team_idx, bracket, n_sims, key, **kwargs):
        self.calls.append(kwargs)
        n, rounds = len(team_idx), len(bracket).bit_length() - 1
        out = {"stage_counts": np.zeros((n, rounds + 2), dtype=np.uint64), "position_counts": np.zeros((n, 8), dtype=np.uint64)}
        if "allocation" in kwargs:
            out["slot_counts"] = np.zeros((kwargs["allocation"]["slots"].shape[1], kwargs["allocation"]["best"]), dtype=np.uint64)
        return out


def test_none_reaches_the_device_call_without_an_allocation():
    m, kw = euro()
    table = kw.pop("best_allocation")
    rec = _Recorder()
    m._device = lambda: rec
    plain = m.simulate_tournament(**kw, num_simulations=10, random_state=1)
    none = m.simulate_tournament(**kw, num_simulations=10, random_state=1, best_allocation=None)
    assert "allocation" not in rec.calls[0] and "allocation" not in rec.calls[1]
    assert sorted(rec.calls[0]) == sorted(rec.calls[1])
    assert "best_slot_count" not in plain and "best_slot_count" not in none
    res = m.simulate_tournament(**kw, num_simulations=10, random_state=1, best_allocation=table)
    sent = rec.calls[2]["allocation"]
    assert {k: v for k, v in rec.calls[2].items() if k != "allocation"}.keys() == rec.calls[0].keys()
    assert sent["best"] == 4 and sent["row_of_mask"].dtype == np.uint16 and sent["row_of_mask"].shape == (64,)
    assert sent["slots"].dtype == np.uint8 and sent["slots"].shape == (15, 6)
    assert res["best_slot_count"].shape == (6, 4) and res["best_slot_count"].dtype == np.int64
    assert res["best_slot_proba"].shape == (6, 4)
    # the checked table and the arrays are part of the checked inputs, for the restatements
    inp = m._tournament_inputs(kw["knockout"], kw["groups"], 2, 4, None, None, None, (3, 1, 0), 10, None,
                               best_allocation={frozenset(k): v for k, v in table.items()})
    assert inp["best_allocation"] == table and (inp["allocation"]["slots"] == sent["slots"]).all()
    assert m._tournament_inputs(kw["knockout"], kw["groups"], 2, 4, None, None, None, (3, 1, 0), 10, None)["allocation"] is None


@pytest.mark.parametrize("mode_id", C.MODE_IDS)
def test_smallest_shape_meets_its_conditions_by_the_restatement_alone(mode_id):
    ref = C.reference("3x3", mode_id)
    assert not ref["flagged"].any()
    assert sorted(np.unique(ref["row"])) == [0, 1, 2]                       # every table row occurs
    ranked = C.ranked_first_round("3x3", mode_id)
    differs = (ranked != ref["bracket"]).any(axis=1)
    assert 0 < differs.sum() < len(differs)                                 # ... and the fill differs from the ranked one
    # the same qualifiers either way, and every non-best entry in its place
    np.testing.assert_array_equal(np.sort(ranked, axis=1), np.sort(ref["bracket"], axis=1))
    fixed = [b for b, e in enumerate(C.shape("3x3")[1]["knockout"]) if e[0] != "best"]
    np.testing.assert_array_equal(ranked[:, fixed], ref["bracket"][:, fixed])
    assert ref["slot_counts"].sum() == 2 * 512 and (ref["slot_counts"].sum(axis=0) == 512).all()


@pytest.mark.parametrize("name,rows", [("euro24", 15), ("wc48", 495), ("14x3", 1001), ("one_row", 1)])
def test_wider_shapes_by_the_restatement_alone(name, rows):
    mode_id = "overall-extra_time" if name == "wc48" else "h2h-redraw" if name == "14x3" else "overall-redraw"
    ref = C.reference(name, mode_id)
    assert not ref["flagged"].any()
    assert len(C.shape(name)[1]["best_allocation"]) == rows
    if name in ("euro24", "one_row"):
        assert len(np.unique(ref["row"])) == rows                           # every row occurs
    else:
        assert len(np.unique(ref["row"])) > 100
