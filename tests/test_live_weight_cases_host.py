"""Every statement of tests/live_weight_cases.py, kept true without a GPU: the lane-by-lane emulation of
search_scan returns #{s : C[s] < target} for every case and every simulation, in the pass counts the table claims;
live_weights' `per` and segment counts are the ones claimed; an exact (0/1-weight) row gives weights in {0, 1}, an
integer scan, ess = K and log evidence 0.0, never selects a dead draw and uses every live draw floor or ceil of
N / K times; and the restatement flags at most 1 % of the simulations of every inexact case (the cap of
tests/test_gpu_live.py: a condition on the seeds, not a measurement)."""
import numpy as np
import pytest

import live_ref as LR
import live_weight_cases as WC
from bpl.base import _prng_key

SEED = WC.SEED


def _rows(S):
    return [name for s, name in WC.ROW_CASES if s == S]


def test_the_table_is_the_one_described():
    assert set(WC.DRAW_COUNTS) == set(WC.PASSES) == set(WC.SEGMENTS)
    assert {1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 4160, 4161, 12289, 65537,
            270001} == set(WC.DRAW_COUNTS)
    for S in WC.DRAW_COUNTS:
        rows = _rows(S)
        assert set(rows) <= set(WC.ROWS) and "first_only" in rows and "equal" in rows
        assert ("generic" in rows) == (S not in WC.EXACT_ONLY)
        assert set(WC.sim_counts(S)) == {1, 7, 64, 4099} | ({S - 1} if S > 1 else set())
    # the rows that were dropped are the ones that need more draws than S has
    assert _rows(1) == ["first_only", "equal", "generic"]
    assert set(WC.ROWS) - set(_rows(2)) == {"head_zero", "tail_zero", "one_segment"}
    for S in WC.DRAW_COUNTS:
        if S >= 63:
            assert set(_rows(S)) == set(WC.ROWS if S not in WC.EXACT_ONLY else WC.EXACT_ROWS), S


@pytest.mark.parametrize("S", list(WC.DRAW_COUNTS))
def test_per_segments_and_pass_counts(S):
    per, used = WC.SEGMENTS[S]
    assert per == WC.per_of(S) == -(-S // 256)
    seg = WC.segments_of(S)
    assert len(seg) == used and seg[0][0] == 0 and seg[-1][1] == S
    assert all(a[1] == b[0] for a, b in zip(seg, seg[1:])) and all(hi - lo == per for lo, hi in seg[:-1])
    assert WC.PASSES[S] == WC.passes_of(S)
    # the statements next to the sizes
    assert (WC.passes_of(64), WC.passes_of(65), WC.passes_of(4160), WC.passes_of(4161)) == (1, 2, 2, 3)
    assert WC.passes_of(270001) == 4 and WC.passes_of(64 * 4161 + 1) == 4 and WC.passes_of(64 * 4161) == 3
    assert len(WC.segments_of(255)) == 255 and len(WC.segments_of(257)) == 129


@pytest.mark.parametrize("S", list(WC.DRAW_COUNTS))
def test_the_emulation_counts_the_scan_values_below_the_target(S):
    most = 0
    for name in _rows(S):
        C = WC.weights(name, S)["C"]
        for N in WC.sim_counts(S):
            t = WC.targets(C, N, _prng_key(SEED + N))
            count, passes = WC.search_scan_emu(C, t)
            np.testing.assert_array_equal(count, np.searchsorted(C, t, side="left"), err_msg=f"{name} N={N}")
            assert passes.max() <= WC.PASSES[S] and passes.min() >= 1
            most = max(most, int(passes.max()))
        # targets the resampler cannot form: below every scan value, on one (the equality of `C[at] < target`),
        # between two, the total and beyond it
        edge = np.concatenate([[-1.0, 0.0, C[0], C[S // 2], np.nextafter(C[S // 2], np.inf), C[-1], 2.0 * C[-1] + 1.0]])
        count, _ = WC.search_scan_emu(C, edge)
        np.testing.assert_array_equal(count, np.searchsorted(C, edge, side="left"), err_msg=name)
        one, p1 = WC.search_scan_emu(C, float(edge[3]))
        assert one == count[3] and 1 <= p1 <= WC.PASSES[S]
    assert most == WC.PASSES[S]


@pytest.mark.parametrize("S", list(WC.DRAW_COUNTS))
def test_exact_rows_have_one_right_answer(S):
    per = WC.per_of(S)
    for name in _rows(S):
        if name not in WC.EXACT_ROWS:
            continue
        lw = WC.log_weights(name, S)
        w = WC.weights(name, S)
        live = lw == lw.max()
        K = WC.live_count(name, S)
        assert K == int(live.sum()) >= 1
        np.testing.assert_array_equal(w["omega"], live.astype(np.float64))          # weights in {0, 1}
        np.testing.assert_array_equal(w["C"], np.cumsum(live).astype(np.float64))   # an integer scan, any association
        assert w["W"] == float(K) and w["ess"] == float(K) and w["log_evidence"] == 0.0
        # the rows are what their names say
        if name == "first_only":
            assert K == 1 and live[0]
        elif name == "last_only":
            assert K == 1 and live[-1]
        elif name == "alternate":
            assert not live[0] and live[1] and K == S // 2
        elif name == "sparse":
            assert 1 <= K and abs(K - 0.3 * S) <= max(3.0, 4.0 * np.sqrt(0.21 * S))
        elif name == "head_zero":
            assert not live[:2 * per + 1].any() and live[2 * per + 1:].all()
        elif name == "tail_zero":
            assert not live[S - 2 * per - 1:].any() and live[:S - 2 * per - 1].all()
        elif name == "one_segment":
            seg = WC.segments_of(S)
            i = len(seg) // 2
            assert 1 <= i <= len(seg) - 2 and live[seg[i][0]:seg[i][1]].all() and K == seg[i][1] - seg[i][0]
        else:
            assert K == S
        for N in WC.sim_counts(S):
            s, _ = LR.resample(w["C"], N, _prng_key(SEED + N))
            assert live[s].all(), (name, N)                              # no dead draw, the tail's S - 1 included
            used = np.bincount(s, minlength=S)[live]
            assert used.min() >= N // K and used.max() <= -(-N // K), (name, N)
            assert (np.diff(s) >= 0).all()
            if name == "tail_zero":
                assert s.max() <= S - 2 * per - 2


@pytest.mark.parametrize("S", [S for S in WC.DRAW_COUNTS if S not in WC.EXACT_ONLY])
def test_inexact_rows_flag_at_most_one_percent(S):
    for name in _rows(S):
        if name not in WC.INEXACT_ROWS:
            continue
        w = WC.weights(name, S)
        assert (w["omega"] > 0.0).all() and np.isfinite(w["C"]).all() and w["log_evidence"] == 0.0
        if name == "wide" and S >= 63:
            # a few draws hold nearly all the weight; most of the others are absorbed by the running sum
            top = np.sort(w["omega"])[::-1]
            assert top[:8].sum() >= 0.99 * w["W"] and (np.diff(w["C"]) == 0.0).any()
        for N in WC.sim_counts(S):
            _, flagged = LR.resample(w["C"], N, _prng_key(SEED + N))
            print(f"S={S} {name} N={N}: flagged {int(flagged.sum())}")
            assert flagged.sum() <= 0.01 * N, (name, N, int(flagged.sum()))
