"""GPU: the counted accumulator rows of dc_eval on their own (csrc/dc_kernels.hip.h: q30, exact_i64, ga_add,
ga_load*, ga_count, ga_value, ga_is_zero, ga_rearm) through bplhip_selftest_lanes' counted-row probe: one
workgroup per contribution adds one value per row, a second launch reads every row through every load form and
re-arms it, a third re-reads it.  Nothing waits on another workgroup: this is about arithmetic and packing.

The reference is Python integer arithmetic in units of 2^-30.  Every case keeps the hi word's total below 2^53,
so ga_value must be the correctly rounded double of the exact sum, bit for bit."""
import numpy as np
import pytest

import wave_cases as wc
from test_gpu_wave_primitives import EXACT_I64, Q30, probe

pytestmark = pytest.mark.gpu

# the layout of a row (dc_kernels.hip.h)
HI_UNIT = 2 ** 44                  # GA_HI_UNIT * GA_LO_SCALE: one unit of the hi word, in units of 2^-30
GA_BIAS = 2 ** 45
COUNT_SHIFT, FLAG_SHIFT = 56, 54
NEGINF, BAD = 1, 2
LIMIT = 2.0 ** 94                  # GA_LIMIT * GA_LO_SCALE


def split(v):
    """(h, r): h = v / 2^44 rounded to nearest, ties to even (rint); r = v - h * 2^44, |r| <= 2^43."""
    h, rem = divmod(v, HI_UNIT)
    if rem > HI_UNIT // 2 or (rem == HI_UNIT // 2 and h & 1):
        h += 1
    return h, v - h * HI_UNIT


def check_rows(hip_ctx, values):
    """values [contributions, rows] (finite entries integer valued; inf / nan / out-of-range raise a flag)."""
    values = np.asarray(values, dtype=np.float64)
    n, rows = values.shape
    words, flags = hip_ctx.selftest_counted_rows(values)
    lo, hi = words[:, 0], words[:, 1]
    for r in range(rows):
        col = values[:, r]
        ok = np.abs(col) < LIMIT                       # (false for nan as well)
        ints = [int(v) for v in col[ok]]
        exact = sum(ints)
        parts = [split(v) for v in ints]
        want_hi = sum(h for h, _ in parts)
        assert abs(want_hi) < 2 ** 53, "the case itself must keep the hi total exact in a double"
        want_flag = (BAD if ((~ok) & (col != -np.inf)).any() else 0) | (NEGINF if (col == -np.inf).any() else 0)
        field = int(lo[r]) & ((1 << FLAG_SHIFT) - 1)
        count = (int(lo[r]) >> COUNT_SHIFT) & 0xFF
        assert count == n and flags[r, 0] == n, (r, count, flags[r, 0])        # complete, flagged or not
        assert (int(lo[r]) >> FLAG_SHIFT) & 3 == want_flag, (r, hex(int(lo[r])))
        assert int(hi[r]) == want_hi and field - n * GA_BIAS == sum(x for _, x in parts), (r, int(hi[r]), field)
        assert int(hi[r]) * HI_UNIT + (field - n * GA_BIAS) == exact, r
        value = words[r:r + 1, 2].view(np.float64)[0]
        if want_flag & BAD:
            assert np.isnan(value), (r, value)
        elif want_flag:
            assert value == -np.inf, (r, value)
        else:
            wc.assert_bits_equal(np.array([value]), np.array([exact / 2 ** 30]), f"ga_value of row {r}")
        assert flags[r, 1] == 0                                               # a counted row is not "zero"
    # every load form returns the same words, each row in its own slot
    nxt = lambda k: np.roll(words[:, 0:2], -k, axis=0)
    assert (words[:, 3:7] == np.hstack([nxt(0), nxt(1)])).all(), "ga_load2"
    assert (words[:, 7:15] == np.hstack([nxt(0), nxt(1), nxt(2), nxt(3)])).all(), "ga_load4"
    assert (words[:, 15:23] == np.hstack([nxt(0), nxt(1), nxt(2), nxt(0)])).all(), "ga_load3"
    assert (words[:, 23:31] == np.hstack([nxt(0), nxt(1), nxt(0), nxt(0)])).all(), "ga_load2rows"
    # re-armed: all zero on the re-read
    assert (words[:, 31] == 0).all() and (flags[:, 2] == 1).all() and (flags[:, 3] == 0).all()
    return words


def test_single_contributions_around_the_hi_lo_split(hip_ctx):
    half = 2 ** 43
    vals = [0, 1, -1, half - 1, -(half - 1), half, -half, half + 1, -(half + 1)]
    for k in (1, 2, 3, 1000, 2 ** 49):                 # ties of rint: to even, both ways
        vals += [s * HI_UNIT * k + t * half for s in (1, -1) for t in (1, -1)]
    vals += [int(np.nextafter(LIMIT, 0)), -int(np.nextafter(LIMIT, 0)), 2 ** 93 + 2 ** 43, 3 * 2 ** 30, 2 ** 52 + 1]
    assert all(float(v) == v for v in vals)
    check_rows(hip_ctx, np.array([[float(v) for v in vals]]))


def _cases_255():
    rs = np.random.RandomState(5)
    n = 255
    cols = [np.full(n, 2.0 ** 43), np.full(n, -2.0 ** 43)]               # the lo field at its extremes
    mag = np.floor(2.0 ** rs.uniform(0, 92, size=n)) * rs.choice([-1.0, 1.0], size=n)
    mag[0], mag[1] = np.nextafter(LIMIT, 0), -(2.0 ** 93)                # up to just under the limit
    cols.append(mag)
    cols.append(np.floor(2.0 ** rs.uniform(0, 50, size=n)) * rs.choice([-1.0, 1.0], size=n))
    pairs = np.floor(2.0 ** rs.uniform(0, 90, size=n // 2))
    cols.append(rs.permutation(np.concatenate([pairs, -pairs, [0.0]])))  # pairs that cancel exactly
    ordinary = np.floor(rs.normal(size=n) * 2.0 ** 46)
    for bad in ([np.inf], [np.nan], [LIMIT], [-LIMIT], [-np.inf], [-np.inf, np.nan], [np.nan, -np.inf, np.inf]):
        c = ordinary.copy()
        c[rs.choice(n, size=len(bad), replace=False)] = bad
        cols.append(c)
    return np.stack(cols, axis=1)


def test_255_contributions_extremes_random_cancelling_and_flagged(hip_ctx):
    values = _cases_255()
    words = check_rows(hip_ctx, values)
    assert (words[:2, 0] >> FLAG_SHIFT & 3 == 0).all() and ((words[:2, 0] >> COUNT_SHIFT) & 0xFF == 255).all()
    assert words[4, 1] == 0 and (words[4, 0] & ((1 << FLAG_SHIFT) - 1)) == 255 * GA_BIAS   # cancelled: exactly zero
    assert np.isnan(words[:, 2].view(np.float64)[[5, 6, 7, 8, 10, 11]]).all()
    assert words[9:10, 2].view(np.float64)[0] == -np.inf


@pytest.mark.parametrize("n", [2, 7, 64])
def test_fewer_contributions(hip_ctx, n):
    rs = np.random.RandomState(n)
    check_rows(hip_ctx, np.floor(rs.normal(size=(n, 37)) * 2.0 ** rs.uniform(0, 60, size=(n, 37))))


def test_q30_is_rint_of_x_times_2_to_the_30(hip_ctx):
    rs = np.random.RandomState(9)
    e = np.repeat(np.arange(-45, 31), 64)[: 64 * 76]
    x = (rs.uniform(1, 2, size=e.size) * 2.0 ** e * rs.choice([-1, 1], size=e.size)).astype(np.float32)
    x[:8] = [0.0, -0.0, 2.0 ** -7, -(2.0 ** -7), 2.0 ** -31, 1.5 * 2.0 ** -30, 2.5 * 2.0 ** -30, np.float32(1e-4)]
    x = x.reshape(-1, 64)
    oD, _, _ = probe(hip_ctx, Q30, f=[x], res_d=[0], res_f=[])
    want = np.rint(x.astype(np.float64) * 2.0 ** 30)
    wc.assert_bits_equal(oD[:, 0, :], want, "q30")
    big = np.abs(x) >= 2.0 ** -7                        # from 2^-7 up a float32 already is a multiple of 2^-30
    assert big.sum() > 1000 and (oD[:, 0, :][big] == x.astype(np.float64)[big] * 2.0 ** 30).all()


def test_exact_i64_is_exact_up_to_2_to_the_51(hip_ctx):
    rs = np.random.RandomState(10)
    top = 2 ** 51 - 1
    v = np.concatenate([[0, 1, -1, top, -top, top - 1, 2 ** 50, -(2 ** 50), 2 ** 32, -(2 ** 32) - 1],
                        rs.randint(-top, top + 1, size=246),
                        (rs.randint(-top, top + 1, size=256) >> rs.randint(0, 51, size=256))]).astype(np.int64)
    x = v.astype(np.float64).reshape(-1, 64)
    assert (x.astype(np.int64).ravel() == v).all()
    oD, _, _ = probe(hip_ctx, EXACT_I64, d=[x])
    assert (oD[:, 0, :].view(np.int64) == v.reshape(-1, 64)).all()


def test_rows_do_not_depend_on_how_the_addends_are_partitioned(hip_ctx):
    """the same multiset of q30 values over 1, 7 and 255 contributors, shuffled.  The raw words cannot be compared
    as they are: lo carries the count and one bias per contribution, and each contribution is split into hi and lo
    on its own.  What must be identical is what they hold, hi * 2^44 + lo as an exact integer, and ga_value's bits."""
    rs = np.random.RandomState(11)
    rows = 24
    x = (rs.normal(size=(2000, rows)) * 10.0 ** rs.uniform(-4, 4, size=(1, rows))).astype(np.float32)
    q = np.rint(x.astype(np.float64) * 2.0 ** 30)                      # q30, as checked above
    seen = []
    for n in (1, 7, 255):
        owner = rs.randint(0, n, size=2000)
        owner[:n] = np.arange(n)
        part = np.array([[sum(int(v) for v in q[owner == k, r]) for r in range(rows)] for k in range(n)], dtype=object)
        assert (np.abs(part.astype(np.float64)) < 2.0 ** 53).all()
        words = check_rows(hip_ctx, part.astype(np.float64))
        seen.append([(int(w[0]) & ((1 << FLAG_SHIFT) - 1)) - n * GA_BIAS + int(w[1]) * HI_UNIT for w in words])
        total = [sum(int(v) for v in q[:, r]) for r in range(rows)]
        assert seen[-1] == total
        values = words[:, 2].view(np.float64).copy()
        seen[-1] = (seen[-1], values.tobytes())
    assert seen[0] == seen[1] == seen[2]
