"""GPU: the cross-lane layer on its own -- the written-out reductions of csrc/wave_reduce.hip.h through their
dc:: wrappers, the DPP helpers and scans of csrc/dc_kernels.hip.h, block_sum, nd_wave_sum* and wave_top2* --
through bplhip_selftest_lanes, which calls the library's own functions and returns what every lane holds.

References are exact (tests/wave_cases.py): integer-valued sums against Python ints, maxima against max, both
bit for bit; one case of random normals per sum against math.fsum within 6 * 2^-53 * sum|x| (six pairwise
levels; block_sum adds its serial combine of 8 waves: 13).  Every call also carries bystander values in all the
channels the probe does not use, live in registers across the call: they must come back bit-identical."""
import numpy as np
import pytest

import wave_cases as wc
from bpl import _ffi

pytestmark = pytest.mark.gpu
CH = _ffi.SELFTEST_CHANNELS

# bplhip_selftest_lanes' `which`, in the order of include/bplhip.h
(SUM4_F64, BOUNDS, LANES8, MAX3_F32, SUM1_F64, SUM2_F64, MAX1_F64, MAX1_F32, MAX_F64_F32, MAX3_F64, ROW_SUM6, SUM_F32,
 SUM2_F32, PREV_LANE, PREFIX, SUFFIX, SUMN_2, SUMN_7, SUMN_13, BLOCK_2, BLOCK_5_LDS, BLOCK_6_LDS, ND_SUM, ND_SUM2,
 TOP2_F32, TOP2_F64, TOP2_PAIR, Q30, EXACT_I64) = range(29)
assert _ffi.SELFTEST_COUNTED_ROWS == 29

# every instantiation in the library (a search for `wave_sumN_f64(`, `row_sum_f64(` and `block_sum<` in csrc/):
#   wave_sumN_f64<NV>: 2 (dc_dynamic, dc_neutral `both`), 7 (dc_neutral `sv`, `t`), 13 (dc_neutral `loc`)
#   row_sum_f64<NV>: 6 (dc_neutral `s6`);  block_sum<NV, LDS_ONLY>: <2, false>, <5, true>, <6, true> (dc_kernels)
WAVE_SUMS_F64 = {"wave_sum4_f64": (SUM4_F64, 4), "wave_sum_f64": (SUM1_F64, 1), "wave_sum2_f64": (SUM2_F64, 2),
                 "wave_sumN_f64<2>": (SUMN_2, 2), "wave_sumN_f64<7>": (SUMN_7, 7), "wave_sumN_f64<13>": (SUMN_13, 13),
                 "nd_wave_sum": (ND_SUM, 1), "nd_wave_sum2": (ND_SUM2, 2)}
BLOCK_SUMS = {"block_sum<2>": (BLOCK_2, 2), "block_sum<5, true>": (BLOCK_5_LDS, 5), "block_sum<6, true>": (BLOCK_6_LDS, 6)}
WAVE_SUMS_F32 = {"wave_sum_f32": (SUM_F32, 1), "wave_sum2_f32": (SUM2_F32, 2)}


def probe(ctx, which, d=(), f=(), i=(), res_d=None, res_f=None, res_i=None):
    """Run one probe with the given operand channels ([n, 64] each) and random bystanders everywhere else; check
    that everything outside the result channels came back bit-identical; return the three output arrays."""
    n = len((list(d) + list(f) + list(i))[0])
    rs = np.random.RandomState(which)
    D = rs.normal(size=(n, CH, 64)) * 1e3
    F = (rs.normal(size=(n, CH, 64)) * 1e3).astype(np.float32)
    I = rs.randint(-2 ** 31, 2 ** 31, size=(n, CH, 64)).astype(np.int32)
    for arr, ops in ((D, d), (F, f), (I, i)):
        for c, x in enumerate(ops):
            arr[:, c, :] = x
    oD, oF, oI = ctx.selftest_lanes(which, D, F, I)
    for name, got, sent, res, ops in (("f64", oD, D, res_d, d), ("f32", oF, F, res_f, f), ("i32", oI, I, res_i, i)):
        keep = sorted(set(range(CH)) - set(range(len(ops)) if res is None else res))
        wc.assert_bits_equal(got[:, keep], sent[:, keep], f"probe {which}: {name} bystander channels {keep}")
    return oD, oF, oI


def _uniform(x):
    return np.asarray(x)[:, None]


def _check_sum_chain(got, x, levels, eps, what, n_exact):
    """got [n, k] (every lane that must hold the total), x [n, m] the operands: the first n_exact cases are integer
    valued (bit equality), the rest normals (levels * eps * sum|x|)."""
    wc.assert_bits_equal(got[:n_exact], _uniform(wc.int_sum(x[:n_exact]).astype(np.float64)), what)
    want, mag = wc.fsum_last(x[n_exact:])
    err = np.abs(got[n_exact:].astype(np.float64) - _uniform(want))
    print(f"{what}: normals, max error / (eps * sum|x|) = {(err / _uniform(eps * mag)).max():.3f} (bound {levels})")
    assert (err <= levels * eps * _uniform(mag)).all(), what


def _sum_inputs(nv, f32=False, multiple=1):
    xs = [np.concatenate([wc.sum_waves(c, f32), wc.normal_waves(c, f32)]) for c in range(nv)]
    n_exact = len(xs[0]) - 16
    if multiple > 1:   # whole workgroups: exact cases and normals each padded (by repetition) to a multiple
        pad = lambda x: np.resize(x, (-(-len(x) // multiple) * multiple, 64))
        xs = [np.concatenate([pad(x[:n_exact]), pad(x[n_exact:])]) for x in xs]
        n_exact = -(-n_exact // multiple) * multiple
    return xs, n_exact


@pytest.mark.parametrize("name", sorted(WAVE_SUMS_F64))
def test_wave_sums_f64_are_exact_and_wave_uniform(hip_ctx, name):
    which, nv = WAVE_SUMS_F64[name]
    xs, n_exact = _sum_inputs(nv)
    oD, _, _ = probe(hip_ctx, which, d=xs)
    for c in range(nv):
        _check_sum_chain(oD[:, c, :], xs[c], 6, 2.0 ** -53, f"{name} chain {c}", n_exact)


@pytest.mark.parametrize("name", sorted(WAVE_SUMS_F32))
def test_wave_sums_f32_are_exact_and_wave_uniform(hip_ctx, name):
    which, nv = WAVE_SUMS_F32[name]
    xs, n_exact = _sum_inputs(nv, f32=True)
    _, oF, _ = probe(hip_ctx, which, f=xs)
    for c in range(nv):
        _check_sum_chain(oF[:, c, :], xs[c], 6, 2.0 ** -24, f"{name} chain {c}", n_exact)


@pytest.mark.parametrize("name", sorted(BLOCK_SUMS))
def test_block_sums_are_exact_in_every_thread(hip_ctx, name):
    which, nv = BLOCK_SUMS[name]
    xs, n_exact = _sum_inputs(nv, multiple=8)
    oD, _, _ = probe(hip_ctx, which, d=xs)
    for c in range(nv):
        _check_sum_chain(oD[:, c, :].reshape(-1, 512), xs[c].reshape(-1, 512), 13, 2.0 ** -53, f"{name} value {c}",
                         n_exact // 8)


def test_row_sums_give_every_lane_its_own_rows_total(hip_ctx):
    xs, n_exact = _sum_inputs(6)
    oD, _, _ = probe(hip_ctx, ROW_SUM6, d=xs)
    for c in range(6):
        rows = xs[c].reshape(-1, 4, 16)
        want = np.repeat(wc.int_sum(rows[:n_exact]).astype(np.float64), 16, axis=-1)
        assert len({tuple(w[::16]) for w in want}) > 30          # (the rows of a wave do have different totals)
        wc.assert_bits_equal(oD[:n_exact, c, :], want, f"row_sum_f64<6> chain {c}")
        ref, mag = wc.fsum_last(rows[n_exact:])
        assert (np.abs(oD[n_exact:, c, :] - np.repeat(ref, 16, axis=-1)) <= 6 * 2.0 ** -53 * np.repeat(mag, 16, axis=-1)).all()


def _max_inputs(nf, nd, lanes=64):
    f = [wc.max_waves(c, f32=True, lanes=lanes) for c in range(nf)]
    d = [wc.max_waves(nf + c, lanes=lanes) for c in range(nd)]
    return f, d


@pytest.mark.parametrize("name,which,nf,nd", [("wave_max3_f32", MAX3_F32, 3, 0), ("wave_max_f64", MAX1_F64, 0, 1),
                                              ("wave_max_f32", MAX1_F32, 1, 0), ("wave_max3_f64", MAX3_F64, 0, 3)])
def test_wave_maxima_are_bit_equal_to_max_and_wave_uniform(hip_ctx, name, which, nf, nd):
    f, d = _max_inputs(nf, nd)
    oD, oF, _ = probe(hip_ctx, which, d=d, f=f)
    for c in range(nf):
        wc.assert_bits_equal(oF[:, c, :], _uniform(f[c].max(axis=-1)), f"{name} float chain {c}")
    for c in range(nd):
        wc.assert_bits_equal(oD[:, c, :], _uniform(d[c].max(axis=-1)), f"{name} double chain {c}")


def test_max_f64_f32_raw_keeps_its_promise_in_lane_63(hip_ctx):
    f, d = _max_inputs(1, 1)
    oD, oF, _ = probe(hip_ctx, MAX_F64_F32, d=d, f=f)
    wc.assert_bits_equal(oF[:, 0, 63], f[0].max(axis=-1), "float")
    wc.assert_bits_equal(oD[:, 0, 63], d[0].max(axis=-1), "double")


@pytest.mark.parametrize("name,which,lanes", [("wave_bounds_reduce", BOUNDS, 64), ("lanes8_max3_sum", LANES8, 8)])
def test_seven_value_bounds_keep_their_chains_apart(hip_ctx, name, which, lanes):
    """three float maxima, three double maxima and a double sum in one call, every chain on its own scale; the
    eight-lane form takes its values in lanes 0..7 (zeros elsewhere), the extremum in each of the 8 lanes in turn."""
    f, d = _max_inputs(3, 3, lanes)
    s = np.concatenate([wc.sum_waves(3, lanes=lanes), wc.normal_waves(3, lanes=lanes)])
    n_exact = len(s) - 16
    f = [np.resize(x, (len(s), 64)) for x in f]
    d = [np.resize(x, (len(s), 64)) for x in d]
    oD, oF, _ = probe(hip_ctx, which, d=d + [s], f=f)
    for c in range(3):
        wc.assert_bits_equal(oF[:, c, :], _uniform(f[c].max(axis=-1)), f"{name} float maximum {c}")
        wc.assert_bits_equal(oD[:, c, :], _uniform(d[c].max(axis=-1)), f"{name} double maximum {c}")
    _check_sum_chain(oD[:, 3, :], s, 6, 2.0 ** -53, f"{name} sum", n_exact)


def _scan_inputs():
    rs = np.random.RandomState(7)
    seams = np.zeros((len(wc.SEAMS), 64))
    seams[np.arange(len(wc.SEAMS)), wc.SEAMS] = 1.0
    return np.concatenate([seams, np.ones((1, 64)), rs.randint(-2 ** 40 + 1, 2 ** 40, size=(64, 64)).astype(np.float64)])


def test_prefix_and_suffix_scans_match_cumsum_across_the_row_seams(hip_ctx):
    x = _scan_inputs()
    oD, _, _ = probe(hip_ctx, PREFIX, d=[x])
    wc.assert_bits_equal(oD[:, 0, :], np.cumsum(x, axis=-1), "wave_prefix_dpp_f64")
    oD, _, _ = probe(hip_ctx, SUFFIX, d=[x])
    wc.assert_bits_equal(oD[:, 0, :], np.cumsum(x[:, ::-1], axis=-1)[:, ::-1], "wave_suffix_dpp_f64")


def test_prev_lane_hands_every_lane_its_neighbour_and_lane_0_the_fill(hip_ctx):
    rs = np.random.RandomState(8)
    v = rs.randint(-2 ** 31, 2 ** 31, size=(32, 64)).astype(np.int32)
    fill = rs.randint(-2 ** 31, 2 ** 31, size=(32, 64)).astype(np.int32)
    _, _, oI = probe(hip_ctx, PREV_LANE, i=[v, fill], res_i=[0])
    want = np.concatenate([fill[:, :1], v[:, :-1]], axis=1)
    assert (oI[:, 0, :] == want).all()


# ---- wave_top2

TOP2_T = (1, 2, 3, 63, 64, 65, 255, 256, 257, 300)


def _top2_cases(dtype, seed):
    """(T, values[T]) per case: positive random values with the top (4) and the runner-up (3) placed; ties."""
    rs = np.random.RandomState(seed)
    cases = []
    for T in TOP2_T:
        base = lambda: rs.uniform(1.0, 2.0, size=T).astype(dtype)
        places = [(0, 1), (1, 0), (5, 6), (T - 1, T - 2), (0, 63), (63, 0), (3, 67), (67, 3), (70, 134), (255, 256),
                  (256, 255), (191, 256), (260, 4), (4, 260), (299, 43)]
        for top, second in [p for p in places if max(p) < T and min(p) >= 0]:
            v = base()
            v[top], v[second] = 4.0, 3.0
            cases.append((T, v))
            v = base()                 # two equal maxima: both reported
            v[top] = v[second] = 4.0
            cases.append((T, v))
        cases.append((T, base()))
        cases.append((T, np.full(T, 1.5, dtype=dtype)))       # all values equal
    return cases


def _flat(cases, width, dtype):
    out = np.zeros((len(cases), width), dtype=dtype)
    for k, (T, v) in enumerate(cases):
        out[k, :T] = v
    return out


def _check_top2(cases, m1, m2, i1, i2, what):
    """every lane of every case against the reference; equal maxima in different lanes must both be reported"""
    for k, (T, v) in enumerate(cases):
        w1, w2, j1, j2 = wc.top2_reference(list(v), T)
        dt = v.dtype.type
        wc.assert_bits_equal(m1[k], dt(w1), f"{what} case {k} (T={T}) m1")
        wc.assert_bits_equal(m2[k], dt(w2), f"{what} case {k} (T={T}) m2")
        assert (i1[k] == j1).all() and (i2[k] == j2).all(), (what, k, T, i1[k][0], i2[k][0], j1, j2)
        if T == 1:
            assert j2 == -1 and w2 == 0
        else:   # (the reference itself is held to the plain definition: the two largest, of different teams)
            order = np.sort(v)[::-1]
            assert (w1, w2) == (order[0], order[1]) and j1 != j2 and v[j1] == w1 and v[j2] == w2


@pytest.mark.parametrize("which,dtype", [(TOP2_F32, np.float32), (TOP2_F64, np.float64)])
def test_wave_top2_values_indices_and_ties(hip_ctx, which, dtype):
    cases = _top2_cases(dtype, 11)
    T = np.repeat(np.array([c[0] for c in cases], dtype=np.int32)[:, None], 64, axis=1)
    tab = _flat(cases, CH * 64, dtype).reshape(-1, CH, 64)
    ops = {"d" if dtype == np.float64 else "f": list(tab.transpose(1, 0, 2))}
    res = {"res_d" if dtype == np.float64 else "res_f": [0, 1]}
    oD, oF, oI = probe(hip_ctx, which, i=[T], res_i=[1, 2], **ops, **res)
    o = oD if dtype == np.float64 else oF
    _check_top2(cases, o[:, 0, :], o[:, 1, :], oI[:, 1, :], oI[:, 2, :], f"wave_top2<{dtype.__name__}>")


def test_wave_top2_pair_keeps_its_two_arrays_apart(hip_ctx):
    a = _top2_cases(np.float32, 12)
    b = []
    for T in TOP2_T:                                 # the second array: another case of the same T, on another scale
        same = [c for c in a if c[0] == T]
        b += [(T, v * np.float32(8.0)) for _, v in same[1:] + same[:1]]
    T = np.repeat(np.array([c[0] for c in a], dtype=np.int32)[:, None], 64, axis=1)
    tab = np.concatenate([_flat(a, CH * 32, np.float32), _flat(b, CH * 32, np.float32)], axis=1).reshape(-1, CH, 64)
    _, oF, oI = probe(hip_ctx, TOP2_PAIR, f=list(tab.transpose(1, 0, 2)), i=[T], res_f=[0, 1, 2, 3], res_i=[1, 2, 3, 4])
    _check_top2(a, oF[:, 0, :], oF[:, 1, :], oI[:, 1, :], oI[:, 2, :], "wave_top2_pair_f32 first array")
    _check_top2(b, oF[:, 2, :], oF[:, 3, :], oI[:, 3, :], oI[:, 4, :], "wave_top2_pair_f32 second array")
