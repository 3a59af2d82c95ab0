"""Inputs and exact references for the tests of the cross-lane layer, shared by the host emulator's tests
(test_wave_reduce_host.py) and the GPU probes (test_gpu_wave_primitives.py).

Sum operands are integer valued with every partial sum below 2^53 (2^24 in float32): the true total does not
depend on the order of summation, the reference is Python int arithmetic and the claim is bit equality.  Maxima
are order independent anyway.  Every generator takes the CHAIN number of a multi-chain reduction and gives that
chain data of its own scale and lane placement, so two chains swapped or mixed cannot cancel out."""
import math

import numpy as np

LANES = np.arange(64)
SEAMS = (0, 15, 16, 31, 32, 47, 48, 63)   # first and last lane of each 16-lane row

# the eleven written-out reductions: float maxima, double chains, and where the comment promises the result
CONTRACTS = {
    "wave_reduce_sum4_f64_raw": (0, ["add"] * 4, "lane63"),
    "wave_reduce_bounds_raw": (3, ["max", "max", "max", "add"], "lane63"),
    "lanes8_reduce_bounds_raw": (3, ["max", "max", "max", "add"], "lane4"),
    "wave_reduce_max3_f32_raw": (3, [], "lane63"),
    "wave_reduce_sum1_f64_raw": (0, ["add"], "lane63"),
    "wave_reduce_sum2_f64_raw": (0, ["add"] * 2, "lane63"),
    "wave_reduce_max1_f64_raw": (0, ["max"], "lane63"),
    "wave_reduce_max1_f32_raw": (1, [], "lane63"),
    "wave_reduce_max_f64_f32_raw": (1, ["max"], "lane63"),
    "wave_reduce_max3_f64_raw": (0, ["max"] * 3, "lane63"),
    "row_reduce_sum6_f64_raw": (0, ["add"] * 6, "row"),
}


def sum_waves(chain, f32=False, lanes=64):
    """[n, 64] integer-valued operands of one sum chain (zeros from lane `lanes` on): a one-hot 1 in every lane in
    turn, the weighted pattern 2^(k mod 48) (float32: 2^(k mod 20)) that any dropped or repeated lane changes,
    and random integers of mixed sign below 2^40 (2^17), on a scale of the chain's own."""
    rs = np.random.RandomState(1000 + chain + 100 * f32)
    onehot = np.roll(np.eye(64), 5 * chain, axis=1) if lanes == 64 else np.eye(64)[:lanes]
    weighted = (chain % 3 + 1) * np.roll(2.0 ** (LANES % (20 if f32 else 48)), 3 * chain)
    top = (2 ** 17 >> chain) if f32 else (2 ** 40 >> 2 * chain)
    ints = rs.randint(-top + 1, top, size=(40, 64)).astype(np.float64)
    ints[:8] *= rs.uniform(size=(8, 64)) < 0.2     # mostly zeros: a lone small lane among nothing
    ints[8:16, :] = np.where(rs.uniform(size=(8, 64)) < 0.1, rs.randint(-3, 4, size=(8, 64)), ints[8:16])
    x = np.concatenate([onehot, weighted[None], ints])
    x[:, lanes:] = 0.0
    return x.astype(np.float32 if f32 else np.float64)


def normal_waves(chain, f32=False, lanes=64):
    """[16, 64] random normals on the chain's own scale: the one non-integer case of every sum."""
    x = np.random.RandomState(2000 + chain).normal(size=(16, 64)) * 10.0 ** chain
    x[:, lanes:] = 0.0
    return x.astype(np.float32 if f32 else np.float64)


def max_waves(chain, f32=False, lanes=64):
    """[n, 64] operands >= 0 of one maximum chain: the maximum in every lane in turn, +0.0 everywhere, denormals,
    the largest finite number, all lanes equal."""
    dt = np.float32 if f32 else np.float64
    rs = np.random.RandomState(3000 + chain + 100 * f32)
    scale = 2.0 ** (5 * chain + 1)
    moving = rs.uniform(0, 1, size=(lanes, 64)) * scale
    moving[np.arange(lanes), (np.arange(lanes) + 3 * chain) % lanes] = 1.5 * scale
    tiny = float(np.nextafter(dt(0), dt(1)))
    denormal = tiny * rs.randint(1, 1000, size=(2, 64)) * (chain + 1)
    huge = rs.uniform(0, 1, size=(2, 64)) * scale
    huge[0, (17 + chain) % lanes] = huge[1, (lanes - 1 - chain) % lanes] = np.finfo(dt).max
    x = np.concatenate([moving, np.zeros((1, 64)), denormal, huge, np.full((1, 64), 0.3 * scale)])
    x[:, lanes:] = 0.0
    return x.astype(dt)


def int_sum(x):
    """Exact totals over the last axis of integer-valued floats, as Python ints (object array)."""
    flat = x.reshape(-1, x.shape[-1])
    assert (flat == np.rint(flat)).all()
    return np.array([sum(int(v) for v in row) for row in flat], dtype=object).reshape(x.shape[:-1])


def fsum_last(x):
    """(correctly rounded totals, sum |x|) over the last axis."""
    flat = np.asarray(x, dtype=np.float64).reshape(-1, x.shape[-1])
    return (np.array([math.fsum(r) for r in flat]).reshape(x.shape[:-1]),
            np.array([math.fsum(np.abs(r)) for r in flat]).reshape(x.shape[:-1]))


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def assert_bits_equal(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want, dtype=np.asarray(got).dtype)
    bad = np.argwhere(bits(got) != bits(np.broadcast_to(want, got.shape).copy()))
    assert bad.size == 0, f"{what}: {len(bad)} mismatches, first at {bad[0].tolist()}: " \
                          f"got {got[tuple(bad[0])]!r}, want {np.broadcast_to(want, got.shape)[tuple(bad[0])]!r}"


def top2_reference(values, T):
    """wave_top2's documented result on values[:T] (> 0), as (m1, m2, i1, i2): lanes stride over the teams, a lane
    keeps its first-seen largest and the largest of the rest; the lowest lane holding the wave maximum wins, the
    runner-up is the largest of what is left (the winner lane's second, the other lanes' first), lowest lane again.
    No second team: i2 = -1, m2 = 0."""
    a1, a2, j1, j2 = [0.0] * 64, [0.0] * 64, [-1] * 64, [-1] * 64
    for t in range(T):
        l, v = t % 64, values[t]
        if v > a1[l]:
            a2[l], j2[l], a1[l], j1[l] = a1[l], j1[l], v, t
        elif v > a2[l]:
            a2[l], j2[l] = v, t
    m1 = max(a1)
    win = min(l for l in range(64) if a1[l] == m1 and j1[l] >= 0)
    c = [a2[l] if l == win else a1[l] for l in range(64)]
    jc = [j2[l] if l == win else j1[l] for l in range(64)]
    m2 = max(c)
    cand = [l for l in range(64) if c[l] == m2 and jc[l] >= 0]
    if not cand:
        return m1, type(m1)(0), j1[win], -1
    return m1, m2, j1[win], jc[cand[0]]
