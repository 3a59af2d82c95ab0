"""The case table of the weighted-draw tests (tests/test_live_weight_cases_host.py without a GPU,
tests/test_gpu_live_weights.py on one): draw counts S, log-weight rows per S and simulation counts N for
csrc/dc_live.hip.h's live_weights (one workgroup, thread i owns the i-th contiguous segment of per = ceil(S / 256)
draws) and search_scan (a wave-uniform 64-ary search of the scan C), and a lane-by-lane emulation of that search.

EXACT rows hold only 0.0 and -1e4 (or one constant): exp(0.0) is exactly 1 and exp(-1e4) exactly 0 on the device
and in numpy, so the weights are 0 or 1, every scan value is an integer below 2^53 whatever the association, and
W = K, the number of live draws.  The targets min((j + U) W / N, W) are the same IEEE multiply, divide and min on
both sides: the draw of every simulation has one right answer, bit for bit, and the tests that use these rows take
no tolerance and excuse no simulation.  INEXACT rows carry generic weights: there `exp` may differ in its last bit
and live_ref.resample's flags apply, at most 1 % of a case's simulations."""
import functools

import numpy as np

import live_ref as LR

THREADS = LR.THREADS
DEAD = -1e4            # exp(DEAD - 0.0) == 0.0 exactly
SEED = 20261           # a call with N simulations runs under random_state SEED + N

# S -> why it is here
DRAW_COUNTS = {
    1: "a single draw: every target lands on it, per = 1, one segment",
    2: "two draws, the smallest scan with a step in it",
    63: "one search pass; the `at < hi` mask leaves lane 63 out",
    64: "one search pass with every lane in range",
    65: "the first size with two passes: step 2, lanes 0..32 in range, then a window of one",
    255: "per = 1 and the last thread's segment is empty",
    256: "per = 1 with every segment full: S an exact multiple of the workgroup",
    257: "per goes from 1 to 2: only 129 segments are used, the last holds one draw",
    511: "per = 2, the last segment partial",
    512: "per = 2 with every segment full",
    513: "per goes from 2 to 3: 171 segments",
    4095: "two passes, step 64 then a full window of 63",
    4096: "two passes, S = 64 * 64",
    4097: "two passes, step 65",
    4160: "the last size with two passes: the second has all 64 lanes in range",
    4161: "the first size with three passes",
    12289: "three passes, per = 49: one past predict_in_play's largest posterior",
    65537: "three passes, per = 257: segments longer than the workgroup is wide",
    270001: "four passes, per = 1055 (beyond any real posterior, a few megabytes): the 0/1 rows only",
}
# the most passes search_scan takes at each S (a window that runs into `hi` may end one pass sooner)
PASSES = {1: 1, 2: 1, 63: 1, 64: 1, 65: 2, 255: 2, 256: 2, 257: 2, 511: 2, 512: 2, 513: 2, 4095: 2, 4096: 2,
          4097: 2, 4160: 2, 4161: 3, 12289: 3, 65537: 3, 270001: 4}
# (per, the number of non-empty segments) of live_weights at each S
SEGMENTS = {1: (1, 1), 2: (1, 2), 63: (1, 63), 64: (1, 64), 65: (1, 65), 255: (1, 255), 256: (1, 256),
            257: (2, 129), 511: (2, 256), 512: (2, 256), 513: (3, 171), 4095: (16, 256), 4096: (16, 256),
            4097: (17, 241), 4160: (17, 245), 4161: (17, 245), 12289: (49, 251), 65537: (257, 256),
            270001: (1055, 256)}
EXACT_ONLY = (270001,)

EXACT_ROWS = ("first_only", "last_only", "alternate", "sparse", "head_zero", "tail_zero", "one_segment", "equal")
INEXACT_ROWS = ("generic", "wide")
ROWS = EXACT_ROWS + INEXACT_ROWS


def per_of(S):
    return (S + THREADS - 1) // THREADS


def segments_of(S):
    """The non-empty (lo, hi) segments of live_weights, thread order."""
    return [(lo, hi) for lo, hi in LR._segments(S) if hi > lo]


def passes_of(S):
    """The most passes of search_scan over S draws: a pass over a window of w leaves at most ceil(w / 64) - 1."""
    n, w = 0, S
    while w > 0:
        w = (w + 63) // 64 - 1
        n += 1
    return n


def _live_mask(name, S):
    """bool [S] the live draws of an exact row, or None when S has too few draws for it."""
    per, seg = per_of(S), segments_of(S)
    live = np.zeros(S, dtype=bool)
    if name == "first_only":
        live[0] = True
    elif name == "last_only":
        if S < 2:
            return None
        live[-1] = True
    elif name == "alternate":              # 0, 1, 0, 1, ...
        if S < 2:
            return None
        live[1::2] = True
    elif name == "sparse":                 # about 30 % live, at least one
        if S < 2:
            return None
        rs = np.random.RandomState(S)
        live = rs.uniform(size=S) < 0.3
        if not live.any():
            live[rs.randint(S)] = True
    elif name in ("head_zero", "tail_zero"):   # two whole segments and one draw more are dead
        dead = 2 * per + 1
        if S < dead + 1:
            return None
        live[:] = True
        if name == "head_zero":
            live[:dead] = False
        else:
            live[S - dead:] = False
    elif name == "one_segment":            # one interior thread's segment, whole empty segments on both sides
        if len(seg) < 3:
            return None
        lo, hi = seg[len(seg) // 2]
        live[lo:hi] = True
    else:
        raise KeyError(name)
    return live


@functools.lru_cache(maxsize=None)
def log_weights(name, S):
    """float64 [S] the row `name` at S draws (read-only), or None when the row needs more draws than S has."""
    if name == "equal":
        lw = np.full(S, 3.5)
    elif name == "generic":                # live_cases.random_log_weights' law
        lw = np.random.RandomState(S).normal(0.0, 1.5, S)
    elif name == "wide":                   # a few draws hold all the weight, the rest is tiny but not zero
        if S < 2 or S in EXACT_ONLY:
            return None
        lw = np.random.RandomState(S + 1).normal(0.0, 30.0, S)
    else:
        live = _live_mask(name, S)
        if live is None:
            return None
        lw = np.where(live, 0.0, DEAD)
    if name in INEXACT_ROWS and S in EXACT_ONLY:
        return None
    lw.setflags(write=False)
    return lw


def live_count(name, S):
    """K: the number of draws of weight 1 of an exact row."""
    lw = log_weights(name, S)
    return int((lw == lw.max()).sum())


def sim_counts(S):
    """N: fewer simulations than draws, more than draws, no divisor relation."""
    return tuple(sorted({1, 7, 64, 4099} | ({S - 1} if S > 1 else set())))


# every (S, row) of the table, and every (S, row, N)
ROW_CASES = [(S, name) for S in DRAW_COUNTS for name in ROWS if log_weights(name, S) is not None]
CASES = [(S, name, N) for S, name in ROW_CASES for N in sim_counts(S)]


@functools.lru_cache(maxsize=None)
def weights(name, S):
    """live_ref.weights of the row with no state part (L0 = 0), computed once and shared."""
    return LR.weights(log_weights(name, S), np.zeros(S))


def targets(C, N, key):
    """float64 [N]: the resampling targets of a call, as live_ref.resample and dc_season_live form them."""
    o0, _ = LR.SR.threefry_block(key, np.zeros(1, np.uint32), np.full(1, LR.RESAMPLE_COUNTER, np.uint32))
    U = LR.SR.unit_open(o0)[0]
    W = C[-1]
    return np.minimum((np.arange(N, dtype=np.float64) + U) * (W / float(N)), W)


def search_scan_emu(C, target):
    """(count, passes): search_scan of csrc/dc_live.hip.h restated lane by lane -- the window [lo, hi], `step`, the
    lanes' probe positions `at`, the ballot's population count and the two updates -- for one target or an array of
    them (each target is one wave; the 64 lanes are the last axis).  It also asserts what the kernel's comment
    claims: the probes below the target are a prefix of the lanes."""
    C = np.asarray(C, dtype=np.float64)
    t = np.atleast_1d(np.asarray(target, dtype=np.float64))
    S = C.size
    lane = np.arange(64, dtype=np.int64)[None, :]
    lo = np.zeros(t.size, dtype=np.int64)
    hi = np.full(t.size, S, dtype=np.int64)
    passes = np.zeros(t.size, dtype=np.int64)
    while True:
        run = np.nonzero(lo < hi)[0]
        if run.size == 0:
            break
        l, h = lo[run], hi[run]
        step = (h - l + 63) >> 6
        at = l[:, None] + (lane + 1) * step[:, None] - 1
        in_range = at < h[:, None]
        below = in_range & (C[np.where(in_range, at, 0)] < t[run, None])
        cnt = below.sum(axis=1)
        assert (below == (lane < cnt[:, None])).all()
        l = l + cnt * step
        lo[run] = l
        hi[run] = np.minimum(l + step - 1, h)
        passes[run] += 1
    if np.ndim(target) == 0:
        return int(lo[0]), int(passes[0])
    return lo, passes
