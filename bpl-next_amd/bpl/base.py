"""Predict side of the match predictors: everything the reference's BaseMatchPredictor offers
(bpl/base.py:25-348 -- same method names, arguments, return shapes, error behaviour), built on
ONE device primitive instead of re-tiling scoreline queries: the per-fixture scoreline grid
`bplhip_predict_score_grid` (csrc/dc_predict.hip.h, one wave per fixture on the matrix cores).
Outcome probabilities, n-goal marginals and the sampling methods are reductions of that grid;
`predict_score_proba` for arbitrary scorelines uses the pointwise kernel.  Arrays are numpy
(the reference returns jax arrays).  There is no host fallback: the predict path needs the HIP
library and a GPU, like `fit`.
"""

from __future__ import annotations

from datetime import datetime
from typing import Dict, Iterable, Optional, Tuple, Union

import numpy as np

from bpl import diagnostics as _diagnostics
from bpl import elpd as _elpd
from bpl import inplay as _inplay
from bpl import markets as _markets
from bpl import periods as _periods
from bpl import ratings as _ratings
from bpl import ppc as _ppc
from bpl import loo_scores as _loo_scores
from bpl import scenarios as _scenarios
from bpl import scoring as _scoring
from bpl import sensitivity as _sensitivity
from bpl import sequential as _sequential
from bpl import slate as _slate
from bpl._ffi import prng_key
from bpl._util import MAX_MATCH_POINTS, check_points, check_simulations, map_choice

MAX_GOALS = 15
# simulate_season's bounds (include/bplhip.h BPLHIP_SEASON_*): they keep every table field of the
# device ranking keys in 32 bits
SEASON_MAX_TEAMS = 64
SEASON_MAX_FIXTURES = 1 << 20
SEASON_MAX_TABLE_VALUE = 1 << 24
SEASON_MAX_MATCH_POINTS = MAX_MATCH_POINTS
LIVE_MAX_GOALS = 63   # a current score of simulate_season's in_play (include/bplhip.h BPLHIP_LIVE_MAX_GOALS)
# match_leverage's bounds (include/bplhip.h BPLHIP_LEVERAGE_*) and default targets
LEVERAGE_MAX_FIXTURES = 4096
LEVERAGE_MAX_TARGETS = 8
LEVERAGE_TARGETS = {"title": (0,), "top_four": (0, 1, 2, 3), "relegation": (-3, -2, -1)}
# points_needed's bound on the points axis (include/bplhip.h BPLHIP_POINTS_MAX_BINS)
POINTS_MAX_BINS = 1024
# season_trajectory's bound on the matchdays (include/bplhip.h BPLHIP_TRAJECTORY_MAX_ROUNDS)
TRAJECTORY_MAX_ROUNDS = 256
GRID_MAX_GOALS = 63  # depth of the device grid kernel (csrc/dc_predict.hip.h); deeper grids go pointwise
DTYPES = {
    "goals": "uint8",
    "teams": "uint16",
    "conferences": "uint8",
    "venue": "uint8",
    "outcome": "uint8",
}

TeamArg = Union[str, int, Iterable[str], Iterable[int]]
_prng_key = prng_key  # the name this module exported before the key moved to bpl._ffi; callers still import it


def _wall_clock_seed() -> int:
    # the reference seeds from the clock when random_state is None (bpl/base.py:173-174)
    return int(datetime.now().timestamp() * 100)


def _fingerprint(arrays) -> tuple:
    """Identity of a set of posterior arrays BY CONTENT: shape, dtype and a 128-bit hash of the whole
    buffer -- any in-place edit (`model.attack[:, j] = ...`, a swap of two columns) changes it, and
    neither a recycled `id` nor a temporary made by `np.asarray` enters it.  blake2b runs at ~1 GB/s: 0.6 ms
    for the four [1000, 20] tables of a league fit (the dynamic class hashes one gameweek's slices).
    Plain Python values (the dynamic class's gameweek) are part of the stamp as they are."""
    import hashlib

    out = []
    for a in arrays:
        if a is None or isinstance(a, (int, float, str, bool)):
            out.append(a)
            continue
        a = np.ascontiguousarray(a)
        out.append((a.shape, a.dtype.str, hashlib.blake2b(memoryview(a).cast("B"), digest_size=16).digest()))
    return tuple(out)


class PosteriorOnDevice:
    """The posterior draws of a fitted model, resident on one GPU for the predict kernels.  A mixin:
    the class says which arrays make up its posterior (`_posterior_arrays`) and how a context takes
    them (`_upload_posterior`).  The device context is created on first use, re-fed whenever the
    arrays change (assignment, `add_new_team`, in-place edits: `_fingerprint`), and is NOT part of the
    model's state: a fitted model pickles and deep-copies like the reference's (plain arrays), the
    copy re-creating its context on its first predict call."""

    #: GPU index for the predict path; None = this rank's GPU (bpl._dist) / GPU 0 on one process
    predict_device: Optional[int] = None
    _predict_ctx = None   # bpl._ffi.HipContext holding the uploaded posterior
    _uploaded = None      # fingerprint of the arrays last uploaded

    def _posterior_arrays(self) -> tuple:
        raise NotImplementedError

    def _upload_posterior(self, ctx) -> None:
        raise NotImplementedError

    def invalidate_predict_cache(self) -> None:
        """Force the next predict call to upload the posterior again."""
        self._uploaded = None

    def _device(self):
        """The context with this model's current posterior draws on the GPU."""
        if self._predict_ctx is None:
            from bpl import _dist
            from bpl._ffi import HipContext

            index = self.predict_device
            if index is None:
                index = _dist.local_device_index() if _dist.world()[1] > 1 else 0
            self._predict_ctx = HipContext(int(index))
            self._uploaded = None
        stamp = _fingerprint(self._posterior_arrays())
        if stamp != self._uploaded:
            self._upload_posterior(self._predict_ctx)
            self._uploaded = stamp
        return self._predict_ctx

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop("_predict_ctx", None)
        state.pop("_uploaded", None)
        return state

    def __deepcopy__(self, memo):
        import copy

        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for key, value in self.__getstate__().items():
            setattr(new, key, copy.deepcopy(value, memo))
        return new


def grid_from_pointwise(score_proba, n_fixtures: int, max_goals: int) -> np.ndarray:
    """A scoreline grid deeper than the grid kernel goes (max_goals > GRID_MAX_GOALS) through the
    pointwise kernel: `score_proba(fixture_index, x, y)` over every cell."""
    width = max_goals + 1
    x, y = np.divmod(np.arange(width * width), width)
    which = np.repeat(np.arange(n_fixtures), width * width)
    return score_proba(which, np.tile(x, n_fixtures), np.tile(y, n_fixtures)).reshape(n_fixtures, width, width)


# ---- the reductions of the scoreline grid, shared by every model class (plain functions on arrays)
def score_grid(device, home, away, max_goals, neutral=None, conf=None) -> np.ndarray:
    """[fixtures, max_goals+1, max_goals+1]: P(home scores x, away scores y).  `device()` returns the
    context holding the posterior (called after the argument check); `neutral` (0/1, scalar or per
    fixture) and `conf` = (home, away confederation indices) are given by the venue-aware classes."""
    max_goals = int(max_goals)
    if max_goals < 0:
        raise ValueError("max_goals must be >= 0")
    m = len(home)
    if neutral is not None:
        neutral = np.broadcast_to(np.asarray(neutral), (m,))
    dev = device()
    if max_goals <= GRID_MAX_GOALS:
        return dev.predict_score_grid(home, away, max_goals, neutral=neutral, conf=conf)
    at = lambda v, f: None if v is None else v[f]
    pick = lambda f: None if conf is None else (np.asarray(conf[0])[f], np.asarray(conf[1])[f])
    return grid_from_pointwise(
        lambda f, x, y: dev.predict_score_proba(home[f], away[f], x, y, neutral=at(neutral, f), conf=pick(f)),
        m, max_goals)


def outcome_from_grid(grid, knockout: bool = False) -> Dict[str, np.ndarray]:
    """Home win / draw / away win: the strictly lower triangle (home goals, axis 1, > away goals,
    axis 2), the diagonal and the strictly upper triangle of each fixture's grid.  `knockout`: no
    draws, the two wins renormalised."""
    home_win = np.tril(grid, -1).sum(axis=(1, 2))
    away_win = np.triu(grid, 1).sum(axis=(1, 2))
    if knockout:
        decided = home_win + away_win
        return {"home_win": home_win / decided, "away_win": away_win / decided}
    return {"home_win": home_win, "draw": np.trace(grid, axis1=1, axis2=2), "away_win": away_win}


def goals_wanted(n) -> np.ndarray:
    """The goal counts asked of an n-goal marginal, as an int64 vector; ValueError for a negative one."""
    wanted = np.atleast_1d(np.asarray(n, dtype=np.int64))
    if wanted.size and wanted.min() < 0:
        raise ValueError("n must be >= 0")
    return wanted


def goal_marginal(grid, wanted, max_goals, own_axis: int) -> np.ndarray:
    """P(`wanted` goals on `own_axis` (0: the home side's, 1: the away side's)) with the other side's
    goals summed over 0..max_goals: a row or column sum of ONE fixture's grid, which has to be
    max(max_goals, wanted.max()) deep."""
    other = np.take(grid, np.arange(max_goals + 1), axis=1 - own_axis)
    return other.sum(axis=1 - own_axis)[wanted]


def draw_scores(grid, max_goals, num_samples, random_state) -> Dict[str, np.ndarray]:
    """Scorelines drawn from each fixture's grid, [fixtures, num_samples] per side: one categorical
    draw over the flattened grid, then cell -> (row, column)."""
    seed = _wall_clock_seed() if random_state is None else random_state
    width = max_goals + 1
    cell = map_choice(prng_key(seed), np.arange(width * width, dtype="uint32"), num_samples,
                      grid.reshape(len(grid), width * width))
    rows, cols = np.divmod(cell, width)
    return {"home_score": rows.astype(DTYPES["goals"]), "away_score": cols.astype(DTYPES["goals"])}


def draw_winners(p, home, away, teams, num_samples, random_state) -> np.ndarray:
    """Winner's name, or 'Draw', [fixtures, num_samples], from outcome probabilities `p` (with or
    without "draw"): pick 0 is the home side, the last pick the away side."""
    seed = _wall_clock_seed() if random_state is None else random_state
    order = ("home_win", "draw", "away_win") if "draw" in p else ("home_win", "away_win")
    table = np.column_stack([p[k] for k in order])
    pick = map_choice(prng_key(seed), np.arange(len(order), dtype="uint32"), num_samples, table)
    labels = np.append(teams, "Draw")
    home_col, away_col = np.asarray(home)[:, None], np.asarray(away)[:, None]
    who = np.where(pick == 0, home_col, np.where(pick == len(order) - 1, away_col, len(teams)))
    return labels[who]


def leverage_targets(targets, n: int) -> Tuple[list, list]:
    """match_leverage's `targets` on a table of n rows: (names, masks), mask bit p = finishing position p.
    Negative positions count from the bottom, duplicates merge, positions outside the table are dropped."""
    targets = LEVERAGE_TARGETS if targets is None else targets
    if not 1 <= len(targets) <= LEVERAGE_MAX_TARGETS:
        raise ValueError(f"match_leverage takes 1..{LEVERAGE_MAX_TARGETS} targets, not {len(targets)}")
    names, masks = [], []
    for name, positions in targets.items():
        mask = 0
        for p in positions:
            if isinstance(p, (bool, np.bool_)) or int(p) != p:
                raise ValueError(f"targets[{name!r}]: positions are integers")
            p = int(p) + n if p < 0 else int(p)
            if 0 <= p < n:
                mask |= 1 << p
        if mask == 0:
            raise ValueError(f"targets[{name!r}] has no position inside a table of {n}")
        names.append(name)
        masks.append(mask)
    return names, masks


def leverage_from_counts(outcome_count, target_count, joint_count, n_sims: int) -> Dict[str, np.ndarray]:
    """match_leverage's derived floats from its three integer tables ([F, 3], [n, K], [F, 3, n, K])."""
    outcome_count = np.asarray(outcome_count).astype(np.int64)
    target_count = np.asarray(target_count).astype(np.int64)
    joint_count = np.asarray(joint_count).astype(np.int64)
    outcome_proba = outcome_count / n_sims
    target_proba = target_count / n_sims
    seen = outcome_count[:, :, None, None] > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        conditional = np.where(seen, joint_count / outcome_count[:, :, None, None], np.nan)
        se = np.sqrt(conditional * (1.0 - conditional) / outcome_count[:, :, None, None])
    moved = np.where(seen, np.abs(conditional - target_proba[None, None]), 0.0)
    return {
        "outcome_count": outcome_count, "outcome_proba": outcome_proba,
        "target_count": target_count, "target_proba": target_proba,
        "joint_count": joint_count, "conditional_proba": conditional, "conditional_se": se,
        "leverage": (outcome_proba[:, :, None, None] * moved).sum(axis=1),
    }


def points_axis(init_points, home_slot, away_slot, points) -> Tuple[int, int]:
    """points_needed's points axis, (points_min, P): slot t with m_t remaining matches ends on
    init_t + m_t min(points) .. init_t + m_t max(points); points_min is the least of the lower ends and
    P = the largest upper end - points_min + 1."""
    init = np.asarray(init_points, dtype=np.int64)
    m = (np.bincount(np.asarray(home_slot, dtype=np.int64), minlength=init.size)
         + np.bincount(np.asarray(away_slot, dtype=np.int64), minlength=init.size))
    lo, hi = init + m * int(min(points)), init + m * int(max(points))
    return int(lo.min()), int(hi.max()) - int(lo.min()) + 1


def check_levels(levels) -> np.ndarray:
    """points_needed's `levels`: non-empty, every value in (0, 1]."""
    try:
        lv = np.array([float(v) for v in levels], dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("levels must be a non-empty sequence of numbers in (0, 1]") from None
    if lv.size == 0 or not np.all((lv > 0.0) & (lv <= 1.0)):
        raise ValueError("levels must be a non-empty sequence of numbers in (0, 1]")
    return lv


def _first_bin(reached, points) -> np.ndarray:
    """The points value of the first True along the last axis of `reached` [..., P]; NaN where there is none."""
    return np.where(reached.any(axis=-1), points[reached.argmax(axis=-1)].astype(np.float64), np.nan)


def points_from_counts(team_points_count, team_target_count, position_points_count, gap_count, points_min: int,
                       n_sims: int, levels) -> Dict[str, np.ndarray]:
    """points_needed's derived floats from its four integer tables ([n, P], [n, P, K], [n, P], [n - 1, P]) and
    `levels` [L]: one float64 operation per cell on integer sums."""
    tp = np.asarray(team_points_count).astype(np.int64)
    tt = np.asarray(team_target_count).astype(np.int64)
    pp = np.asarray(position_points_count).astype(np.int64)
    gap = np.asarray(gap_count).astype(np.int64)
    levels = np.asarray(levels, dtype=np.float64)
    points = int(points_min) + np.arange(tp.shape[1], dtype=np.int64)
    target_count = tt.sum(axis=1)
    # "at least p": the integer reverse cumulative sums over the bins
    M = tp[:, ::-1].cumsum(axis=1)[:, ::-1]
    R = tt[:, ::-1].cumsum(axis=1)[:, ::-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        given = np.where(tp[:, :, None] > 0, tt / tp[:, :, None], np.nan)
        se = np.sqrt(given * (1.0 - given) / tp[:, :, None])
        at_least = np.where(M[:, :, None] > 0, R / M[:, :, None], np.nan)
    # [n, K, L, P]: the bin's "at least" odds reach the level (NaN compares False)
    with np.errstate(invalid="ignore"):
        reached = at_least.transpose(0, 2, 1)[:, :, None, :] >= levels[None, None, :, None]
    cdf = pp.cumsum(axis=1) / n_sims                                           # [n, P]
    quantile = points[(cdf[None] >= levels[:, None, None]).argmax(axis=-1)]    # [L, n]: cdf ends on 1.0 >= level
    return {
        "points": points, "levels": levels,
        "team_points_count": tp, "team_points_proba": tp / n_sims,
        "team_target_count": tt, "target_count": target_count, "target_proba": target_count / n_sims,
        "proba_given_points": given, "se_given_points": se, "proba_given_at_least": at_least,
        "points_needed": _first_bin(reached, points),
        "position_points_count": pp, "position_points_mean": (pp * points).sum(axis=1) / n_sims,
        "position_points_quantile": quantile,
        "gap_count": gap, "level_proba": gap[:, 0] / n_sims,
    }


def trajectory_rounds(matchday, nf: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """season_trajectory's `matchday` over nf fixtures: (matchdays int64 [R], the distinct labels ascending; fix_id
    int32 [nf], the fixtures' indices sorted by label, fixtures of one label in the order given; round_end int32 [R],
    one past each matchday's last entry of fix_id).  ValueError unless `matchday` holds one integer per fixture
    (floats and bools do not pass, integer-valued or not), for no fixtures, and for more than TRAJECTORY_MAX_ROUNDS
    distinct labels."""
    seq = matchday if isinstance(matchday, np.ndarray) else list(matchday)
    if not isinstance(matchday, np.ndarray) and any(isinstance(v, (bool, np.bool_)) for v in seq):
        raise ValueError("matchday must be integers")
    m = np.asarray(seq)
    if nf < 1:
        raise ValueError("season_trajectory needs at least one fixture")
    if m.shape != (nf,):
        raise ValueError("matchday must have one label per fixture")
    if m.dtype.kind not in "iu":
        raise ValueError("matchday must be integers")
    if m.dtype.kind == "u" and m.size and int(m.max()) > np.iinfo(np.int64).max:
        raise ValueError("matchday labels must fit 64 bits signed")
    values, index = np.unique(m.astype(np.int64), return_inverse=True)
    if values.size > TRAJECTORY_MAX_ROUNDS:
        raise ValueError(f"{values.size} matchdays: season_trajectory takes at most {TRAJECTORY_MAX_ROUNDS}")
    index = index.reshape(nf)
    fix_id = np.argsort(index, kind="stable").astype(np.int32)
    round_end = np.cumsum(np.bincount(index, minlength=values.size)).astype(np.int32)
    return values, fix_id, round_end


def trajectory_axis(init_points, home_slot, away_slot, points) -> Tuple[int, int]:
    """season_trajectory's points axis, (points_min, P): `points_axis` widened downwards to the least current
    total -- a table on the way passes through every total between a slot's current one and its last."""
    points_min, n_bins = points_axis(init_points, home_slot, away_slot, points)
    low = min(points_min, int(np.asarray(init_points, dtype=np.int64).min()))
    return low, n_bins + points_min - low


def trajectory_from_counts(position_count, target_count, target_final_count, points_sum, points_sq_sum,
                           rounds_inside_count, secured_count, lead_changes_count, points_min: int,
                           n_sims: int) -> Dict[str, np.ndarray]:
    """season_trajectory's result from the device's eight integer tables ([R, n, n], [R, n, K], [R, n, K], [R, n],
    [R, n], [n, K, R + 1], [n, K, R + 1], [R]); the two sums arrive as sums of v = points - points_min and of v^2 and
    are shifted back in exact integer arithmetic.  Every float is formed here from those integers."""
    pc, tc, tf, ric, sc, lc = (np.asarray(v).astype(np.int64) for v in (
        position_count, target_count, target_final_count, rounds_inside_count, secured_count, lead_changes_count))
    R = pc.shape[0]
    N, lo = int(n_sims), int(points_min)
    # Python integers: N sum(p^2) - (sum p)^2 can pass 64 bits
    v1 = np.asarray(points_sum).astype(np.int64).astype(object)
    v2 = np.asarray(points_sq_sum).astype(np.int64).astype(object)
    p1 = v1 + N * lo
    p2 = v2 + 2 * lo * v1 + N * lo * lo
    spread = (N * p2 - p1 * p1).astype(np.float64)          # N^2 times the variance
    if p2.size and int(p2.max()) > np.iinfo(np.int64).max:
        raise ValueError("points_sq_sum passes 64 bits: fewer simulations, or a current table on fewer points")
    outside = N - tc
    with np.errstate(divide="ignore", invalid="ignore"):
        given_in = np.where(tc > 0, tf / tc, np.nan)
        se_in = np.sqrt(given_in * (1.0 - given_in) / tc)
        given_out = np.where(outside > 0, (tc[R - 1][None] - tf) / outside, np.nan)
        se_out = np.sqrt(given_out * (1.0 - given_out) / outside)
    return {
        "position_count": pc, "position_proba": pc / N,
        "target_count": tc, "target_proba": tc / N, "target_final_count": tf,
        "final_given_inside": given_in, "final_given_inside_se": se_in,
        "final_given_outside": given_out, "final_given_outside_se": se_out,
        "points_sum": p1.astype(np.int64), "points_sq_sum": p2.astype(np.int64),
        "points_mean": p1.astype(np.float64) / N, "points_sd": np.sqrt(spread) / N,
        "rounds_inside_count": ric, "expected_rounds_inside": (ric * np.arange(R + 1)).sum(axis=-1) / N,
        "secured_count": sc, "secured_by_proba": sc[..., :R].cumsum(axis=-1) / N,
        "lead_changes_count": lc, "expected_lead_changes": float((lc * np.arange(R)).sum() / N),
    }


TIEBREAKS = ("overall", "head_to_head")
PAIR_HALF = 0xFFFF      # each half of a pair record travels as 16 bits (csrc/dc_h2h.hip.h)
PAIR_MATCH_GOALS = 255  # the sampler's cap on a side's goals in one match


def check_tiebreak(tiebreak) -> bool:
    """`tiebreak` of simulate_season, match_leverage and simulate_tournament: True for "head_to_head"."""
    if not isinstance(tiebreak, str) or tiebreak not in TIEBREAKS:
        raise ValueError(f"tiebreak must be one of {TIEBREAKS}, not {tiebreak!r}")
    return tiebreak == "head_to_head"


def played_matches(played, slot_of) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """`played` (a dict with home_team, away_team, home_goals, away_goals) checked and resolved through
    `slot_of` (team -> table slot): (home slots, away slots, home goals, away goals) as int64.  ValueError for a
    missing column, unequal lengths, a team that is unknown or outside the table, a team playing itself, or
    goals that are not non-negative integers."""
    try:
        cols = [list(played[k]) for k in ("home_team", "away_team", "home_goals", "away_goals")]
    except (KeyError, TypeError, IndexError):
        raise ValueError("played must have home_team, away_team, home_goals and away_goals") from None
    if len({len(c) for c in cols}) != 1:
        raise ValueError("played: home_team, away_team, home_goals and away_goals must have equal length")
    m = len(cols[0])
    out = np.zeros((4, m), dtype=np.int64)
    for f, (home, away, x, y) in enumerate(zip(*cols)):
        for t in (home, away):
            try:
                known = t in slot_of
            except TypeError:
                known = False
            if not known:
                raise ValueError(f"played[{f}]: {t!r} is unknown or outside the table")
        if slot_of[home] == slot_of[away]:
            raise ValueError(f"played[{f}]: a team cannot play itself")
        for g in (x, y):
            ok = not isinstance(g, (bool, np.bool_)) and isinstance(g, (int, float, np.integer, np.floating))
            if not ok or not np.isfinite(g) or int(g) != g or g < 0:
                raise ValueError(f"played[{f}]: goals must be non-negative integers, not {g!r}")
        out[:, f] = (slot_of[home], slot_of[away], int(x), int(y))
    return out[0], out[1], out[2], out[3]


def pair_records(played, slot_of, n: int, points, remaining=None) -> np.ndarray:
    """The pair records of the matches already played, as the head-to-head entry points take them: uint32
    [n, n], row i column k = the points slot i took from slot k << 16 | the goals i scored against k, summed
    over every match between the two (either venue).  `slot_of` maps a team to its slot, `points` is (win,
    draw, loss); `played` None gives zeros.  `remaining` [n, n] counts the meetings of each pair still to be
    simulated (default none): ValueError when, for an ordered pair, points + meetings x max(points) or goals +
    meetings x 255 can pass the 16 bits of its half, besides the errors of `played_matches`."""
    win, draw, loss = check_points(points)
    pts = np.zeros((n, n), dtype=np.int64)
    gls = np.zeros((n, n), dtype=np.int64)
    if played is not None:
        hs, as_, x, y = played_matches(played, slot_of)
        if hs.size and max(int(hs.max()), int(as_.max())) >= n:
            raise ValueError("played: a slot outside the table")
        np.add.at(pts, (hs, as_), np.where(x > y, win, np.where(x == y, draw, loss)))
        np.add.at(pts, (as_, hs), np.where(y > x, win, np.where(x == y, draw, loss)))
        np.add.at(gls, (hs, as_), x)
        np.add.at(gls, (as_, hs), y)
    meet = np.zeros((n, n), dtype=np.int64) if remaining is None else np.asarray(remaining, dtype=np.int64).reshape(n, n)
    off = ~np.eye(n, dtype=bool)
    bad = off & ((pts + meet * max(win, draw, loss) > PAIR_HALF) | (gls + meet * PAIR_MATCH_GOALS > PAIR_HALF))
    if bad.any():
        i, k = (int(v) for v in np.argwhere(bad)[0])
        raise ValueError(f"the pair record of slots {i} and {k} can pass 16 bits "
                         f"({int(pts[i, k])} points, {int(gls[i, k])} goals played, {int(meet[i, k])} meetings to come)")
    return ((pts << 16) | gls).astype(np.uint32)


def remaining_meetings(home_slot, away_slot, n: int) -> np.ndarray:
    """[n, n] int64: how often each pair of slots still meets among the fixtures (symmetric)."""
    meet = np.zeros((n, n), dtype=np.int64)
    hs, as_ = np.asarray(home_slot, dtype=np.int64), np.asarray(away_slot, dtype=np.int64)
    np.add.at(meet, (hs, as_), 1)
    np.add.at(meet, (as_, hs), 1)
    return meet


def table_from_played(played, slot_of, n: int, points) -> np.ndarray:
    """[n, 3] int64 (points, goals for, goals against) of the matches in `played`."""
    win, draw, loss = check_points(points)
    hs, as_, x, y = played_matches(played, slot_of)
    table = np.zeros((n, 3), dtype=np.int64)
    np.add.at(table[:, 0], hs, np.where(x > y, win, np.where(x == y, draw, loss)))
    np.add.at(table[:, 0], as_, np.where(y > x, win, np.where(x == y, draw, loss)))
    np.add.at(table[:, 1], hs, x)
    np.add.at(table[:, 1], as_, y)
    np.add.at(table[:, 2], hs, y)
    np.add.at(table[:, 2], as_, x)
    return table


PLAYOFF_MAX_ROUNDS = 6
PLAYOFF_MAX_SLOTS = 64                 # table rows plus guests (csrc/dc_playoff.hip.h)
PLAYOFF_GUEST, PLAYOFF_BYE = 0x8000, 0xFFFF   # bracket codes (BPLHIP_PLAYOFF_GUEST / _BYE)
PLAYOFF_EXTRA_TIME_SCALE = 1.0 / 3.0
PLAYOFF_MAX_STRENGTH = 20.0            # |shoot-out strength| (BPLHIP_TOURNAMENT_MAX_STRENGTH)
PLAYOFF_VENUES = ("seed", "neutral")
PLAYOFF_KEYS = ("bracket", "legs", "venue", "extra_time_scale", "shootout", "away_goals")


# pylint: disable=too-many-locals,too-many-branches,too-many-statements
def playoff_inputs(playoffs, table_idx, teams_dict) -> dict:
    """simulate_season's `playoffs` checked and resolved on the host, for a table whose rows are the model
    indices `table_idx` and a model that knows `teams_dict` (name -> index).  Returns a dict: "rounds",
    "bracket" (uint16 codes of bplhip_simulate_season_playoff: a finishing position, PLAYOFF_GUEST | i,
    PLAYOFF_BYE), "guests" (uint16 model indices, in bracket order), "guest_names", "legs" [R] (1 / 2),
    "legs_mask", "venue" (R names), "neutral_mask", "extra_time_scale", "strength" float64 [n + guests] (table
    rows, then guests) and "away_goals".  ValueError for everything malformed."""
    def is_int(v):
        return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))

    def is_real(v):
        return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))

    if not isinstance(playoffs, dict):
        raise ValueError("playoffs must be None or a dict")
    unknown = [k for k in playoffs if k not in PLAYOFF_KEYS]
    if unknown:
        raise ValueError(f"playoffs: unknown keys {unknown!r} (known: {PLAYOFF_KEYS})")
    if "bracket" not in playoffs:
        raise ValueError('playoffs needs "bracket"')
    try:
        entries = list(playoffs["bracket"])
    except TypeError:
        raise ValueError("playoffs['bracket'] must be a sequence") from None
    if isinstance(playoffs["bracket"], (str, dict)):
        raise ValueError("playoffs['bracket'] must be a sequence of positions, guest names and None")
    nb = len(entries)
    rounds = nb.bit_length() - 1
    if nb < 2 or nb != 1 << rounds or rounds > PLAYOFF_MAX_ROUNDS:
        raise ValueError(f"playoffs['bracket'] must have 2**R entries, 1 <= R <= {PLAYOFF_MAX_ROUNDS}, not {nb}")
    table_idx = np.asarray(table_idx).astype(np.int64)
    n = table_idx.size
    in_table = set(int(i) for i in table_idx)
    codes = np.zeros(nb, dtype=np.uint16)
    guests, guest_names, positions = [], [], set()
    for b, entry in enumerate(entries):
        if entry is None:
            if b & 1 and entries[b - 1] is None:
                raise ValueError(f"playoffs['bracket']: entries {b - 1} and {b} are both byes")
            codes[b] = PLAYOFF_BYE
        elif isinstance(entry, str):
            if entry not in teams_dict:
                raise ValueError(f"playoffs['bracket'][{b}]: the model does not know {entry!r}")
            idx = int(teams_dict[entry])
            if idx in in_table:
                raise ValueError(f"playoffs['bracket'][{b}]: {entry!r} is a row of the table, not a guest "
                                 "(table teams enter by finishing position)")
            if idx in guests:
                raise ValueError(f"playoffs['bracket'][{b}]: guest {entry!r} appears twice")
            codes[b] = PLAYOFF_GUEST | len(guests)
            guests.append(idx)
            guest_names.append(entry)
        elif is_int(entry):
            pos = int(entry) + n if entry < 0 else int(entry)
            if not 0 <= pos < n:
                raise ValueError(f"playoffs['bracket'][{b}]: position {int(entry)} is outside a table of {n}")
            if pos in positions:
                raise ValueError(f"playoffs['bracket'][{b}]: position {int(entry)} appears twice")
            positions.add(pos)
            codes[b] = pos
        else:
            raise ValueError(f"playoffs['bracket'][{b}] must be a position (int), a guest (str) or None, not {entry!r}")
    if n + len(guests) > PLAYOFF_MAX_SLOTS:
        raise ValueError(f"table rows plus guests number at most {PLAYOFF_MAX_SLOTS}, not {n + len(guests)}")

    legs = playoffs.get("legs")
    if legs is None or is_int(legs):
        legs = [1 if legs is None else legs] * rounds
    try:
        legs = list(legs)
    except TypeError:
        raise ValueError("playoffs['legs'] must be 1, 2 or one of them per round") from None
    if isinstance(playoffs.get("legs"), (str, dict)) or len(legs) != rounds \
            or not all(is_int(v) and int(v) in (1, 2) for v in legs):
        raise ValueError(f"playoffs['legs'] must be 1, 2 or {rounds} values of 1 / 2, first round first")
    venue = playoffs.get("venue", "seed")
    if isinstance(venue, str):
        venue = [venue] * rounds
    elif isinstance(venue, dict) or venue is None:
        raise ValueError(f"playoffs['venue'] must be one of {PLAYOFF_VENUES} or one of them per round")
    try:
        venue = list(venue)
    except TypeError:
        raise ValueError(f"playoffs['venue'] must be one of {PLAYOFF_VENUES} or one of them per round") from None
    if len(venue) != rounds or not all(isinstance(v, str) and v in PLAYOFF_VENUES for v in venue):
        raise ValueError(f"playoffs['venue'] must be one of {PLAYOFF_VENUES} or {rounds} of them, first round first")
    scale = playoffs.get("extra_time_scale", PLAYOFF_EXTRA_TIME_SCALE)
    if not is_real(scale) or not 0.0 < float(scale) <= 1.0:
        raise ValueError("playoffs['extra_time_scale'] must be a number in (0, 1]")
    away_goals = playoffs.get("away_goals", False)
    if not isinstance(away_goals, (bool, np.bool_)):
        raise ValueError("playoffs['away_goals'] must be True or False")
    shootout = playoffs.get("shootout")
    if shootout is not None and not isinstance(shootout, dict):
        raise ValueError("playoffs['shootout'] must be a dict {team: strength}")
    slot = {int(t): i for i, t in enumerate(table_idx)}
    slot.update({t: n + i for i, t in enumerate(guests)})
    strength = np.zeros(n + len(guests), dtype=np.float64)
    for name, v in (shootout or {}).items():
        if not isinstance(name, str) or name not in teams_dict:
            raise ValueError(f"playoffs['shootout']: the model does not know {name!r}")
        if int(teams_dict[name]) not in slot:
            raise ValueError(f"playoffs['shootout']: {name!r} is neither a row of the table nor a guest")
        if not is_real(v) or not abs(float(v)) <= PLAYOFF_MAX_STRENGTH:
            raise ValueError(f"playoffs['shootout'][{name!r}] must be a finite number, at most "
                             f"{PLAYOFF_MAX_STRENGTH:g} in size")
        strength[slot[int(teams_dict[name])]] = float(v)
    return {
        "rounds": rounds, "bracket": codes, "guests": np.array(guests, dtype=np.uint16), "guest_names": guest_names,
        "legs": np.array(legs, dtype=np.uint8), "legs_mask": sum(1 << r for r, v in enumerate(legs) if int(v) == 2),
        "venue": venue, "neutral_mask": sum(1 << r for r, v in enumerate(venue) if v == "neutral"),
        "extra_time_scale": float(scale), "strength": strength, "away_goals": bool(away_goals),
    }


def playoff_result(inp, raw, n_sims: int) -> Dict[str, np.ndarray]:
    """simulate_season's play-off keys from the integer counts: `raw` has "stage_counts" [n + g, R + 2] and
    "decided_counts" [R, 4] (and the per-simulation records when they were asked for)."""
    R = inp["rounds"]
    stage = np.asarray(raw["stage_counts"]).astype(np.int64)
    decided = np.asarray(raw["decided_counts"]).astype(np.int64)
    reached = stage[:, ::-1].cumsum(axis=1)[:, ::-1]        # column c: stage >= c
    played = decided.sum(axis=1, keepdims=True)
    out = {"playoff_round_proba": reached[:, 1:R + 2] / n_sims,
           "playoff_decided_proba": np.where(played > 0, decided / np.maximum(played, 1), 0.0)}
    for key in ("playoff_stage", "playoff_decided"):
        if key in raw:
            out[key] = raw[key]
    return out


class BaseMatchPredictor(PosteriorOnDevice, _elpd.PointwiseLikelihood, _ppc.PosteriorPredictiveCheck,
                         _scoring.ForecastScores, _markets.PredictMarkets, _inplay.PredictInPlay,
                         _periods.PredictPeriods, _sequential.SequentialScores, _diagnostics.McmcDiagnostics,
                         _ratings.TeamRatings, _slate.PredictSlate, _loo_scores.LooScores,
                         _sensitivity.PowerscaleSensitivity):
    """Common predict API of the team-level models.  A subclass provides `fit` and the four
    posterior arrays (`attack`, `defence` [draws, teams]; `home_advantage` [draws] or
    [draws, teams]; `corr_coef` [draws])."""

    def __init__(self):
        self.teams = None          # sorted unique team names
        self._teams_dict = None    # name -> index

    # ------------------------------------------------------------------ plumbing
    def fit(self, training_data, **kwargs) -> "BaseMatchPredictor":
        raise NotImplementedError("subclasses implement fit()")

    def _team_indices(self, *team_args: TeamArg):
        """Names (or ready indices), scalar or iterable -> uint16 index arrays.  Unknown names
        raise KeyError, as the reference's dictionary lookup does."""
        out = []
        for arg in team_args:
            items = [arg] if isinstance(arg, (str, int, np.integer)) else list(arg)
            out.append(np.fromiter((self._teams_dict[t] if isinstance(t, str) else int(t) for t in items),
                                   dtype=DTYPES["teams"], count=len(items)))
        return out if len(out) > 1 else out[0]

    # (name kept: the reference's helper of the same role, bpl/base.py:62-72)
    def _parse_fixture_args(self, home_team: TeamArg, away_team: TeamArg):
        return tuple(self._team_indices(home_team, away_team))

    def _posterior_arrays(self):
        return (self.attack, self.defence, self.home_advantage, self.corr_coef)

    def _upload_posterior(self, ctx):
        ctx.predict_set_posterior(self.attack, self.defence, self.home_advantage, self.corr_coef)

    def _fixture_groups(self, data, with_goals: bool):
        """log_likelihood / waic / loo (with the goals), predict_markets (without): data's home_team,
        away_team[, home_goals, away_goals] checked on the host (bpl/elpd.py)."""
        n = _elpd.fixture_count(data, ("home_team", "away_team") + (("home_goals", "away_goals") if with_goals else ()))
        kwargs = {"home_idx": _elpd.lookup(data["home_team"], self._teams_dict, n),
                  "away_idx": _elpd.lookup(data["away_team"], self._teams_dict, n)}
        if with_goals:
            kwargs.update(home_goals=_elpd.goals(data["home_goals"], n), away_goals=_elpd.goals(data["away_goals"], n))
        return [(None, self._device, kwargs)], n

    def _calculate_expected_goals(self, home_team: TeamArg, away_team: TeamArg) -> Tuple[np.ndarray, np.ndarray]:
        """Home and away scoring rates, [draws, fixtures] (bpl/dixon_coles.py:126-137,
        bpl/extended_dixon_coles.py:335-358)."""
        h, a = self._team_indices(home_team, away_team)
        edge = self.home_advantage[:, None] if np.ndim(self.home_advantage) == 1 else self.home_advantage[:, h]
        log_home = self.attack[:, h] - self.defence[:, a] + edge
        log_away = self.attack[:, a] - self.defence[:, h]
        return np.exp(log_home), np.exp(log_away)

    # ------------------------------------------------------------------ probabilities
    def predict_score_proba(self, home_team: TeamArg, away_team: TeamArg,
                            home_goals: Union[int, Iterable[int]],
                            away_goals: Union[int, Iterable[int]]) -> np.ndarray:
        """Probability of each requested scoreline: posterior mean of tau * Poisson * Poisson
        (bpl/dixon_coles.py:139-163)."""
        h, a = self._team_indices(home_team, away_team)
        x = np.broadcast_to(np.asarray(home_goals), h.shape)
        y = np.broadcast_to(np.asarray(away_goals), h.shape)
        return self._device().predict_score_proba(h, a, x, y)

    def predict_score_grid_proba(self, home_team: TeamArg, away_team: TeamArg,
                                 max_goals: Optional[int] = MAX_GOALS,
                                 ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(probabilities [fixtures, G+1, G+1], home-goal grid, away-goal grid)
        (bpl/base.py:74-111)."""
        h, a = self._team_indices(home_team, away_team)
        counts = np.arange(max_goals + 1)
        return (score_grid(self._device, h, a, max_goals),) + tuple(np.meshgrid(counts, counts, indexing="ij"))

    def predict_outcome_proba(self, home_team: TeamArg, away_team: TeamArg,
                              max_goals: Optional[int] = MAX_GOALS) -> Dict[str, np.ndarray]:
        """Home win / draw / away win (bpl/base.py:113-148)."""
        h, a = self._team_indices(home_team, away_team)
        return outcome_from_grid(score_grid(self._device, h, a, max_goals))

    def _goal_marginal(self, n, team: TeamArg, opponent: TeamArg, team_is_home: bool,
                       count_team_goals: bool, max_goals: int) -> np.ndarray:
        """P(`team` scores [concedes] n) with the other side's goals summed over 0..max_goals."""
        wanted = goals_wanted(n)
        t, o = self._team_indices(team, opponent)
        depth = max(int(max_goals), int(wanted.max()))
        grid = score_grid(self._device, *((t, o) if team_is_home else (o, t)), depth)[0]
        # axis 0 counts the home side's goals: the team's when it is at home and we count its own
        return goal_marginal(grid, wanted, max_goals, 0 if team_is_home == count_team_goals else 1)

    def predict_score_n_proba(self, n: Union[int, Iterable[int]], team: TeamArg, opponent: TeamArg,
                              home: Optional[bool] = True,
                              max_goals: Optional[int] = MAX_GOALS) -> np.ndarray:
        """Probability that `team` scores n goals against `opponent` (bpl/base.py:248-297)."""
        return self._goal_marginal(n, team, opponent, bool(home), True, max_goals)

    def predict_concede_n_proba(self, n: Union[int, Iterable[int]], team: TeamArg, opponent: TeamArg,
                                home: Optional[bool] = True,
                                max_goals: Optional[int] = MAX_GOALS) -> np.ndarray:
        """Probability that `team` concedes n goals against `opponent` (bpl/base.py:299-348)."""
        return self._goal_marginal(n, team, opponent, bool(home), False, max_goals)

    # ------------------------------------------------------------------ sampling
    def sample_score(self, home_team: TeamArg, away_team: TeamArg, num_samples: int = 1,
                     random_state: int = None, max_goals: Optional[int] = MAX_GOALS,
                     ) -> Dict[str, np.ndarray]:
        """Scorelines drawn from each fixture's grid, [fixtures, num_samples] per side
        (bpl/base.py:150-195)."""
        h, a = self._team_indices(home_team, away_team)
        return draw_scores(score_grid(self._device, h, a, max_goals), max_goals, num_samples, random_state)

    def sample_outcome(self, home_team: TeamArg, away_team: TeamArg, num_samples: int = 1,
                       random_state: int = None, max_goals: Optional[int] = MAX_GOALS) -> np.ndarray:
        """Winner's name, or 'Draw', [fixtures, num_samples] (bpl/base.py:197-246)."""
        h, a = self._team_indices(home_team, away_team)
        return draw_winners(self.predict_outcome_proba(h, a, max_goals=max_goals), h, a, self.teams, num_samples,
                            random_state)

    # ------------------------------------------------------------------ season simulation
    def _season_inputs(self, home_team: TeamArg, away_team: TeamArg, num_simulations, current_table,
                       teams, points):
        """simulate_season's arguments checked and resolved on the host: (home, away, table slots as
        model indices, [n, 3] current table, (win, draw, loss), num_simulations)."""
        h, a = self._team_indices(home_team, away_team)
        if h.size != a.size:
            raise ValueError("home_team and away_team must have equal length")
        n_model = len(self.teams)
        if h.size and max(int(h.max()), int(a.max())) >= n_model:
            raise ValueError("team index out of range")
        if h.size > SEASON_MAX_FIXTURES:
            raise ValueError(f"at most {SEASON_MAX_FIXTURES} fixtures")
        if np.any(h == a):
            raise ValueError("a team cannot play itself")
        num_simulations = check_simulations(num_simulations)
        points = check_points(points)
        rows = {}
        for name, entry in (current_table or {}).items():
            idx = int(self._team_indices(name)[0])
            if idx >= n_model:
                raise ValueError("team index out of range")
            vals = tuple(entry)
            if len(vals) != 3 or any(isinstance(v, (bool, np.bool_)) or int(v) != v for v in vals):
                raise ValueError(f"current_table[{name!r}] must be (points, goals_for, goals_against) integers")
            vals = tuple(int(v) for v in vals)
            if any(not 0 <= v <= SEASON_MAX_TABLE_VALUE for v in vals):
                raise ValueError(f"current_table[{name!r}] entries must be in [0, {SEASON_MAX_TABLE_VALUE}]")
            rows[idx] = vals
        if teams is None:
            table_idx = np.union1d(np.union1d(h, a), np.fromiter(rows, dtype=np.int64, count=len(rows)))
        else:
            table_idx = np.unique(self._team_indices(teams).astype(np.int64))
            if table_idx.size and table_idx.max() >= n_model:
                raise ValueError("team index out of range")
        n = table_idx.size
        if not 1 <= n <= SEASON_MAX_TEAMS:
            raise ValueError(f"the table must have 1..{SEASON_MAX_TEAMS} teams, not {n}")
        in_table = np.zeros(n_model, dtype=bool)
        in_table[table_idx] = True
        if not (in_table[h].all() and in_table[a].all()):
            raise ValueError("every fixture's teams must be in the table")
        if not all(in_table[i] for i in rows):
            raise ValueError("every current_table team must be in the table")
        table = np.array([rows.get(int(i), (0, 0, 0)) for i in table_idx], dtype=np.int64).reshape(n, 3)
        return h, a, table_idx.astype(DTYPES["teams"]), table, points, num_simulations

    def _season_h2h_inputs(self, home_team, away_team, num_simulations, current_table, teams, points, tiebreak,
                           played):
        """`_season_inputs` with `tiebreak` and `played`: its six results, then head_to_head (bool) and the
        pair records uint32 [n, n] (None unless head_to_head).  Everything is checked here, before any
        device call."""
        head_to_head = check_tiebreak(tiebreak)
        if played is not None:
            by_name = {str(t): i for i, t in enumerate(self.teams)}
            hs, as_, _, _ = played_matches(played, by_name)
            if current_table is None:
                # the current table is what `played` adds up to (its teams become table rows)
                totals = table_from_played(played, by_name, len(by_name), check_points(points))
                current_table = {str(self.teams[i]): tuple(int(v) for v in totals[i])
                                 for i in np.union1d(hs, as_)}
        h, a, table_idx, table, points, n_sims = self._season_inputs(
            home_team, away_team, num_simulations, current_table, teams, points)
        pair = None
        if head_to_head:
            n = table_idx.size
            slot_of = {str(self.teams[int(t)]): i for i, t in enumerate(table_idx)}
            slot = np.full(len(self.teams), -1, dtype=np.int64)
            slot[table_idx.astype(np.int64)] = np.arange(n)
            pair = pair_records(played, slot_of, n, points, remaining=remaining_meetings(slot[h], slot[a], n))
        elif played is not None:
            played_matches(played, {str(self.teams[int(t)]): i for i, t in enumerate(table_idx)})
        return h, a, table_idx, table, points, n_sims, head_to_head, pair

    def _in_play_inputs(self, in_play):
        """simulate_season's `in_play` checked and resolved on the host: (home, away model indices uint16, home,
        away goals uint8, elapsed float64), each [L]; None gives L = 0.  ValueError for a missing column, unequal
        lengths, an unknown team, a team playing itself, goals that are not integers in 0..LIVE_MAX_GOALS, an
        elapsed outside [0, 1) or 0 away from 0-0."""
        if in_play is None:
            in_play = {k: () for k in ("home_team", "away_team", "home_goals", "away_goals", "elapsed")}
        try:
            cols = [in_play[k] for k in ("home_team", "away_team", "home_goals", "away_goals", "elapsed")]
            cols = [[c] if isinstance(c, (str, int, float, np.integer, np.floating)) else list(c) for c in cols]
        except (KeyError, TypeError, IndexError):
            raise ValueError("in_play must have home_team, away_team, home_goals, away_goals and elapsed") from None
        if len({len(c) for c in cols}) != 1:
            raise ValueError("in_play: every column must have the same length")
        try:
            h, a = self._team_indices(cols[0], cols[1])
        except (KeyError, TypeError, ValueError):
            raise ValueError("in_play: unknown team") from None
        if h.size and max(int(h.max()), int(a.max())) >= len(self.teams):
            raise ValueError("in_play: team index out of range")
        if np.any(h == a):
            raise ValueError("in_play: a team cannot play itself")
        goals = []
        for col in cols[2:4]:
            for g in col:
                ok = not isinstance(g, (bool, np.bool_)) and isinstance(g, (int, float, np.integer, np.floating))
                if not ok or not np.isfinite(g) or int(g) != g or not 0 <= g <= LIVE_MAX_GOALS:
                    raise ValueError(f"in_play: current goals must be integers in 0..{LIVE_MAX_GOALS}, not {g!r}")
            goals.append(np.array([int(g) for g in col], dtype=np.uint8))
        t = _inplay.check_elapsed(cols[4], h.size)
        if np.any((t == 0.0) & ((goals[0] != 0) | (goals[1] != 0))):
            raise ValueError("in_play: elapsed = 0 with a score other than 0-0")
        return h, a, goals[0], goals[1], t

    def _live_inputs(self, home_team, away_team, in_play, log_weights):
        """What every live call does first: (`_in_play_inputs`' five columns, the checked log weights or None, the
        CONCATENATED home and away lists as model indices).  The matches in play are fixtures of the concatenated
        list -- table rows, meetings to come, the fixture bound -- so `_season_h2h_inputs` takes the two lists."""
        ip = self._in_play_inputs(in_play)
        lw = _inplay.check_log_weights(log_weights, int(np.asarray(self.corr_coef).shape[0]))
        home = np.concatenate([self._team_indices(home_team), ip[0]])
        away = np.concatenate([self._team_indices(away_team), ip[1]])
        return ip, lw, home, away

    def simulate_season(self, home_team: TeamArg, away_team: TeamArg, num_simulations: int = 10_000,
                        random_state: int = None, current_table: Optional[Dict] = None,
                        teams: Optional[TeamArg] = None, points: Tuple[int, int, int] = (3, 1, 0),
                        return_tables: bool = False, return_scores: bool = False, tiebreak: str = "overall",
                        played: Optional[Dict] = None, playoffs: Optional[Dict] = None,
                        in_play: Optional[Dict] = None, reweight: bool = True, log_weights=None,
                        return_weights: bool = False) -> Dict[str, np.ndarray]:
        """Finishing-position odds from simulating the remaining fixtures (no reference counterpart).

        Each simulated season takes ONE posterior draw (simulation j: draw j mod draws) and plays every
        fixture from it, so the uncertainty all fixtures share stays in the table -- a table built from
        `sample_score` (each fixture drawn on its own from the posterior-mean grid) comes out too narrow.
        A fixture's scoreline is drawn exactly from max(tau, 0) Poisson Poisson / Z with that draw's
        rates (no max_goals truncation); the table adds `points` = (win, draw, loss), goals for and
        against to `current_table` (name -> (points, goals_for, goals_against); missing teams start at
        zero) and is ordered by points, goal difference, goals for, then a random tie-break (the
        head-to-head rule: see `tiebreak`).  `teams` (default: every team of the fixtures and of
        `current_table`) are the table's rows, in the model's (sorted) team order; at most 64.  The device
        kernel is csrc/dc_season.hip.h.

        `tiebreak="head_to_head"` (default "overall": the order above, same kernel and results as without
        the keyword) orders the teams level on points by the matches between them first: points taken from
        the teams level with it, then goal difference and goals scored in those matches, and only then
        overall goal difference, goals for and the random tie-break (csrc/dc_h2h.hip.h).  The mini-table is
        formed once over ALL teams level on points: UEFA's re-application of the criteria to a still-tied
        subset is not modelled, nor is La Liga's omission of the head-to-head goals scored.  `played` (a dict
        with home_team, away_team, home_goals, away_goals, names as in the training data) lists the matches
        already played: it fills the head-to-head records, and when `current_table` is None the current
        table is computed from it with `points`.  With both given `current_table` supplies the totals (points
        deductions stay expressible), `played` only the head-to-head records; the two are not cross-checked.
        ValueError for an unknown team or one outside the table, a team playing itself, unequal lengths,
        goals that are not non-negative integers, or a pair whose record could pass 16 bits (65535 points or
        goals between two teams, counting 255 goals for every meeting to come).

        Returns numpy arrays: "teams" [n]; "position_proba" [n, n] (row = team, column = finishing
        position, 0 = top); "expected_points", "expected_goal_difference" [n]; with return_tables
        "points" int32 and "position" uint8 [num_simulations, n]; with return_scores "home_goals" and
        "away_goals" uint8 [num_simulations, fixtures].

        `playoffs` (default None: nothing changes, the same kernels and results) plays ONE knockout bracket
        after every simulated table, seeded by that table and from the same posterior draw as the league
        run-in (csrc/dc_playoff.hip.h).  It is a dict.  "bracket" (required) is the first round in bracket
        order, 2**R entries with 1 <= R <= 6: entry 2m meets entry 2m + 1 and the winners of matches 2m and
        2m + 1 meet next.  An entry is an int -- a finishing position of this simulation, 0 = top, negative
        from the bottom, each at most once; a str -- a guest, a team the model knows that is NOT a row of the
        table (the club from the division below), each at most once; or None -- a bye: the other entry of the
        pair goes through without a match (two byes cannot be paired).  Table rows plus guests number at most
        64.  A table team's seed is its finishing position in that simulation, a guest's is n + its index among
        the guests in bracket order (worse than every table team), a winner carries its seed on; in every tie
        the better seed is q and the worse seed p.  "legs": None or 1, 2, or R values of 1 / 2 (first round
        first).  "venue": "seed" (default), "neutral", or R of them, read for single-leg rounds only: "seed"
        puts q at home with the home advantage, "neutral" lists p as the home side and leaves the home-advantage
        term out.  A two-legged tie plays leg 1 at p's ground and leg 2 at q's; the higher aggregate goes
        through, with "away_goals" (default False) a level aggregate goes to the side with more away goals.
        Still level, extra time is played at the venue of the only leg or of leg 2 with both rates times
        "extra_time_scale" (default 1/3, in (0, 1]), then the shoot-out: p goes through with probability
        1 / (1 + exp(-(s[p] - s[q]))), s from "shootout" {team: strength} (finite, at most 20 in size, default
        0; a table row or a guest).  The rule is `simulate_tournament(knockout_rule="extra_time")`'s with the
        base classes' rates; there is no redraw rule here.  Unknown keys and everything malformed raise
        ValueError before any device call.

        With `playoffs` the result also has "playoff_teams" [n + g] (table rows, then guests);
        "playoff_round_proba" [n + g, R + 1] (column r: P(the team is in round r, by a match or a bye);
        column R: P(it wins the bracket)); "playoff_decided_proba" [R, 4] (the shares of the matches actually
        played in round r decided in normal time / by away goals / in extra time / by the shoot-out); with
        return_tables "playoff_stage" uint8 [num_simulations, n + g] (0 = not in the bracket, r + 1 = the
        furthest round entered was r, R + 1 = winner) and "playoff_decided" uint8 [num_simulations, 2**R - 1]
        (0..3 as above per bracket match, 255 for a bye).  Every other key is bit for bit what the call without
        `playoffs` returns under the same random_state.  The Championship (24 teams; two go up, 3rd to 6th play
        off): playoffs={"bracket": [5, 2, 4, 3], "legs": (2, 1), "venue": ("seed", "neutral")} gives
        P(promoted) = position_proba[:, :2].sum(1) + playoff_round_proba[:n, R] with R = 2.

        Out of scope: re-seeding or a draw between rounds, a third-place match, more than one bracket per
        call, play-offs in `match_leverage` and `points_needed`, and play-offs in the neutral classes.

        `in_play` (default None), `log_weights` (default None) and `reweight`: the table on a day with matches
        IN PROGRESS, and posterior draws that carry weights (csrc/dc_live.hip.h).  With
        `in_play=None`, `log_weights=None` and `return_weights=False` nothing changes: the same kernels, the same
        results, the same keys.  `in_play` is a dict with home_team, away_team, home_goals,
        away_goals (the CURRENT score, integers in 0..63) and elapsed (the fraction of the match played, in
        [0, 1); 0 only at 0-0 -- `predict_in_play`'s rule), each of length L >= 0.  These matches come IN ADDITION
        to the positional fixtures (those still to kick off): `current_table` and `played` describe the table
        WITHOUT them -- their current goals are not in it, the final score is booked once -- and both teams of
        each must be rows of the table (with `teams=None` they become rows).  Under `tiebreak="head_to_head"`
        they are booked into the head-to-head records like any fixture and count as meetings to come in the
        16-bit bound.  A match in progress draws its FINAL score from that draw's conditional law given the state:
        remaining goals Poisson with the rates thinned by 1 - elapsed, the Dixon-Coles factor on the final score
        with the full-match rates (`predict_in_play`'s law, sampled exactly); it is fixture F + m of the
        concatenated list and takes that fixture's random block, so at 0-0 and elapsed = 0 it IS that fixture.
        With `reweight` (read only when L > 0) draw s is weighted by the JOINT likelihood of all the states,
        exp(sum_m l[s, m]) with `predict_in_play`'s l -- one update over all matches in progress, which that
        method leaves out; `log_weights` [draws], all finite (a row of `sequential_scores(return_weights=True)
        ["log_weights"]`, say), is added to the log weights, with `in_play=None` too: the updated-without-a-refit
        season.  Weights are IN FORCE when `log_weights` is given or (`reweight` and L > 0).  Then the draws are
        resampled on the device by systematic resampling: with w[s] = exp(L[s] - max L), C its running sum in
        draw order, W its total and ONE uniform U per call, simulation j takes the first draw whose C reaches
        (j + U) W / num_simulations -- draw s is used floor or ceil of num_simulations w[s] / W times, a draw of
        weight 0 never.  Without weights in force simulation j takes draw j mod draws, as ever.  Either way every
        simulation is an EQUALLY weighted draw from the (updated) posterior predictive: all counts stay integers
        and every output is bit-identical run to run.

        With any of them given the result also has "ess" (float: (sum w)^2 / sum w^2; the number of draws without weights in force);
        "log_evidence" (float: the posterior-predictive log probability of all states jointly, 0.0 when L = 0; NaN
        when L > 0 and no weights are in force -- `reweight=False` without `log_weights` evaluates no likelihood);
        with return_tables "draw" int32 [num_simulations]; with return_scores "in_play_home_goals" and
        "in_play_away_goals" uint8 [num_simulations, L] (FINAL scores; "home_goals" / "away_goals" keep the
        positional fixtures); with `return_weights` "log_weights" float64 [draws] = L - max L, which
        `predict_in_play(reweight=False, log_weights=...)` takes: its markets under the joint update.

        Out of scope: `in_play`, `log_weights` or `return_weights` together with `playoffs` (ValueError:
        not supported together), `season_trajectory`, `simulate_tournament`, and the neutral and dynamic classes.
        `match_leverage`, `points_needed` and `match_scenarios` take `in_play`, `reweight` and `log_weights` with this
        meaning (csrc/dc_live_queries.hip.h)."""
        live = in_play is not None or log_weights is not None or bool(return_weights)
        if live and playoffs is not None:
            raise ValueError("in_play / log_weights / return_weights and playoffs are not supported together")
        if live:
            ip, lw, home_team, away_team = self._live_inputs(home_team, away_team, in_play, log_weights)
        h, a, table_idx, table, points, n_sims, head_to_head, pair = self._season_h2h_inputs(
            home_team, away_team, num_simulations, current_table, teams, points, tiebreak, played)
        if live:
            return self._simulate_season_live(h, a, ip, table_idx, table, points, n_sims, random_state, head_to_head,
                                              pair, bool(reweight), lw, return_tables, return_scores, return_weights)
        po = None if playoffs is None else playoff_inputs(playoffs, table_idx, self._teams_dict)
        seed = _wall_clock_seed() if random_state is None else random_state
        extra = {"pair_init": pair, "head_to_head": True} if head_to_head else {}
        if po is not None:
            extra["playoff"] = {"guests": po["guests"], "bracket": po["bracket"], "legs_mask": po["legs_mask"],
                                "neutral_mask": po["neutral_mask"], "scale": po["extra_time_scale"],
                                "away_goals": po["away_goals"], "strength": po["strength"]}
        raw = self._device().simulate_season(h, a, table_idx, table, points, n_sims, prng_key(seed),
                                             return_tables=return_tables, return_scores=return_scores, **extra)
        out = {
            "teams": np.asarray(self.teams)[table_idx],
            "position_proba": raw["counts"] / n_sims,
            "expected_points": raw["points_sum"] / n_sims,
            "expected_goal_difference": raw["gd_sum"] / n_sims,
        }
        for key in ("points", "position", "home_goals", "away_goals"):
            if key in raw:
                out[key] = raw[key]
        if po is not None:
            out["playoff_teams"] = np.asarray(self.teams)[np.concatenate([table_idx, po["guests"]]).astype(np.int64)]
            out.update(playoff_result(po, raw, n_sims))
        return out

    def _simulate_season_live(self, h, a, ip, table_idx, table, points, n_sims, random_state, head_to_head, pair,
                              reweight, lw, return_tables, return_scores, return_weights):
        """simulate_season through csrc/dc_live.hip.h: `h`, `a` the concatenated list whose last len(ip[0])
        entries are the matches in play `ip`; everything has been checked."""
        n_live = ip[0].size
        nf = h.size - n_live
        seed = _wall_clock_seed() if random_state is None else random_state
        extra = {"pair_init": pair, "head_to_head": True} if head_to_head else {}
        raw = self._device().simulate_season_live(
            h[:nf], a[:nf], table_idx, table, points, n_sims, prng_key(seed), in_play=ip, reweight=reweight,
            log_weights=lw, return_tables=return_tables, return_scores=return_scores,
            return_weights=bool(return_weights), **extra)
        out = {
            "teams": np.asarray(self.teams)[table_idx],
            "position_proba": raw["counts"] / n_sims,
            "expected_points": raw["points_sum"] / n_sims,
            "expected_goal_difference": raw["gd_sum"] / n_sims,
            "ess": float(raw["ess"]),
            "log_evidence": float(raw["log_evidence"]),
        }
        for key in ("points", "position", "draw", "home_goals", "away_goals", "in_play_home_goals",
                    "in_play_away_goals"):
            if key in raw:
                out[key] = raw[key]
        if return_weights:
            out["log_weights"] = raw["L"] - raw["L"].max()
        return out

    def match_leverage(self, home_team: TeamArg, away_team: TeamArg, num_simulations: int = 10_000,
                       random_state: int = None, current_table: Optional[Dict] = None,
                       teams: Optional[TeamArg] = None, points: Tuple[int, int, int] = (3, 1, 0),
                       targets: Optional[Dict] = None, tiebreak: str = "overall",
                       played: Optional[Dict] = None, in_play: Optional[Dict] = None, reweight: bool = True,
                       log_weights=None) -> Dict[str, np.ndarray]:
        """Which remaining fixtures decide the table: every fixture's result cross-tabulated against every
        team's finishing-position targets, over `simulate_season`'s simulations (no reference counterpart).

        The first seven arguments are `simulate_season`'s, and under the same `random_state` and arguments
        simulation j here IS simulation j there (the same draw, scorelines, tie-break and ranking); only
        the counting differs, and it happens on the device (csrc/dc_leverage.hip.h): no per-simulation
        array comes back.  `targets` maps a name to finishing positions, 0 = top, negative = from the
        bottom as Python indices; duplicates merge, positions outside the table are dropped, a target left
        empty raises ValueError, as do fewer than 1 or more than 8 targets.  Default: "title" (0,),
        "top_four" (0..3), "relegation" (the last three).  At most 4096 fixtures.  `tiebreak` and `played`
        are `simulate_season`'s: with "head_to_head" the positions are those of its head-to-head order.

        Returns numpy arrays (F fixtures in the order given, n table rows, K targets, N simulations,
        o = 0 home win, 1 draw, 2 away win): "teams" [n]; "targets" [K]; "outcome_count" int64 [F, 3] and
        "outcome_proba" = / N; "target_count" int64 [n, K] (team t finished inside target k) and
        "target_proba"; "joint_count" int64 [F, 3, n, K] (fixture f ended o AND t finished inside k);
        "conditional_proba" = joint_count / outcome_count and its binomial "conditional_se"
        sqrt(p (1 - p) / outcome_count), both NaN where the outcome never occurred; "leverage" [F, n, K] =
        sum_o outcome_proba |conditional_proba - target_proba| over the outcomes that occurred: the
        expected absolute movement of t's odds once f's result is known, 0 where f cannot matter.

        The conditional is the POSTERIOR-PREDICTIVE one: a simulation plays all fixtures from one
        posterior draw, so a result also says something about how strong the two teams are, and with it
        moves every other fixture of theirs -- intended: it is what the joint simulation buys over
        per-fixture arithmetic.  The derived floats are formed here from the integer counts.

        `in_play`, `reweight` and `log_weights` (defaults None, True, None: nothing changes, the same entry point,
        kernels, results and keys) are `simulate_season`'s, with its meaning, checks and error messages: the leverage
        of a day with matches IN PROGRESS, and of posterior draws that carry weights (csrc/dc_live_queries.hip.h).
        The fixture list becomes the F positional fixtures followed by the L matches in play (F + L at most 4096);
        `current_table` and `played` leave the matches in play out, and those count as meetings to come in the
        head-to-head bound.  Under the same `random_state` and arguments simulation j here IS simulation j of
        `simulate_season(in_play=..., reweight=..., log_weights=...)`, in both tie-break modes: the same draw (weights
        are in force when `log_weights` is given, or `reweight` and L > 0), the same final scores of the matches in
        play, the same tie-break and ranking.  The fixture axis then has F + L rows, the matches in play last, each
        classified by its FINAL score, and the result gains "in_play" (int64 [L]: their rows on that axis), "ess" and
        "log_evidence" (`simulate_season`'s values and conventions: the number of draws, and NaN with L > 0 / 0.0
        with L = 0, when no weights are in force).  The weights themselves come from `simulate_season(
        return_weights=True)`.

        Not modelled: `playoffs`; `in_play` and `log_weights` in `season_trajectory` (a match in play would need a
        matchday label, and that kernel walks by blocks of matchdays), in `simulate_season(playoffs=...)`, in the
        tournament family, and in the neutral and dynamic classes."""
        live = in_play is not None or log_weights is not None or not reweight
        if live:
            ip, lw, home_team, away_team = self._live_inputs(home_team, away_team, in_play, log_weights)
        h, a, table_idx, table, points, n_sims, head_to_head, pair = self._season_h2h_inputs(
            home_team, away_team, num_simulations, current_table, teams, points, tiebreak, played)
        if h.size > LEVERAGE_MAX_FIXTURES:
            raise ValueError(f"at most {LEVERAGE_MAX_FIXTURES} fixtures")
        names, masks = leverage_targets(targets, table_idx.size)
        seed = _wall_clock_seed() if random_state is None else random_state
        extra = {"pair_init": pair, "head_to_head": True} if head_to_head else {}
        out = {"teams": np.asarray(self.teams)[table_idx], "targets": np.asarray(names)}
        if live:
            nf = h.size - ip[0].size
            raw = self._device().match_leverage_live(h[:nf], a[:nf], table_idx, table, points, n_sims, prng_key(seed),
                                                     masks, in_play=ip, reweight=bool(reweight), log_weights=lw,
                                                     **extra)
            out.update(in_play=np.arange(nf, h.size, dtype=np.int64), ess=float(raw["ess"]),
                       log_evidence=float(raw["log_evidence"]))
        else:
            raw = self._device().match_leverage(h, a, table_idx, table, points, n_sims, prng_key(seed), masks, **extra)
        out.update(leverage_from_counts(raw["outcome"], raw["target"], raw["joint"], n_sims))
        return out

    def points_needed(self, home_team: TeamArg, away_team: TeamArg, num_simulations: int = 10_000,
                      random_state: int = None, current_table: Optional[Dict] = None,
                      teams: Optional[TeamArg] = None, points: Tuple[int, int, int] = (3, 1, 0),
                      targets: Optional[Dict] = None, tiebreak: str = "overall", played: Optional[Dict] = None,
                      levels=(0.5, 0.9, 0.99), in_play: Optional[Dict] = None, reweight: bool = True,
                      log_weights=None) -> Dict[str, np.ndarray]:
        """How many points it takes: every team's final points total cross-tabulated against its
        finishing-position targets, the points of every finishing position and the gap between neighbouring
        positions, over `simulate_season`'s simulations (no reference counterpart).

        All arguments but `levels` are `match_leverage`'s, under its rules and defaults (1..8 targets, at most
        4096 fixtures), and under the same `random_state` simulation j here IS simulation j of `simulate_season`
        and `match_leverage` (the same draw, scorelines, tie-break and ranking, in both tie-break modes); the
        counting happens on the device (csrc/dc_points.hip.h) and no per-simulation array comes back.  `levels`
        is non-empty with every value in (0, 1] (ValueError otherwise).  The points axis: a team with m
        remaining matches ends on its current points + m min(points) .. + m max(points); "points" [P] runs from
        the least of these over the table to the largest, and P above 1024 raises ValueError.

        Returns numpy arrays (n table rows, K targets, L levels, P bins, N simulations): "teams" [n]; "targets"
        [K]; "levels" [L]; "points" [P]; the integer tables from the device, int64: "team_points_count" [n, P]
        (team t ended on p), "team_target_count" [n, P, K] (and inside target k), "position_points_count" [n, P]
        (the team finishing in position k, 0 = top, had p points), "gap_count" [n - 1, P] (the points of position k
        minus those of position k + 1, column 0 = level on points: decided by the tie-break); and from those
        integers "team_points_proba"; "target_count" [n, K] = team_target_count.sum(1) and "target_proba";
        "proba_given_points" [n, P, K] = team_target_count / team_points_count with its binomial
        "se_given_points", NaN where the team never ended on p; "proba_given_at_least" [n, P, K] = P(inside k |
        at least p points), NaN where the team never reached p; "points_needed" [n, K, L]: the smallest points
        value p of the axis that the team reached or passed at least once and from which P(inside k | at least p
        points) >= level, NaN when there is none; "position_points_mean" [n]; "position_points_quantile" int64 [L, n] (the inverted CDF of the counts at
        `levels`: an order statistic, no interpolation); "level_proba" [n - 1] = gap_count[:, 0] / N.

        `points_needed` reads "AT LEAST p points", so it is meaningful for targets one wants to be inside: for
        survival pass targets={"safe": range(0, n - 3)}, not the default "relegation".  Like every conditional
        here it is the posterior-predictive one: reaching p points also says something about the team's strength.

        `in_play`, `reweight` and `log_weights` (defaults None, True, None: nothing changes, the same entry point,
        kernels, results and keys) are `match_leverage`'s, which are `simulate_season`'s: whether the points a side is
        on will be enough, asked with matches IN PROGRESS or of weighted draws (csrc/dc_live_queries.hip.h).  The
        tables are unchanged; the matches in play are fixtures F .. F + L - 1 of the concatenated list, remaining
        matches on the points axis (`current_table` leaves them out, their final score is booked once), and
        simulation j is simulation j of `simulate_season` and `match_leverage` under the same live arguments.  The
        result gains "ess" and "log_evidence", as there.

        Not modelled: `playoffs`; `in_play` and `log_weights` in `season_trajectory`, `simulate_season(playoffs=...)`,
        the tournament family and the neutral and dynamic classes."""
        live = in_play is not None or log_weights is not None or not reweight
        if live:
            ip, lw, home_team, away_team = self._live_inputs(home_team, away_team, in_play, log_weights)
        h, a, table_idx, table, points, n_sims, head_to_head, pair = self._season_h2h_inputs(
            home_team, away_team, num_simulations, current_table, teams, points, tiebreak, played)
        if h.size > LEVERAGE_MAX_FIXTURES:
            raise ValueError(f"at most {LEVERAGE_MAX_FIXTURES} fixtures")
        names, masks = leverage_targets(targets, table_idx.size)
        levels = check_levels(levels)
        slot = np.full(len(self.teams), -1, dtype=np.int64)
        slot[table_idx.astype(np.int64)] = np.arange(table_idx.size)
        points_min, n_bins = points_axis(table[:, 0], slot[h], slot[a], points)
        if n_bins > POINTS_MAX_BINS:
            raise ValueError(f"the points axis would have {n_bins} bins ({points_min}..{points_min + n_bins - 1} "
                             f"points); at most {POINTS_MAX_BINS}")
        seed = _wall_clock_seed() if random_state is None else random_state
        extra = {"pair_init": pair, "head_to_head": True} if head_to_head else {}
        out = {"teams": np.asarray(self.teams)[table_idx], "targets": np.asarray(names)}
        if live:
            nf = h.size - ip[0].size
            raw = self._device().season_points_live(h[:nf], a[:nf], table_idx, table, points, n_sims, prng_key(seed),
                                                    masks, points_min, n_bins, in_play=ip, reweight=bool(reweight),
                                                    log_weights=lw, **extra)
            out.update(ess=float(raw["ess"]), log_evidence=float(raw["log_evidence"]))
        else:
            raw = self._device().season_points(h, a, table_idx, table, points, n_sims, prng_key(seed), masks,
                                               points_min, n_bins, **extra)
        out.update(points_from_counts(raw["team_points"], raw["team_target"], raw["position_points"], raw["gap"],
                                      points_min, n_sims, levels))
        return out

    def match_scenarios(self, home_team: TeamArg, away_team: TeamArg, fixtures, num_simulations: int = 10_000,
                        random_state: int = None, current_table: Optional[Dict] = None,
                        teams: Optional[TeamArg] = None, points: Tuple[int, int, int] = (3, 1, 0),
                        targets: Optional[Dict] = None, tiebreak: str = "overall", played: Optional[Dict] = None,
                        margin_cap=1, in_play: Optional[Dict] = None, reweight: bool = True,
                        log_weights=None) -> Dict[str, np.ndarray]:
        """The joint result of a few chosen fixtures against every team's finishing targets: "we stay up if we win,
        or if we draw and they lose by two", over `simulate_season`'s simulations (no reference counterpart).

        Every argument other than `fixtures` and `margin_cap` is `match_leverage`'s, under its rules, defaults and
        errors (1..8 targets, at most 4096 fixtures), and under the same `random_state` simulation j here IS
        simulation j of `simulate_season`, `match_leverage`, `points_needed` and `season_trajectory` (the same draw,
        scorelines, tie-break and ranking, in both tie-break modes); the counting happens on the device
        (csrc/dc_scenario.hip.h) and no per-simulation array comes back.  `fixtures` names the key fixtures as
        positions in the fixture list: 1..8 distinct integers in 0..F - 1 (bools, non-integers, duplicates,
        out-of-range values and an empty list raise ValueError).  `margin_cap` is an integer c in 1..3, or one per key
        fixture: a key fixture with cap c has C = 2 c + 1 classes, class j holding the simulations whose clipped
        margin clip(home goals - away goals, -c, c) equals c - j -- class 0 is "home by c or more", class 2 c "away
        by c or more", and with c = 1 the classes are `match_leverage`'s outcomes 0 home win, 1 draw, 2 away win.  A
        scenario is one class per key fixture, indexed row-major in the order given (m = sum_q class_q prod_{r > q}
        C_r), so every array with a leading M reshapes to (*shape, ...); M = prod C_q above 6561 raises ValueError.

        Returns numpy arrays (n table rows, K targets, k key fixtures, M scenarios, N simulations): "teams" [n];
        "targets" [K]; "fixtures" int64 [k] with their "home" and "away" names [k]; "margin_cap" int64 [k]; "shape"
        (the tuple of the C_q); "margins" int64 [M, k] (the clipped margin of every key fixture in scenario m, where
        +-c reads "by c or more"); the integer tables from the device, int64: "scenario_count" [M] and "joint_count"
        [M, n, K] (scenario m occurred AND team t finished inside target k); and from those integers
        "scenario_proba"; "target_count" [n, K] = joint_count.sum(0) (`match_leverage`'s) and "target_proba";
        "conditional_proba" [M, n, K] = joint_count / scenario_count and its binomial "conditional_se", both NaN
        exactly where the scenario never occurred; "settled" int8 [M, n, K]: +1 where the scenario occurred and the
        team was inside in every one of its simulations, -1 where it occurred and the team never was, 0 otherwise;
        "leverage" [n, K] = sum_m scenario_proba |conditional_proba - target_proba| over the scenarios that
        occurred: `match_leverage`'s measure for the k fixtures jointly.  `bpl.scenarios` has `marginal`, `coarsen`,
        `requirements` and `format_table` for a result.

        "settled" is about the SIMULATED seasons, not mathematical certainty: +1 says that none of the N simulations
        in which the scenario occurred left the team outside, which a rare chain of other results still could.  The
        conditional is the posterior-predictive one, as in `match_leverage`: a result also says something about how
        strong the two teams are.

        `in_play`, `reweight` and `log_weights` (defaults None, True, None: nothing changes, the same entry point,
        kernels, results and keys) are `match_leverage`'s, which are `simulate_season`'s: the question asked at 1-0
        after an hour, with the key fixtures themselves IN PROGRESS (csrc/dc_live_queries.hip.h).  The fixture list
        becomes the F positional fixtures followed by the L matches in play, and `fixtures` indexes that concatenated
        list: F + m names match m in play (values from F + L on raise ValueError), "home" and "away" come from it.  A
        key in play is classed by its FINAL clipped margin, so a class the current score has already ruled out simply
        has `scenario_count` 0 and NaN conditionals, as any scenario that never occurred; `bpl.scenarios`' helpers
        take the result unchanged.  Simulation j is simulation j of `simulate_season` and `match_leverage` under the
        same live arguments, and the result gains "ess" and "log_evidence", as there.

        Not modelled: `playoffs`; more than 8 key fixtures, or margins beyond +-3; scenario classes other than the
        clipped margin; `in_play` and `log_weights` in `season_trajectory`, `simulate_season(playoffs=...)`, the
        tournament family and the neutral and dynamic classes."""
        live = in_play is not None or log_weights is not None or not reweight
        if live:
            ip, lw, home_team, away_team = self._live_inputs(home_team, away_team, in_play, log_weights)
        h, a, table_idx, table, points, n_sims, head_to_head, pair = self._season_h2h_inputs(
            home_team, away_team, num_simulations, current_table, teams, points, tiebreak, played)
        if h.size > LEVERAGE_MAX_FIXTURES:
            raise ValueError(f"at most {LEVERAGE_MAX_FIXTURES} fixtures")
        names, masks = leverage_targets(targets, table_idx.size)
        keys, caps = _scenarios.check_keys(fixtures, margin_cap, h.size)
        seed = _wall_clock_seed() if random_state is None else random_state
        extra = {"pair_init": pair, "head_to_head": True} if head_to_head else {}
        team_names = np.asarray(self.teams)
        out = {"teams": team_names[table_idx], "targets": np.asarray(names), "fixtures": keys,
               "home": team_names[h[keys]], "away": team_names[a[keys]], "margin_cap": caps,
               "shape": _scenarios.scenario_shape(caps), "margins": _scenarios.scenario_margins(caps)}
        if live:
            nf = h.size - ip[0].size
            raw = self._device().season_scenarios_live(h[:nf], a[:nf], table_idx, table, points, n_sims, prng_key(seed),
                                                       masks, keys, caps, in_play=ip, reweight=bool(reweight),
                                                       log_weights=lw, **extra)
            out.update(ess=float(raw["ess"]), log_evidence=float(raw["log_evidence"]))
        else:
            raw = self._device().season_scenarios(h, a, table_idx, table, points, n_sims, prng_key(seed), masks, keys,
                                                  caps, **extra)
        out.update(_scenarios.scenario_from_counts(raw["scenario"], raw["joint"], n_sims))
        return out

    def season_trajectory(self, home_team: TeamArg, away_team: TeamArg, matchday, num_simulations: int = 10_000,
                          random_state: int = None, current_table: Optional[Dict] = None,
                          teams: Optional[TeamArg] = None, points: Tuple[int, int, int] = (3, 1, 0),
                          targets: Optional[Dict] = None, tiebreak: str = "overall",
                          played: Optional[Dict] = None) -> Dict[str, np.ndarray]:
        """The road to the final table: the table after EVERY remaining matchday, over `simulate_season`'s
        simulations -- who is top at Christmas and what that is worth, by which matchday a target is usually
        settled, how many matchdays a side spends in the bottom three, how often the lead changes hands (no
        reference counterpart).

        All arguments but `matchday` are `points_needed`'s, under its rules and defaults (1..8 targets, at most
        4096 fixtures).  `matchday` gives one integer label per fixture, any integers in any order; floats, bools,
        a wrong length and an empty fixture list raise ValueError.  The R distinct labels, sorted, are the
        matchdays, at most 256.  Under the same `random_state` simulation j here IS simulation j of
        `simulate_season`, `match_leverage` and `points_needed`: the same draw, the same scoreline for every fixture
        (a fixture keeps the random numbers of its place in the list, whatever its matchday) and the same tie-break
        word for a team at every matchday, in both tie-break modes.  The table after matchday r is the current table
        plus every fixture whose label is at most that matchday, ranked by exactly the rule of the final table:
        points (not points per game), and under "head_to_head" the mini-table over the matches booked so far,
        `played` included.  The table after the last matchday is `simulate_season`'s final table, position for
        position.  Everything is counted on the device (csrc/dc_trajectory.hip.h); no per-simulation array comes
        back.  The points axis runs from the least current total to the largest total anyone can end on; more than
        1024 values raise ValueError.

        Returns numpy arrays (n table rows, K targets, R matchdays, N simulations): "teams" [n]; "targets" [K];
        "matchdays" int64 [R]; the integer tables from the device, int64: "position_count" [R, n, n] (team t is in
        position p after matchday r), "target_count" [R, n, K] (inside target k after matchday r),
        "target_final_count" [R, n, K] (inside after matchday r AND at the end), "points_sum" and "points_sq_sum"
        [R, n] (the sums over the simulations of the points after matchday r and of their squares),
        "rounds_inside_count" [n, K, R + 1] (the number of matchdays after which the team was inside),
        "secured_count" [n, K, R + 1] (bin r < R: the earliest matchday from which the team is inside after that
        and every later matchday; bin R: not inside at the end), "lead_changes_count" [R] (the number of matchdays
        r >= 1 whose leader differs from the leader after matchday r - 1); and from those integers
        "position_proba" and "target_proba"; "final_given_inside" [R, n, K] = target_final_count / target_count
        and "final_given_outside" = (target_count[R - 1] - target_final_count) / (N - target_count), each with its
        binomial standard error ("..._se"), NaN where the denominator is 0; "points_mean" and "points_sd" [R, n]
        (the population form); "expected_rounds_inside" [n, K]; "secured_by_proba" [n, K, R] =
        cumsum(secured_count[..., :R]) / N, whose last column is target_proba[R - 1]; "expected_lead_changes".

        Limits: "secured" is hindsight over the simulated positions -- the matchday after which the team never left
        the target in that simulation -- not mathematical certainty; the current table before the first remaining
        matchday is not a row of the trajectory.  Not modelled: mathematical clinching, points per game for unequal
        games played, `in_play`, `log_weights`, `playoffs`, and the neutral and dynamic classes."""
        h, a, table_idx, table, points, n_sims, head_to_head, pair = self._season_h2h_inputs(
            home_team, away_team, num_simulations, current_table, teams, points, tiebreak, played)
        if h.size > LEVERAGE_MAX_FIXTURES:
            raise ValueError(f"at most {LEVERAGE_MAX_FIXTURES} fixtures")
        matchdays, fix_id, round_end = trajectory_rounds(matchday, h.size)
        names, masks = leverage_targets(targets, table_idx.size)
        slot = np.full(len(self.teams), -1, dtype=np.int64)
        slot[table_idx.astype(np.int64)] = np.arange(table_idx.size)
        points_min, n_bins = trajectory_axis(table[:, 0], slot[h], slot[a], points)
        if n_bins > POINTS_MAX_BINS:
            raise ValueError(f"the points axis would have {n_bins} bins ({points_min}..{points_min + n_bins - 1} "
                             f"points); at most {POINTS_MAX_BINS}")
        seed = _wall_clock_seed() if random_state is None else random_state
        extra = {"pair_init": pair, "head_to_head": True} if head_to_head else {}
        raw = self._device().season_trajectory(h, a, table_idx, table, points, n_sims, prng_key(seed), masks,
                                               points_min, n_bins, fix_id, round_end, **extra)
        out = {"teams": np.asarray(self.teams)[table_idx], "targets": np.asarray(names), "matchdays": matchdays}
        out.update(trajectory_from_counts(raw["position"], raw["target"], raw["target_final"], raw["points_sum"],
                                          raw["points_sq_sum"], raw["rounds_inside"], raw["secured"],
                                          raw["lead_changes"], points_min, n_sims))
        return out
