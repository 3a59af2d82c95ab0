"""The hand-built configurations the live-season tests share (tests/test_live_host.py without a GPU,
tests/test_gpu_live.py on one): the posteriors of tests/test_gpu_season.py cut to six teams, nine fixtures still to
kick off, the states of the matches in progress, and the numpy restatement (tests/live_ref.py) of each
configuration, computed once per process."""
import functools

import numpy as np

import live_ref as LR
from bpl.base import _prng_key
from test_gpu_season import _posterior

KINDS = ("basic", "extended", "rho_bounds", "clipped")
T, S, N, SEED = 6, 257, 4096, 20260
# (home goals, away goals, elapsed) of the matches in progress
STATES = ((0, 0, 0.0), (1, 0, 0.3), (0, 1, 0.5), (1, 1, 0.7), (2, 1, 0.9), (0, 3, 0.999))
LIVE_PAIRS = ((0, 1), (2, 3), (4, 5), (1, 0), (3, 2), (5, 4))
FIXTURES = ((0, 2), (1, 3), (2, 4), (3, 5), (4, 0), (5, 1), (0, 3), (1, 4), (2, 5))   # F = 9
TABLE = {"t00": (31, 30, 22), "t02": (31, 28, 20), "t03": (28, 25, 25), "t05": (12, 9, 30)}


def posterior(kind):
    return _posterior(kind, T=T, S=S, seed=4)


def names(m, idx):
    return [str(m.teams[i]) for i in idx]


def in_play(m, states=STATES, pairs=LIVE_PAIRS):
    """The `in_play` dict of `states` on the first len(states) of `pairs`."""
    n = len(states)
    return {"home_team": names(m, [p[0] for p in pairs[:n]]), "away_team": names(m, [p[1] for p in pairs[:n]]),
            "home_goals": [s[0] for s in states], "away_goals": [s[1] for s in states],
            "elapsed": [s[2] for s in states]}


def fixtures(m, pairs=FIXTURES):
    return names(m, [p[0] for p in pairs]), names(m, [p[1] for p in pairs])


def random_log_weights(seed=8):
    return np.random.RandomState(seed).normal(0.0, 1.5, S)


def reference(m, home, away, ip, n_sims, seed, current_table=None, reweight=True, log_weights=None, tiebreak="overall"):
    """tests/live_ref.py on the arguments `m.simulate_season` takes (names resolved by the model's own host code)."""
    ipr = m._in_play_inputs(ip)
    hh = np.concatenate([m._team_indices(home), ipr[0]])
    aa = np.concatenate([m._team_indices(away), ipr[1]])
    h, a, table_idx, table, points, n, h2h, pair = m._season_h2h_inputs(hh, aa, n_sims, current_table, None, (3, 1, 0),
                                                                        tiebreak, None)
    F = h.size - ipr[0].size
    return LR.simulate_season_live(m.attack, m.defence, m.home_advantage, m.corr_coef, h[:F], a[:F], ipr, table_idx,
                                   table, points, n, _prng_key(seed), reweight, log_weights, h2h, pair)


@functools.lru_cache(maxsize=None)
def restatement(kind, with_log_weights, tiebreak):
    """(model, reference) of the restatement configuration: S = 257, N = 4096, T = 6, F = 9, the six STATES."""
    m = posterior(kind)
    home, away = fixtures(m)
    lw = random_log_weights() if with_log_weights else None
    return m, reference(m, home, away, in_play(m), N, SEED, TABLE, True, lw, tiebreak)
