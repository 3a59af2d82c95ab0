"""The neutral-venue model with time-varying (per gameweek) parameters -- host-side
mirror of the reference's bpl/dynamic_dixon_coles.py:23-584
(`DynamicNeutralDixonColesMatchPredictor`), which is unfinished there: not exported from
bpl/__init__.py, untested, and its random walk is a no-op because the results of
`attack.at[j].set(...)` are discarded (:192-218).  `fit(random_walk=True)` (default) runs the
INTENDED model, attack[g] = attack[g-1] + standardised_attack[g]*std_attack[g];
`random_walk=False` runs the model as the reference code computes it.  Other defects of the
reference are not reproduced: num_gameweeks = max(gameweek)+1 (reference: max, :287), the
debug prints (:303-307) are dropped, `mean_away_attack` reads its own site (:324 reads
mean_home_attack), the predict side uses the signs of `_model` (:220-231) and takes the
gameweek to predict for (default: the last one).  `_model` + NUTS run in libbplhip.so.
Like the reference, the class is importable from this module, not from `bpl`."""

from __future__ import annotations

import warnings

from typing import Any, Dict, Iterable, Optional, Tuple, Union

import numpy as np

from bpl import diagnostics as _diagnostics
from bpl import elpd as _elpd
from bpl import inplay as _inplay
from bpl import markets as _markets
from bpl import periods as _periods
from bpl import ratings as _ratings
from bpl import ppc as _ppc
from bpl import loo_scores as _loo_scores
from bpl import scoring as _scoring
from bpl import sensitivity as _sensitivity
from bpl import sequential as _sequential
from bpl import slate as _slate
from bpl._mcmc import check_goals, concat_init, dynamic_sites, same_start, sample_chains, standardise_covariates
from bpl.base import MAX_GOALS, PosteriorOnDevice, outcome_from_grid, score_grid

__all__ = ["DynamicNeutralDixonColesMatchPredictor"]


def latent_sites(G: int, T: int, K: int):
    """(name, shape) in flat (sorted-name) order; D = 7GT + 10G + 2 + 2K."""
    s = []
    if K:
        s.append(("attack_coefficients", (K,)))
    s += [("away_attack_decentered", (G, T)), ("away_defence_decentered", (G, T)),
          ("corr_coef_raw", ())]
    if K:
        s.append(("defence_coefficients", (K,)))
    s += [("home_attack_decentered", (G, T)), ("home_defence_decentered", (G, T)),
          ("mean_away_attack", (G,)), ("mean_away_defence", (G,)), ("mean_defence", ()),
          ("mean_home_attack", (G,)), ("mean_home_defence", (G,)),
          ("standardised_attack", (G, T)), ("standardised_defence", (G, T)),
          ("std_attack", (G,)), ("std_away_attack", (G,)), ("std_away_defence", (G,)),
          ("std_defence", (G,)), ("std_home_attack", (G,)), ("std_home_defence", (G,)),
          ("u", (G, T))]
    return s


# pylint: disable=too-many-instance-attributes
class DynamicNeutralDixonColesMatchPredictor(PosteriorOnDevice, _elpd.PointwiseLikelihood,
                                             _ppc.PosteriorPredictiveCheck, _scoring.ForecastScores,
                                             _markets.PredictMarkets, _inplay.PredictInPlay,
                                             _periods.PredictPeriods, _sequential.SequentialScores,
                                             _diagnostics.McmcDiagnostics,
                                             _ratings.TeamRatings, _slate.PredictSlate, _loo_scores.LooScores,
                                             _sensitivity.PowerscaleSensitivity):
    """Dixon-Coles with neutral venues, separate home/away attack/defence offsets and a
    random walk of the team strengths over gameweeks."""

    def __init__(self):
        self.teams = None
        self.attack = None        # [S, G, T]
        self.defence = None       # [S, G, T]
        self.home_attack = None
        self.away_attack = None
        self.home_defence = None
        self.away_defence = None
        self.corr_coef = None
        self.u = None
        self.rho = None
        self.attack_coefficients = None
        self.defence_coefficients = None
        self.mean_defence = None
        self.std_defence = None
        self.std_attack = None
        self.mean_home_attack = None
        self.mean_away_attack = None
        self.mean_home_defence = None
        self.mean_away_defence = None
        self.std_home_attack = None
        self.std_away_attack = None
        self.std_home_defence = None
        self.std_away_defence = None
        self.standardised_attack = None
        self.standardised_defence = None
        self._team_covariates_mean = None
        self._team_covariates_std = None
        self.num_gameweeks = None
        self.mcmc_info_ = None

    # pylint: disable=too-many-arguments,too-many-locals
    def fit(
        self,
        training_data: Dict[str, Union[Iterable[str], Iterable[float]]],
        random_state: int = 42,
        num_warmup: int = 500,
        num_samples: int = 1000,
        mcmc_kwargs: Optional[Dict[str, Any]] = None,
        run_kwargs: Optional[Dict[str, Any]] = None,
        random_walk: bool = True,
    ) -> "DynamicNeutralDixonColesMatchPredictor":
        """Fit the model.  training_data keys: home_team, away_team, home_goals,
        away_goals, gameweek (0-based ints), neutral_venue (0/1), optional team_covariates.

        random_walk=True (default) fits the INTENDED model, attack[g] = attack[g-1] + increment;
        the reference's code discards those updates (bpl/dynamic_dixon_coles.py:192-218 assign
        `attack.at[j].set(...)` to nothing), so its posterior is that of random_walk=False.  A
        warning says so once per fit; pass random_walk=False for the reference's behaviour."""
        if random_walk:
            warnings.warn(
                "DynamicNeutralDixonColesMatchPredictor.fit(random_walk=True) fits the intended "
                "random-walk model; the upstream implementation discards the walk (its attack and "
                "defence stay at zero). Results differ from upstream: pass random_walk=False to "
                "reproduce it.", stacklevel=2)

        home_team = list(training_data["home_team"])
        away_team = list(training_data["away_team"])
        self.teams = sorted(list(set(home_team) | set(away_team)))
        tidx = {t: i for i, t in enumerate(self.teams)}
        home_ind = np.array([tidx[t] for t in home_team], dtype=np.uint16)
        away_ind = np.array([tidx[t] for t in away_team], dtype=np.uint16)
        T = len(self.teams)

        cov_std, mean, std = standardise_covariates(training_data.get("team_covariates"), self.teams)
        if cov_std is not None:
            self._team_covariates_mean, self._team_covariates_std = mean, std
        K = 0 if cov_std is None else cov_std.shape[1]

        gameweek = np.array(training_data["gameweek"], dtype=int)
        if gameweek.min() < 0:
            raise ValueError("gameweek must be >= 0")
        G = int(gameweek.max()) + 1
        self.num_gameweeks = G
        hg, ag = check_goals(training_data["home_goals"], training_data["away_goals"])
        nv = np.asarray(training_data["neutral_venue"]).astype(np.uint8)
        sites = latent_sites(G, T, K)
        # (no keyword of mcmc_kwargs / run_kwargs is checked here, and every chain starts from the one
        # init_params point: DESIGN.md section 5, known gaps)
        mcmc_kwargs = dict(mcmc_kwargs or {})
        z0 = concat_init(dict(run_kwargs or {}).get("init_params"), sites)

        def bind(ctx):
            ctx.set_fixtures_dynamic(home_ind, away_ind, hg, ag, gameweek, nv, T, G,
                                     covariates_std=cov_std, random_walk=random_walk)

        z, self.mcmc_info_, tables = sample_chains(
            bind, num_chains=int(mcmc_kwargs.get("num_chains", 1)), thinning=int(mcmc_kwargs.get("thinning", 1)),
            random_state=random_state, num_warmup=num_warmup, num_samples=num_samples,
            init=None if z0 is None else lambda num_chains, D: same_start(z0, num_chains),
            finish=lambda ctx, z: ctx.constrain_dynamic(z), lockstep=False)
        for nm in self._VENUE_TABLES:
            setattr(self, nm, tables[nm])
        self.corr_coef = self.mcmc_info_["corr_coef"]  # a sampler statistic: aux[0] at the accepted proposal
        for nm, v in dynamic_sites(sites, z).items():
            setattr(self, nm, v)
        return self

    # ---- predict side: the tables of ONE gameweek through the venue-aware device kernels
    # (csrc/dc_predict.hip.h, the same entry points the neutral-venue classes use)
    _VENUE_TABLES = ("attack", "defence", "home_attack", "away_attack", "home_defence", "away_defence")
    _predict_gameweek = None   # the gameweek whose tables the device holds (part of the upload stamp, a plain int)

    # mcmc_diagnostics (bpl/diagnostics.py): the per-gameweek tables and every other posterior array kept after a fit
    _DIAGNOSTIC_SITES = _VENUE_TABLES + (
        "corr_coef", "attack_coefficients", "defence_coefficients", "rho", "mean_defence", "std_attack", "std_defence",
        "mean_home_attack", "mean_away_attack", "mean_home_defence", "mean_away_defence", "std_home_attack",
        "std_away_attack", "std_home_defence", "std_away_defence")

    def _latent_sites(self):
        K = 0 if self.attack_coefficients is None else np.shape(self.attack_coefficients)[1]
        return latent_sites(self.num_gameweeks, len(self.teams), K)

    def _posterior_arrays(self):
        g = self._predict_gameweek
        return tuple(getattr(self, nm)[:, g, :] for nm in self._VENUE_TABLES) + (self.corr_coef, int(g))

    def _upload_posterior(self, ctx):
        g = self._predict_gameweek
        ctx.predict_set_posterior_venue(*(getattr(self, nm)[:, g, :] for nm in self._VENUE_TABLES), self.corr_coef)

    def __getstate__(self):
        state = super().__getstate__()
        state.pop("_predict_gameweek", None)   # (a cache key of the device side, not model state)
        return state

    def _week(self, gameweek: Optional[int]) -> int:
        g = self.num_gameweeks - 1 if gameweek is None else int(gameweek)
        if not 0 <= g < self.num_gameweeks:
            raise IndexError(f"gameweek {g} outside 0..{self.num_gameweeks - 1}")
        return g

    def _week_device(self, week: int):
        self._predict_gameweek = week
        return self._device()

    _ratings_venue_model = True

    # pylint: disable=arguments-differ,too-many-arguments
    def team_ratings(self, teams=None, opponents=None, venue: Optional[str] = None, max_goals: int = 15,
                     points=(3, 1, 0), rank_by: str = "points", quantiles=(0.05, 0.5, 0.95),
                     return_draws: bool = False, gameweek=None) -> Dict:
        """`TeamRatings.team_ratings` on the tables of `gameweek`: None (the last gameweek), an int or a sequence
        of ints, a rating trajectory.  Every array that depends on the posterior gains a leading axis of length
        W, the number of gameweeks asked for (1 for None or an int), and "gameweeks" [W] names them; one device
        call per gameweek on that week's tables, so several gameweeks give the stack of the single calls."""
        try:
            weeks = [gameweek] if gameweek is None or isinstance(gameweek, (int, np.integer)) else list(gameweek)
            if not weeks or any(isinstance(g, (bool, np.bool_)) or not isinstance(g, (int, np.integer, type(None)))
                                for g in weeks):
                raise IndexError("gameweek must be None, an int or a non-empty sequence of ints")
            weeks = [self._week(g) for g in weeks]
        except (IndexError, TypeError) as e:
            raise ValueError(str(e)) from e
        return self._team_ratings(teams, opponents, venue, max_goals, points, rank_by, quantiles, return_draws,
                                  weeks=weeks)

    def _fixture_groups(self, data, with_goals: bool):
        """log_likelihood / waic / loo (bpl/elpd.py; with the goals) and predict_markets (without): one
        device call per gameweek of `data` on that week's tables, results scattered back into fixture order."""
        n = _elpd.fixture_count(data, ("home_team", "away_team") + (("home_goals", "away_goals") if with_goals else ())
                                + ("neutral_venue", "gameweek"))
        teams = {t: i for i, t in enumerate(self.teams)}
        h = _elpd.lookup(data["home_team"], teams, n)
        a = _elpd.lookup(data["away_team"], teams, n)
        if with_goals:
            x, y = _elpd.goals(data["home_goals"], n), _elpd.goals(data["away_goals"], n)
        nv = _elpd.venue(data["neutral_venue"], n)
        gw = np.asarray(list(data["gameweek"]))
        if n and (gw.dtype.kind not in "iu"):
            raise ValueError("gameweek must be integers")
        groups = []
        for g in np.unique(gw):
            week = self._week(int(g))
            pos = np.nonzero(gw == g)[0]
            kwargs = {"home_idx": h[pos], "away_idx": a[pos], "neutral": nv[pos]}
            if with_goals:
                kwargs.update(home_goals=x[pos], away_goals=y[pos])
            groups.append((pos, lambda week=week: self._week_device(week), kwargs))
        return groups, n

    def _fixture_indices(self, home_team, away_team):
        home_team = [home_team] if isinstance(home_team, str) else list(home_team)
        away_team = [away_team] if isinstance(away_team, str) else list(away_team)
        return (np.array([self.teams.index(t) for t in home_team], dtype=np.uint16),
                np.array([self.teams.index(t) for t in away_team], dtype=np.uint16))

    def _calculate_expected_goals(self, home_team, away_team, neutral_venue,
                                  gameweek: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        g = self._week(gameweek)
        h, a = self._fixture_indices(home_team, away_team)
        at_home = 1.0 - np.asarray(neutral_venue, dtype=np.float64)
        # signs as in `_model` (bpl/dynamic_dixon_coles.py:220-231)
        log_home = (self.attack[:, g, h] - self.defence[:, g, a]
                    + at_home * self.home_attack[:, g, h] - at_home * self.away_defence[:, g, a])
        log_away = (self.attack[:, g, a] - self.defence[:, g, h]
                    + at_home * self.away_attack[:, g, a] - at_home * self.home_defence[:, g, h])
        return np.exp(log_home), np.exp(log_away)

    def predict_score_proba(self, home_team, away_team, home_goals, away_goals, neutral_venue,
                            gameweek: Optional[int] = None) -> np.ndarray:
        """Probabilities of the given scorelines (mean over posterior draws)."""
        self._predict_gameweek = self._week(gameweek)
        h, a = self._fixture_indices(home_team, away_team)
        m = max(len(h), np.size(home_goals), np.size(away_goals))
        spread = lambda v: np.broadcast_to(np.asarray(v), (m,))
        return self._device().predict_score_proba(spread(h), spread(a), spread(home_goals), spread(away_goals),
                                                  neutral=spread(neutral_venue))

    def predict_outcome_proba(self, home_team, away_team, neutral_venue,
                              gameweek: Optional[int] = None) -> Dict[str, np.ndarray]:
        """Home win, draw and away win probabilities: the triangles of each fixture's scoreline grid."""
        self._predict_gameweek = self._week(gameweek)
        h, a = self._fixture_indices(home_team, away_team)
        return outcome_from_grid(score_grid(self._device, h, a, MAX_GOALS, neutral=neutral_venue))
