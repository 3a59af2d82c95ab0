"""Neutral-venue Dixon-Coles model (host side), SURVEY.md §8 row f-4.

Mirrors the reference's bpl/neutral_dixon_coles.py:30-902 (`NeutralDixonColesMatchPredictor`)
method for method: same names, arguments, return shapes and error behaviour; arrays are
numpy instead of jax.  `fit` drives libbplhip (bplhip_set_fixtures_neutral + bplhip_nuts_run);
the predict methods run on the device like the league models' (bpl/base.py here): ONE primitive,
the per-fixture scoreline grid of `bplhip_predict_score_grid` in its venue form (csrc/dc_predict.hip.h, the
venue-aware rate form), of which outcomes, n-goal marginals and the sampling methods are
reductions; arbitrary scorelines go through the pointwise kernel.  No host fallback.
"""

from __future__ import annotations

import warnings
from typing import Any, Dict, Iterable, Optional, Tuple, Union

import numpy as np

from bpl import allocation as _allocation
from bpl import diagnostics as _diagnostics
from bpl import elpd as _elpd
from bpl import group_points as _group_points
from bpl import inplay as _inplay
from bpl import markets as _markets
from bpl import periods as _periods
from bpl import ratings as _ratings
from bpl import ppc as _ppc
from bpl import loo_scores as _loo_scores
from bpl import paths as _paths
from bpl import scenarios as _scenarios
from bpl import scoring as _scoring
from bpl import sensitivity as _sensitivity
from bpl import sequential as _sequential
from bpl import slate as _slate
from bpl._ffi import prng_key
from bpl._mcmc import (chain_kwargs, check_goals, concat_init, neutral_sites, same_start, sample_chains,
                       standardise_covariates)
from bpl._util import check_points, check_simulations, parse_teams, str_to_list
from bpl.base import (DTYPES, LEVERAGE_MAX_FIXTURES, LIVE_MAX_GOALS, MAX_GOALS, SEASON_MAX_FIXTURES,
                      SEASON_MAX_TABLE_VALUE, PosteriorOnDevice, _wall_clock_seed, check_levels, check_tiebreak,
                      draw_scores, draw_winners, goal_marginal, goals_wanted, leverage_from_counts, outcome_from_grid,
                      pair_records, played_matches, points_axis, remaining_meetings, score_grid, table_from_played)

__all__ = ["NeutralDixonColesMatchPredictor"]

# simulate_tournament's bounds (include/bplhip.h BPLHIP_TOURNAMENT_*, csrc/dc_tournament.hip.h)
TOURNAMENT_MAX_TEAMS = 64
TOURNAMENT_MAX_GROUPS = 16
TOURNAMENT_MAX_GROUP_SIZE = 8
TOURNAMENT_MAX_ROUNDS = 6
TOURNAMENT_MAX_STRENGTH = 20.0          # |shoot-out strength| (BPLHIP_TOURNAMENT_MAX_STRENGTH)
KNOCKOUT_RULES = ("redraw", "extra_time")
EXTRA_TIME_SCALE = 1 / 3                # extra time's 30 minutes of the 90


def latent_sites(T: int, K: int, C: int = 0):
    """(name, size) of every latent site in flat (sorted-name) order; D = 6T + 2K + C + 13
    (C confederations: World-Cup variant)."""
    s = []
    if K:
        s.append(("attack_coefficients", K))
    s += [("away_attack_decentered", T), ("away_defence_decentered", T)]
    if C:
        s.append(("confederation_strength_decentered", C))
    s.append(("corr_coef_raw", 1))
    if K:
        s.append(("defence_coefficients", K))
    s += [("home_attack_decentered", T), ("home_defence_decentered", T),
          ("mean_away_attack", 1), ("mean_away_defence", 1), ("mean_defence", 1),
          ("mean_home_attack", 1), ("mean_home_defence", 1),
          ("standardised_attack", T), ("standardised_defence", T),
          ("std_attack", 1), ("std_away_attack", 1), ("std_away_defence", 1),
          ("std_defence", 1), ("std_home_attack", 1), ("std_home_defence", 1), ("u", 1)]
    return s


def make_weights(n, time_diff, epsilon, game_weights, rescale_weights):
    """bpl/neutral_dixon_coles.py:251-257 (parameter independent, so computed once)."""
    w = np.ones(n)
    if epsilon is not None:
        w = w * np.exp(-epsilon * np.asarray(time_diff, dtype=np.float64))
        if rescale_weights:
            w = n * w / w.sum()
    if game_weights is None:
        # the reference multiplies by `game_weights` unconditionally (:256-257)
        raise TypeError("unsupported operand type(s) for *: 'Array' and 'NoneType' "
                        "(training_data['game_weights'] is required)")
    return w * np.asarray(game_weights, dtype=np.float64)


# pylint: disable=too-many-instance-attributes
class NeutralDixonColesMatchPredictor(PosteriorOnDevice, _elpd.PointwiseLikelihood, _ppc.PosteriorPredictiveCheck,
                                      _scoring.ForecastScores, _markets.PredictMarkets, _inplay.PredictInPlay,
                                      _periods.PredictPeriods, _sequential.SequentialScores, _diagnostics.McmcDiagnostics,
                                      _ratings.TeamRatings, _slate.PredictSlate, _loo_scores.LooScores,
                                      _sensitivity.PowerscaleSensitivity):
    """Dixon-Coles with rho-correlated attack/defence, optional covariates, separate home and
    away attack/defence offsets per team that vanish at neutral venues, time decay and
    per-game weights (see bpl/neutral_dixon_coles.py:30-52)."""

    def __init__(self):
        self.teams = None
        self._teams_dict = None
        for nm in ("attack", "defence", "home_attack", "away_attack", "home_defence", "away_defence",
                   "time_diff", "epsilon", "rescale_weights", "game_weights", "corr_coef", "u", "rho",
                   "attack_coefficients", "defence_coefficients", "mean_attack", "mean_defence",
                   "std_attack", "std_defence", "mean_home_attack", "mean_away_attack",
                   "mean_home_defence", "mean_away_defence", "std_home_attack", "std_away_attack",
                   "std_home_defence", "std_away_defence", "standardised_attack",
                   "standardised_defence", "_team_covariates_mean", "_team_covariates_std",
                   "confederation_strength"):
            setattr(self, nm, None)
        self.mcmc_info_ = None

    # pylint: disable=arguments-differ,too-many-arguments,too-many-statements,too-many-locals
    def fit(
        self,
        training_data: Dict[str, Union[Iterable[str], Iterable[float]]],
        epsilon: Optional[float] = None,
        rescale_weights: Optional[bool] = False,
        random_state: int = 42,
        num_warmup: int = 500,
        num_samples: int = 1000,
        mcmc_kwargs: Optional[Dict[str, Any]] = None,
        run_kwargs: Optional[Dict[str, Any]] = None,
    ) -> "NeutralDixonColesMatchPredictor":
        """Fit model to data (bpl/neutral_dixon_coles.py:286-384)."""
        self.epsilon = epsilon
        self.rescale_weights = rescale_weights
        self.time_diff = training_data.get("time_diff", None)
        if epsilon is not None and self.time_diff is None:
            raise ValueError(
                """
                    time_diff must be provided in training_data
                    to include exponential time decay in model.
                    """
            )
        self.game_weights = training_data.get("game_weights", None)
        n = len(list(training_data["home_goals"]))
        weights = make_weights(n, self.time_diff, epsilon, self.game_weights, rescale_weights)
        return self._fit(training_data, weights, None, random_state, num_warmup, num_samples,
                         mcmc_kwargs, run_kwargs)

    def _fit(self, training_data, weights, conf, random_state, num_warmup, num_samples,
             mcmc_kwargs, run_kwargs):
        """Shared by the neutral and the World-Cup model.  `conf`: None or
        (home_conf_idx, away_conf_idx, n_conf)."""
        self.teams, self._teams_dict, home_ind, away_ind = parse_teams(
            training_data["home_team"], training_data["away_team"], DTYPES["teams"]
        )
        T = len(self.teams)
        cov_std, mean, std = standardise_covariates(training_data.get("team_covariates"), self.teams)
        if cov_std is not None:
            self._team_covariates_mean, self._team_covariates_std = mean, std
        K = 0 if cov_std is None else cov_std.shape[1]
        C = 0 if conf is None else int(conf[2])
        hg, ag = check_goals(training_data["home_goals"], training_data["away_goals"])
        nv = np.asarray(training_data["neutral_venue"]).astype(np.uint8)
        _, run_kwargs, chains = chain_kwargs(mcmc_kwargs, run_kwargs)  # (postprocess_fn, extra_fields: ignored)
        sites = latent_sites(T, K, C)

        def bind(ctx):
            ctx.set_fixtures_neutral(home_ind, away_ind, hg, ag, nv, T, weights=weights, covariates_std=cov_std,
                                     home_conf=None if conf is None else conf[0],
                                     away_conf=None if conf is None else conf[1], n_conf=C)

        def init(num_chains, D):  # one point for every chain ([D]) or one per chain ([num_chains, D])
            z0 = concat_init(run_kwargs.get("init_params"), sites)
            if z0 is None:
                return None
            z0 = np.asarray(z0, np.float64)
            if z0.size == D:
                return same_start(z0.reshape(D), num_chains)
            if z0.size == num_chains * D:
                return z0.reshape(num_chains, D)
            raise ValueError(f"init_params must have {D} or {num_chains}x{D} entries, got {z0.size}")

        z, self.mcmc_info_, _ = sample_chains(bind, random_state=random_state, num_warmup=num_warmup,
                                              num_samples=num_samples, init=init, **chains)
        for nm, v in neutral_sites(sites, z, cov_std, C).items():
            if nm != "confederation_strength" or C:
                setattr(self, nm, v)
        self.corr_coef = self.mcmc_info_["corr_coef"]  # a sampler statistic: aux[0] at the accepted proposal
        return self

    # mcmc_diagnostics (bpl/diagnostics.py): every posterior array kept after a fit
    _DIAGNOSTIC_SITES = ("attack", "defence", "home_attack", "away_attack", "home_defence", "away_defence", "corr_coef",
                         "confederation_strength", "attack_coefficients", "defence_coefficients", "rho", "mean_defence",
                         "std_attack", "std_defence", "mean_home_attack", "mean_away_attack", "mean_home_defence",
                         "mean_away_defence", "std_home_attack", "std_away_attack", "std_home_defence",
                         "std_away_defence")

    def _latent_sites(self):
        K = 0 if self.attack_coefficients is None else np.shape(self.attack_coefficients)[1]
        C = 0 if self.confederation_strength is None else np.shape(self.confederation_strength)[1]
        return latent_sites(len(self.teams), K, C)

    def _fit_weights(self, data):
        """prior_sensitivity (bpl/sensitivity.py): `fit`'s weights on the fixtures of `data`, from its time_diff and
        game_weights columns and the fit's own epsilon and rescale_weights."""
        n = len(list(data["home_goals"]))
        return make_weights(n, data.get("time_diff", None), self.epsilon, data.get("game_weights", None),
                            self.rescale_weights)

    def _parse_fixture_args(self, home_team, away_team, neutral_venue):
        home_team, away_team = str_to_list(home_team, away_team)
        neutral_venue = np.array(neutral_venue, DTYPES["venue"])
        if isinstance(home_team[0], str):
            home_team = np.array([self._teams_dict[t] for t in home_team], DTYPES["teams"])
        if isinstance(away_team[0], str):
            away_team = np.array([self._teams_dict[t] for t in away_team], DTYPES["teams"])
        return np.asarray(home_team), np.asarray(away_team), neutral_venue

    # ---- internals on index arrays; `conf` = None or (home_conf_idx, away_conf_idx)
    _VENUE_TABLES = ("attack", "defence", "home_attack", "away_attack", "home_defence", "away_defence")

    def _posterior_arrays(self):
        return tuple(getattr(self, nm) for nm in self._VENUE_TABLES) + (self.corr_coef, self.confederation_strength)

    def _upload_posterior(self, ctx):
        ctx.predict_set_posterior_venue(*(getattr(self, nm) for nm in self._VENUE_TABLES), self.corr_coef,
                                        confederation_strength=self.confederation_strength)

    # log_likelihood / waic / loo (bpl/elpd.py): the per-fixture keys `fit` reads, checked on the host
    _LOGLIK_KEYS = ("home_team", "away_team", "home_goals", "away_goals", "neutral_venue")

    def _loglik_conf(self, data, n):
        """Confederation indices of the fixtures (None: the plain class has none)."""
        return None

    def _fixture_groups(self, data, with_goals: bool):
        n = _elpd.fixture_count(data, tuple(k for k in self._LOGLIK_KEYS if with_goals or not k.endswith("_goals")))
        kwargs = {"home_idx": _elpd.lookup(data["home_team"], self._teams_dict, n),
                  "away_idx": _elpd.lookup(data["away_team"], self._teams_dict, n)}
        if with_goals:
            kwargs.update(home_goals=_elpd.goals(data["home_goals"], n), away_goals=_elpd.goals(data["away_goals"], n))
        kwargs.update(neutral=_elpd.venue(data["neutral_venue"], n), conf=self._loglik_conf(data, n))
        return [(None, self._device, kwargs)], n

    def _rates(self, home_team, away_team, neutral_venue, conf=None):
        """Scoring rates [draws, fixtures]: the venue offsets count only away from neutral ground."""
        at_home = 1.0 - np.asarray(neutral_venue, dtype=np.float64)
        log_home = (self.attack[:, home_team] - self.defence[:, away_team]
                    + at_home * self.home_attack[:, home_team] - at_home * self.away_defence[:, away_team])
        log_away = (self.attack[:, away_team] - self.defence[:, home_team]
                    + at_home * self.away_attack[:, away_team] - at_home * self.home_defence[:, home_team])
        if conf is not None:
            edge = self.confederation_strength[:, conf[0]] - self.confederation_strength[:, conf[1]]
            log_home, log_away = log_home + edge, log_away - edge
        return np.exp(log_home), np.exp(log_away)

    def _score_proba(self, home_team, away_team, home_goals, away_goals, neutral_venue, conf=None):
        """Posterior-mean probability of each (fixture, scoreline) query: the pointwise kernel."""
        home_team, away_team = np.atleast_1d(home_team), np.atleast_1d(away_team)
        m = max(len(home_team), np.size(home_goals), np.size(away_goals))
        spread = lambda v: np.broadcast_to(np.asarray(v), (m,))
        return self._device().predict_score_proba(
            spread(home_team), spread(away_team), spread(home_goals), spread(away_goals),
            neutral=spread(neutral_venue), conf=None if conf is None else (spread(conf[0]), spread(conf[1])))

    def _grid_probs(self, home_team, away_team, neutral_venue, conf, max_goals) -> np.ndarray:
        """[fixtures, max_goals+1, max_goals+1]: P(home scores x, away scores y)."""
        return score_grid(self._device, home_team, away_team, max_goals, neutral=neutral_venue, conf=conf)

    def _grid(self, home_team, away_team, neutral_venue, conf, max_goals):
        counts = np.arange(max_goals + 1)
        return (self._grid_probs(home_team, away_team, neutral_venue, conf, max_goals),
                *np.meshgrid(counts, counts, indexing="ij"))

    def _outcome(self, home_team, away_team, neutral_venue, conf, knockout, max_goals):
        return outcome_from_grid(self._grid_probs(home_team, away_team, neutral_venue, conf, max_goals), knockout)

    def _sample_score(self, home_team, away_team, neutral_venue, conf, num_samples, random_state,
                      max_goals):
        return draw_scores(self._grid_probs(home_team, away_team, neutral_venue, conf, max_goals), max_goals,
                           num_samples, random_state)

    def _sample_outcome(self, home_team, away_team, neutral_venue, conf, knockout, num_samples,
                        random_state, max_goals):
        return draw_winners(self._outcome(home_team, away_team, neutral_venue, conf, knockout, max_goals),
                            home_team, away_team, self.teams, num_samples, random_state)

    def _n_proba(self, n, team, opponent, conf, home, neutral_venue, max_goals, scored: bool):
        """P(`team` scores [concedes] n), the other side's goals summed over 0..max_goals (the reference
        sums predict_score_proba over the same cells, bpl/neutral_dixon_coles.py:782-902)."""
        wanted = goals_wanted(n)
        depth = max(int(max_goals), int(wanted.max()))
        nv = np.atleast_1d(np.asarray(neutral_venue))[:1]
        if home:
            grid = self._grid_probs(team[:1], opponent[:1], nv, conf, depth)[0]
        else:
            grid = self._grid_probs(opponent[:1], team[:1], nv, None if conf is None else (conf[1], conf[0]), depth)[0]
        # axis 0 counts the home side's goals: the team's when it is at home and we count its own
        return goal_marginal(grid, wanted, max_goals, 0 if bool(home) == scored else 1)

    def _new_team_draws(self, team_name: str, team_covariates):
        """Parameters of a new team drawn from the fitted priors
        (bpl/neutral_dixon_coles.py:490-560)."""
        if team_name in self.teams:
            raise ValueError(f"Team {team_name} already known to model.")
        if self.attack_coefficients is not None:
            if team_covariates is None:
                warnings.warn(
                    f"You haven't provided features for {team_name}."
                    " Assuming team_covariates are the average of known teams."
                    " For better forecasts, provide team_covariates."
                )
                team_covariates = np.zeros(self.attack_coefficients.shape[1])
            else:
                team_covariates = (0.5 * (np.asarray(team_covariates) - self._team_covariates_mean)
                                   / self._team_covariates_std)
            mean_attack = np.dot(self.attack_coefficients, team_covariates.ravel())
            mean_defence = self.mean_defence + np.dot(self.defence_coefficients, team_covariates.ravel())
        else:
            mean_attack = 0.0
            mean_defence = self.mean_defence
        log_a_tilde = np.random.normal(loc=0.0, scale=1.0, size=len(self.std_attack))
        log_b_tilde = np.random.normal(loc=self.rho * log_a_tilde, scale=np.sqrt(1 - self.rho ** 2.0))
        home_attack = np.random.normal(loc=self.mean_home_attack, scale=self.std_home_attack)
        away_attack = np.random.normal(loc=self.mean_away_attack, scale=self.std_away_attack)
        home_defence = np.random.normal(loc=self.mean_home_defence, scale=self.std_home_defence)
        away_defence = np.random.normal(loc=self.mean_away_defence, scale=self.std_away_defence)
        attack = mean_attack + log_a_tilde * self.std_attack
        defence = mean_defence + log_b_tilde * self.std_defence
        self.teams = np.append(self.teams, team_name)
        self._teams_dict[team_name] = len(self._teams_dict)
        self.attack = np.concatenate((self.attack, attack[:, None]), axis=1)
        self.defence = np.concatenate((self.defence, defence[:, None]), axis=1)
        self.home_attack = np.concatenate((self.home_attack, home_attack[:, None]), axis=1)
        self.away_attack = np.concatenate((self.away_attack, away_attack[:, None]), axis=1)
        self.home_defence = np.concatenate((self.home_defence, home_defence[:, None]), axis=1)
        self.away_defence = np.concatenate((self.away_defence, away_defence[:, None]), axis=1)

    # ---- public API (bpl/neutral_dixon_coles.py:399-902)
    def _calculate_expected_goals(self, home_team, away_team, neutral_venue) -> Tuple[np.ndarray, np.ndarray]:
        """Poisson rates of the home and away goals."""
        return self._rates(*self._parse_fixture_args(home_team, away_team, neutral_venue))

    def predict_score_proba(self, home_team, away_team, home_goals, away_goals, neutral_venue) -> np.ndarray:
        """Probability of a particular scoreline between two teams (mean over draws)."""
        h, a, nv = self._parse_fixture_args(home_team, away_team, neutral_venue)
        return self._score_proba(h, a, home_goals, away_goals, nv)

    def add_new_team(self, team_name: str, team_covariates: Optional[np.ndarray] = None):
        """Add another team with parameters drawn from the fitted priors."""
        self._new_team_draws(team_name, team_covariates)

    def predict_score_grid_proba(self, home_team, away_team, neutral_venue,
                                 max_goals: Optional[int] = MAX_GOALS) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Scoreline probabilities on the (max_goals+1)^2 grid for every fixture."""
        h, a, nv = self._parse_fixture_args(home_team, away_team, neutral_venue)
        return self._grid(h, a, nv, None, max_goals)

    def predict_outcome_proba(self, home_team, away_team, neutral_venue, knockout: bool = False,
                              max_goals: Optional[int] = MAX_GOALS) -> Dict[str, np.ndarray]:
        """Home win, away win and draw probabilities; `knockout` renormalises over the wins."""
        h, a, nv = self._parse_fixture_args(home_team, away_team, neutral_venue)
        return self._outcome(h, a, nv, None, knockout, max_goals)

    def sample_score(self, home_team, away_team, neutral_venue, num_samples: int = 1,
                     random_state: int = None, max_goals: Optional[int] = MAX_GOALS) -> Dict[str, np.ndarray]:
        """Sample scorelines between two teams."""
        h, a, nv = self._parse_fixture_args(home_team, away_team, neutral_venue)
        return self._sample_score(h, a, nv, None, num_samples, random_state, max_goals)

    def sample_outcome(self, home_team, away_team, neutral_venue, knockout: bool = False,
                       num_samples: int = 1, random_state: int = None,
                       max_goals: Optional[int] = MAX_GOALS) -> np.ndarray:
        """Sample the winner ('Draw' unless `knockout`) of matches between two teams."""
        h, a, nv = self._parse_fixture_args(home_team, away_team, neutral_venue)
        return self._sample_outcome(h, a, nv, None, knockout, num_samples, random_state, max_goals)

    def predict_score_n_proba(self, n, team, opponent, home: Optional[bool] = True,
                              neutral_venue: Optional[int] = 0,
                              max_goals: Optional[int] = MAX_GOALS) -> np.ndarray:
        """Probability that `team` scores n goals against `opponent`."""
        t, o, _ = self._parse_fixture_args(team, opponent, neutral_venue)
        return self._n_proba(n, t, o, None, home, neutral_venue, max_goals, scored=True)

    def predict_concede_n_proba(self, n, team, opponent, home: Optional[bool] = True,
                                neutral_venue: Optional[int] = 0,
                                max_goals: Optional[int] = MAX_GOALS) -> np.ndarray:
        """Probability that `team` concedes n goals against `opponent`."""
        t, o, _ = self._parse_fixture_args(team, opponent, neutral_venue)
        return self._n_proba(n, t, o, None, home, neutral_venue, max_goals, scored=False)

    _ratings_venue_model = True   # team_ratings (bpl/ratings.py): the default venue is neutral ground

    # ---- tournament simulation (no reference counterpart)
    def _tournament_conf(self, team_conf, teams):
        """Confederation index per tournament team, or None: the plain class has no confederations."""
        if team_conf is not None:
            raise ValueError("team_conf is only taken by NeutralDixonColesMatchPredictorWC")
        return None

    def _tournament_team(self, name, what):
        if isinstance(name, (bool, np.bool_)) or not isinstance(name, (str, np.str_)) or name not in self._teams_dict:
            raise ValueError(f"{what}: unknown team {name!r}")
        return str(name)

    # pylint: disable=too-many-locals,too-many-branches,too-many-statements
    def _tournament_inputs(self, knockout, groups, advance, best_of_rest, group_fixtures, current_table, hosts,
                           points, num_simulations, team_conf, knockout_rule="redraw", legs=None,
                           extra_time_scale=EXTRA_TIME_SCALE, shootout=None, away_goals=False, best_allocation=None):
        """simulate_tournament's arguments checked and resolved on the host, before any device call.
        Returns a dict: "teams" (slot order), "team_idx", "conf" (or None), "host", "group" (or None),
        "group_names", "table" [n, 3], "fix_p" / "fix_q" (slots), "advance", "best_of_rest",
        "bracket" (u16 codes of bplhip_simulate_tournament), "rounds", "group_size", "points",
        "num_simulations", "knockout_rule"; under "extra_time" also "legs" [R] (1 / 2), "legs_mask",
        "extra_time_scale", "strength" f64 [n] and "away_goals"; "best_allocation", None or the checked table
        (bpl.allocation.check's form), and then "allocation", the arrays the device reads."""
        def is_int(v):
            return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))

        def is_real(v):
            return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))

        if not isinstance(knockout_rule, str) or knockout_rule not in KNOCKOUT_RULES:
            raise ValueError(f"knockout_rule must be one of {KNOCKOUT_RULES}, not {knockout_rule!r}")
        if not isinstance(away_goals, (bool, np.bool_)):
            raise ValueError("away_goals must be True or False")
        if not is_real(extra_time_scale) or not 0.0 < float(extra_time_scale) <= 1.0:
            raise ValueError("extra_time_scale must be a number in (0, 1]")
        if shootout is not None and not isinstance(shootout, dict):
            raise ValueError("shootout must be a dict {team: strength}")
        if knockout_rule == "redraw" and (legs is not None or float(extra_time_scale) != EXTRA_TIME_SCALE
                                          or shootout is not None or away_goals):
            raise ValueError('legs, extra_time_scale, shootout and away_goals need knockout_rule="extra_time"')

        num_simulations = check_simulations(num_simulations)
        points = check_points(points)
        knockout = list(knockout)
        nb = len(knockout)
        rounds = nb.bit_length() - 1
        if nb < 2 or nb != 1 << rounds or rounds > TOURNAMENT_MAX_ROUNDS:
            raise ValueError(f"knockout must have 2**R entries, 1 <= R <= {TOURNAMENT_MAX_ROUNDS}, not {nb}")
        group_of = {}
        if groups is None:
            if group_fixtures is not None or current_table is not None:
                raise ValueError("group_fixtures and current_table need groups")
            teams = [self._tournament_team(t, "knockout") for t in knockout]
            if len(set(teams)) != nb:
                raise ValueError("knockout: a team appears twice")
            group_names, group_size = [], 0
            bracket = np.arange(nb, dtype=np.uint16)
        else:
            group_names = list(groups)
            if not 1 <= len(group_names) <= TOURNAMENT_MAX_GROUPS:
                raise ValueError(f"there must be 1..{TOURNAMENT_MAX_GROUPS} groups, not {len(group_names)}")
            if "best" in group_names:
                raise ValueError("'best' is reserved for the best of the rest and cannot name a group")
            teams = []
            for gi, g in enumerate(group_names):
                members = [self._tournament_team(t, f"group {g!r}") for t in groups[g]]
                if not 2 <= len(members) <= TOURNAMENT_MAX_GROUP_SIZE:
                    raise ValueError(f"group {g!r} must have 2..{TOURNAMENT_MAX_GROUP_SIZE} teams")
                for t in members:
                    if t in group_of:
                        raise ValueError(f"team {t!r} is in two groups (or twice in one)")
                    group_of[t] = gi
                teams += members
            if len(teams) > TOURNAMENT_MAX_TEAMS:
                raise ValueError(f"at most {TOURNAMENT_MAX_TEAMS} teams")
            if not is_int(advance) or not 1 <= advance <= TOURNAMENT_MAX_GROUP_SIZE:
                raise ValueError(f"advance must be an integer in [1, {TOURNAMENT_MAX_GROUP_SIZE}]")
            sizes = [len(groups[g]) for g in group_names]
            group_size = max(sizes)
            rest_groups = sum(sz > advance for sz in sizes)
            if not is_int(best_of_rest) or not 0 <= best_of_rest <= rest_groups:
                raise ValueError(f"best_of_rest must be an integer in [0, {rest_groups}] (groups with a place "
                                 f"{advance + 1})")
            advance, best_of_rest = int(advance), int(best_of_rest)
            qualifiers = sum(min(advance, sz) for sz in sizes) + best_of_rest
            if qualifiers != nb:
                raise ValueError(f"{qualifiers} teams qualify but the knockout has {nb} entries")
            bracket = np.zeros(nb, dtype=np.uint16)
            seen = set()
            index = {g: i for i, g in enumerate(group_names)}
            for b, entry in enumerate(knockout):
                try:
                    ref, place = entry
                except (TypeError, ValueError):
                    raise ValueError(f"knockout[{b}] must be (group, place) or ('best', k)") from None
                if not is_int(place):
                    raise ValueError(f"knockout[{b}]: the place must be an integer")
                place = int(place)
                if ref == "best":
                    if not 1 <= place <= best_of_rest:
                        raise ValueError(f"knockout[{b}]: ('best', {place}) with best_of_rest = {best_of_rest}")
                    code = 0xFF00 | place
                elif ref in index:
                    if not 1 <= place <= min(advance, sizes[index[ref]]):
                        raise ValueError(f"knockout[{b}]: place {place} of group {ref!r} does not qualify")
                    code = index[ref] << 8 | place
                else:
                    raise ValueError(f"knockout[{b}]: unknown group {ref!r}")
                if code in seen:
                    raise ValueError(f"knockout[{b}]: {tuple(entry)!r} appears twice")
                seen.add(code)
                bracket[b] = code
        allocation = None
        if best_allocation is not None:
            if groups is None or best_of_rest == 0:
                raise ValueError("best_allocation needs groups and best_of_rest > 0: there is no best of the rest to "
                                 "allocate")
            best_allocation = _allocation.check(best_allocation, groups, best_of_rest, advance)
            allocation = _allocation.device_tables(best_allocation, group_names)
        slot = {t: i for i, t in enumerate(teams)}
        n = len(teams)
        host = np.zeros(n, dtype=np.uint8)
        for t in hosts or ():
            t = self._tournament_team(t, "hosts")
            if t not in slot:
                raise ValueError(f"hosts: {t!r} does not play in the tournament")
            host[slot[t]] = 1
        rule = {"knockout_rule": knockout_rule}
        if knockout_rule == "extra_time":
            if legs is None or is_int(legs):
                legs = [1 if legs is None else legs] * rounds
            try:
                legs = list(legs)
            except TypeError:
                raise ValueError("legs must be 1, 2 or one of them per knockout round") from None
            if len(legs) != rounds or not all(is_int(v) and int(v) in (1, 2) for v in legs):
                raise ValueError(f"legs must be 1, 2 or {rounds} values of 1 / 2, first round first")
            strength = np.zeros(n, dtype=np.float64)
            for name, v in (shootout or {}).items():
                t = self._tournament_team(name, "shootout")
                if t not in slot:
                    raise ValueError(f"shootout: {t!r} does not play in the tournament")
                if not is_real(v) or not abs(float(v)) <= TOURNAMENT_MAX_STRENGTH:
                    raise ValueError(f"shootout[{name!r}] must be a finite number, at most {TOURNAMENT_MAX_STRENGTH:g} "
                                     "in size")
                strength[slot[t]] = float(v)
            rule.update(legs=np.array(legs, dtype=np.uint8),
                        legs_mask=sum(1 << r for r, v in enumerate(legs) if int(v) == 2),
                        extra_time_scale=float(extra_time_scale), strength=strength, away_goals=bool(away_goals))
        conf = self._tournament_conf(team_conf, teams)
        table = np.zeros((n, 3), dtype=np.int64)
        fix_p, fix_q = [], []
        if groups is not None:
            for name, entry in (current_table or {}).items():
                t = self._tournament_team(name, "current_table")
                if t not in slot:
                    raise ValueError(f"current_table: {t!r} is in no group")
                vals = tuple(entry)
                if len(vals) != 3 or not all(is_int(v) for v in vals):
                    raise ValueError(f"current_table[{name!r}] must be (points, goals_for, goals_against) integers")
                if any(not 0 <= int(v) <= SEASON_MAX_TABLE_VALUE for v in vals):
                    raise ValueError(f"current_table[{name!r}] entries must be in [0, {SEASON_MAX_TABLE_VALUE}]")
                table[slot[t]] = [int(v) for v in vals]
            if group_fixtures is None:
                # a single round robin per group, in the given group order; within a group, member i meets
                # every later member k in the listed order: (0, 1), (0, 2), ..., (1, 2), ...
                for g in group_names:
                    members = [slot[str(t)] for t in groups[g]]
                    for i, p in enumerate(members):
                        for q in members[i + 1:]:
                            fix_p.append(p)
                            fix_q.append(q)
            else:
                for f, pair in enumerate(group_fixtures):
                    try:
                        home, away = pair
                    except (TypeError, ValueError):
                        raise ValueError(f"group_fixtures[{f}] must be a (home, away) pair") from None
                    home = self._tournament_team(home, f"group_fixtures[{f}]")
                    away = self._tournament_team(away, f"group_fixtures[{f}]")
                    if home not in slot or away not in slot or home == away or group_of[home] != group_of[away]:
                        raise ValueError(f"group_fixtures[{f}]: two different teams of one group")
                    fix_p.append(slot[home])
                    fix_q.append(slot[away])
                if len(fix_p) > SEASON_MAX_FIXTURES:
                    raise ValueError(f"at most {SEASON_MAX_FIXTURES} group fixtures")
        return {
            "teams": np.asarray(teams),
            "team_idx": np.array([self._teams_dict[t] for t in teams], dtype=DTYPES["teams"]),
            "conf": conf,
            "host": host,
            "group": None if groups is None else np.array([group_of[t] for t in teams], dtype=np.uint8),
            "group_names": group_names,
            "table": table,
            "fix_p": np.array(fix_p, dtype=np.uint8),
            "fix_q": np.array(fix_q, dtype=np.uint8),
            "advance": advance if groups is not None else 0,
            "best_of_rest": best_of_rest if groups is not None else 0,
            "bracket": bracket,
            "rounds": rounds,
            "group_size": group_size,
            "points": points,
            "num_simulations": num_simulations,
            "best_allocation": best_allocation,
            "allocation": allocation,
            **rule,
        }

    # pylint: disable=too-many-arguments
    def _tournament_in_play(self, in_play, inp):
        """simulate_tournament's `in_play` checked and resolved on the host: (slot p, slot q uint8, goals of p, goals
        of q uint8, elapsed float64), each [L], in the listed order.  ValueError, in `simulate_season`'s words where
        the condition is shared, for a missing column, unequal lengths, an unknown team, a team playing itself, two
        teams of different groups, goals that are not integers in 0..LIVE_MAX_GOALS, an elapsed outside [0, 1) or 0
        away from 0-0, and more than SEASON_MAX_FIXTURES fixtures and matches in play together."""
        try:
            cols = [in_play[k] for k in ("home_team", "away_team", "home_goals", "away_goals", "elapsed")]
            cols = [[c] if isinstance(c, (str, int, float, np.integer, np.floating)) else list(c) for c in cols]
        except (KeyError, TypeError, IndexError):
            raise ValueError("in_play must have home_team, away_team, home_goals, away_goals and elapsed") from None
        if len({len(c) for c in cols}) != 1:
            raise ValueError("in_play: every column must have the same length")
        slot = {str(t): i for i, t in enumerate(inp["teams"])}
        sides = []
        for col in cols[:2]:
            for t in col:
                if isinstance(t, (bool, np.bool_)) or not isinstance(t, (str, np.str_)) or str(t) not in slot:
                    raise ValueError("in_play: unknown team")
            sides.append(np.array([slot[str(t)] for t in col], dtype=np.uint8))
        p, q = sides
        if np.any(p == q):
            raise ValueError("in_play: a team cannot play itself")
        if p.size and np.any(inp["group"][p] != inp["group"][q]):
            raise ValueError("in_play: two different teams of one group")
        goals = []
        for col in cols[2:4]:
            for g in col:
                ok = not isinstance(g, (bool, np.bool_)) and isinstance(g, (int, float, np.integer, np.floating))
                if not ok or not np.isfinite(g) or int(g) != g or not 0 <= g <= LIVE_MAX_GOALS:
                    raise ValueError(f"in_play: current goals must be integers in 0..{LIVE_MAX_GOALS}, not {g!r}")
            goals.append(np.array([int(g) for g in col], dtype=np.uint8))
        t = _inplay.check_elapsed(cols[4], p.size)
        if np.any((t == 0.0) & ((goals[0] != 0) | (goals[1] != 0))):
            raise ValueError("in_play: elapsed = 0 with a score other than 0-0")
        if inp["fix_p"].size + p.size > SEASON_MAX_FIXTURES:
            raise ValueError(f"at most {SEASON_MAX_FIXTURES} group fixtures, those in play included")
        return p, q, goals[0], goals[1], t

    def _tournament_call(self, knockout, groups, advance, best_of_rest, group_fixtures, current_table, hosts, points,
                         num_simulations, random_state, team_conf, tiebreak, played, knockout_rule, legs,
                         extra_time_scale, shootout, away_goals, best_allocation=None, in_play=None, log_weights=None,
                         live=False):
        """What simulate_tournament and tournament_paths do before the device call: every argument checked
        (_tournament_inputs), the `played` matches and the head-to-head records prepared, the seed drawn.  Returns
        (inp, {"args", "kwargs"}): the checked inputs and the device method's arguments; "allocation" is among the
        keywords only under a `best_allocation`.  `live` (simulate_tournament and the three queries under `in_play` or
        `log_weights`): `in_play` and `log_weights` are checked as well, the matches in play count as meetings to come, inp gains "in_play" (_tournament_in_play's
        columns, L = 0 without any) and the keywords "in_play" and "log_weights"."""
        head_to_head = check_tiebreak(tiebreak)
        if played is not None and groups is None:
            raise ValueError("played needs groups")
        if in_play is not None and (groups is None or group_fixtures is None):
            raise ValueError("in_play needs groups and an explicit group_fixtures (the matches still to kick off, [] "
                             "for none): group_fixtures=None would replay the whole round robin")
        derive = played is not None and current_table is None
        inp = self._tournament_inputs(knockout, groups, advance, best_of_rest, group_fixtures, current_table, hosts,
                                      points, num_simulations, team_conf, knockout_rule, legs, extra_time_scale,
                                      shootout, away_goals, best_allocation)
        meet_p, meet_q = inp["fix_p"], inp["fix_q"]
        if live:
            none = {k: () for k in ("home_team", "away_team", "home_goals", "away_goals", "elapsed")}
            inp["in_play"] = ip = self._tournament_in_play(none if in_play is None else in_play, inp)
            lw = _inplay.check_log_weights(log_weights, int(np.asarray(self.corr_coef).shape[0]))
            meet_p, meet_q = np.concatenate([meet_p, ip[0]]), np.concatenate([meet_q, ip[1]])
        n = len(inp["teams"])
        pair = None
        if played is not None:
            slot_of = {str(t): i for i, t in enumerate(inp["teams"])}
            hs, as_, _, _ = played_matches(played, slot_of)
            if np.any(inp["group"][hs] != inp["group"][as_]):
                raise ValueError("played: a match between teams of different groups")
            if derive:
                inp["table"] = table_from_played(played, slot_of, n, inp["points"])
                if inp["table"].max(initial=0) > SEASON_MAX_TABLE_VALUE:
                    raise ValueError(f"played: table entries must be in [0, {SEASON_MAX_TABLE_VALUE}]")
        if head_to_head:
            pair = pair_records(played, None if played is None else slot_of, n, inp["points"],
                                remaining=remaining_meetings(meet_p, meet_q, n))
        extra = {"pair_init": pair, "head_to_head": True} if head_to_head else {}
        if inp["knockout_rule"] == "extra_time":
            extra["knockout"] = {"legs_mask": inp["legs_mask"], "scale": inp["extra_time_scale"],
                                 "away_goals": inp["away_goals"], "strength": inp["strength"]}
        if inp["allocation"] is not None:
            extra["allocation"] = inp["allocation"]
        if live:
            extra.update(in_play=ip, log_weights=lw)
        seed = _wall_clock_seed() if random_state is None else random_state
        kwargs = dict(team_conf=inp["conf"], team_host=inp["host"], team_group=inp["group"], table=inp["table"],
                      fix_p=inp["fix_p"], fix_q=inp["fix_q"], advance=inp["advance"],
                      best_of_rest=inp["best_of_rest"], points=inp["points"], **extra)
        return inp, {"args": (inp["team_idx"], inp["bracket"], inp["num_simulations"], prng_key(seed)),
                     "kwargs": kwargs}

    # pylint: disable=too-many-arguments
    def simulate_tournament(self, knockout, groups: Optional[Dict] = None, advance: int = 2, best_of_rest: int = 0,
                            group_fixtures=None, current_table: Optional[Dict] = None, hosts=None,
                            points: Tuple[int, int, int] = (3, 1, 0), num_simulations: int = 10_000,
                            random_state: int = None, return_stages: bool = False,
                            team_conf: Optional[Dict] = None, tiebreak: str = "overall",
                            played: Optional[Dict] = None, knockout_rule: str = "redraw", legs=None,
                            extra_time_scale: float = EXTRA_TIME_SCALE, shootout: Optional[Dict] = None,
                            away_goals: bool = False, best_allocation=None, in_play: Optional[Dict] = None,
                            reweight: bool = True, log_weights=None,
                            return_weights: bool = False) -> Dict[str, np.ndarray]:
        """Group and knockout odds from simulating a tournament (no reference counterpart).

        `groups` ({name: [teams]}, 1..16 groups of 2..8 teams, at most 64 teams) play `group_fixtures`
        ([(home, away), ...], both of one group; default: a single round robin of every group, group
        by group in the given order, member i against every later member k in the listed order) on
        top of `current_table` (name -> (points, goals_for, goals_against), as in `simulate_season`).
        A group is ranked by points (`points` = (win, draw, loss)), goal difference, goals for and a
        random tie-break (the head-to-head rule: see `tiebreak`).  The top `advance` of each group qualify, and the
        best `best_of_rest` of the teams placed advance + 1 (ranked across the groups by the same
        keys).  `knockout` is the first knockout round in bracket order, 2**R entries (1 <= R <= 6):
        entry 2k meets entry 2k + 1 and the winners of matches 2m and 2m + 1 meet next.  With groups
        an entry is (group name, place) (1-based, at most `advance`) or ("best", k) (the k-th best
        of the rest), every qualifier exactly once; without groups it is a team.

        A match with exactly one team of `hosts` is played at the host's venue (the host is the home
        side, neutral_venue = 0); every other match is neutral.  A level knockout scoreline is drawn
        again from the same posterior draw, up to 32 attempts, so the winner comes from that draw's
        scoreline distribution conditioned on a winner; after 32 level attempts (probability about
        1e-17) the first-listed side goes through.  Simulation j plays every match from posterior
        draw j mod draws, so the uncertainty all matches share stays in the odds.  The device kernel
        is csrc/dc_tournament.hip.h.

        `tiebreak="head_to_head"` (default "overall": the order above, same kernel and results as without
        the keyword) orders the teams of a group that are level on points by the matches between them first
        -- points, goal difference, goals scored in those matches -- and only then by overall goal difference,
        goals for and the random tie-break (csrc/dc_h2h.hip.h), as `simulate_season` does; the mini-table is
        formed once over all teams of the group level on points (UEFA's re-application of the criteria to a
        still-tied subset is not modelled, nor is La Liga's omission of the head-to-head goals scored).  The
        best of the rest keep the overall keys: teams of different groups have no matches between them.
        `played` (a dict with home_team, away_team, home_goals, away_goals) lists the group matches already
        played: it fills the head-to-head records, and when `current_table` is None the current table is
        computed from it with `points`; with both, `current_table` supplies the totals and the two are not
        cross-checked.  ValueError as in `simulate_season`, and for a `played` match between two groups.

        `knockout_rule="extra_time"` (default "redraw": the rule above, same kernel and results as without the
        keyword) plays a level knockout match the way competitions do (csrc/dc_knockout.hip.h).  `legs` is None
        or 1 (single matches), 2, or one value of 1 / 2 per knockout round, first round first.  A single match
        is played at the venue the hosts give; a two-legged tie has the first-listed entry at home in leg 1 and
        the second-listed at home in leg 2 (neutral_venue = 0 in both, `hosts` not read), and the higher
        aggregate goes through; with `away_goals` a level aggregate goes to the side with more goals scored
        away.  A tie still level plays extra time at the venue of the only or the second leg, drawn from the
        same posterior draw with both rates times `extra_time_scale` (in (0, 1], default 1/3: 30 minutes of
        90) and the same corr_coef, and then a shoot-out, which the first-listed side p wins against q with
        probability 1 / (1 + exp(-(shootout[p] - shootout[q]))) (`shootout`: {team: strength}, finite, at most
        20 in size, 0 for teams not named: an even shoot-out).  Nothing is redrawn.  Under one `random_state` a
        single match that is not level after 90 minutes has the "redraw" rule's winner.  Not modelled: a
        third-place play-off; away goals applied to extra time (they count after the two legs only); the order
        of the penalties or any shoot-out skill beyond one strength per team; groups larger than eight; and
        `predict_outcome_proba(knockout=True)`, which works on the posterior-mean grid and keeps its own rule.
        The new arguments raise ValueError when malformed, and when given under "redraw".

        `best_allocation` (default None: ("best", k) is the k-th best of the rest by rank, same kernel and results
        as without the keyword) fills the bracket the way the Euros since 2016 and the World Cup from 2026 do: by
        WHICH groups the qualifiers placed advance + 1 come from.  It is a mapping from those B = `best_of_rest`
        groups (a tuple or frozenset of names, any order) to the same groups in slot order -- element k - 1 is the
        group whose team takes the bracket position of ("best", k), which then reads "allocation slot k" -- with
        one row for every combination of B groups that have a place advance + 1 (bpl/allocation.py: `check`, the
        validator; `from_constraints`, a table from the rule behind one; `format_table`).  Which teams qualify does
        not change, nor any random number: under one `random_state` simulation j has the same scorelines, group
        positions and qualifiers with and without the table, and differs only in the bracket positions of the best
        of the rest and the knockout that follows.  ValueError for a table without `groups` or with `best_of_rest`
        = 0, one that is no mapping, an unknown group or one without a place advance + 1, a key that is not B
        distinct groups, a value that is no permutation of its key, and a missing or repeated combination.  Not
        modelled: allocation by anything but the set of groups (rank among the thirds, confederation, pot);
        several allocation tiers (say thirds and fourths allocated separately); and the league and dynamic classes.

        Returns numpy arrays: "teams" [n] (the groups flattened in the given order, else bracket
        order); "round_proba" [n, R + 1] (column r < R: P(the team plays knockout round r, 0 = the
        first, R - 1 = the final), column R: P(it wins)); with groups "group_position_proba"
        [n, largest group] (0 = top); with return_stages "stage" uint8 [num_simulations, n]
        (0 = out in the groups, r + 1 = furthest column r reached).  Under "extra_time" also "decided_proba"
        [R, 4] (the share of round r's matches decided in normal time / by away goals / in extra time / by the
        shoot-out) and with return_stages "decided" uint8 [num_simulations, 2**R - 1] (the same 0..3 per match,
        the matches numbered over the rounds, first round first).  Under a `best_allocation` also "best_slot_count"
        int64 [groups, B] (how often the team placed advance + 1 in group g took allocation slot k, counted on the
        device) and "best_slot_proba" = best_slot_count / num_simulations.

        `in_play` (default None), `log_weights` (default None) and `reweight`: the tournament on a day with group
        matches IN PROGRESS, and with re-weighted posterior draws (csrc/dc_tournament_live.hip.h).  With
        `in_play=None`, `log_weights=None` and `return_weights=False` nothing changes: the same kernels, the same
        results, the same keys.  `in_play` is a dict with home_team, away_team (the first- and second-listed side, as
        in `group_fixtures`: two different teams of one group), home_goals, away_goals (the current score of the
        listed sides, integers in 0..63) and elapsed (the fraction of the match played, in [0, 1); 0 only at 0-0 --
        `predict_in_play`'s rule), each of length L >= 0.  These matches come IN ADDITION to `group_fixtures`, which
        then lists only the matches still to kick off and must be given ([] for none: None would replay the whole
        round robin, a ValueError); `current_table` and `played` describe the table WITHOUT them.  A match in play
        has its venue decided like any group fixture (a host listed second is the home side: the sides swap and the
        two goal counts with them; the outputs stay in the listed order), draws its final score from that posterior
        draw's conditional law given the state -- remaining goals thinned by 1 - elapsed, tau on the final score
        with the full-match rates of the tournament, `simulate_season`'s law, sampled exactly -- is group fixture
        F + m of the concatenated list (at 0-0 with elapsed = 0 bit for bit the ordinary fixture at that position),
        and is booked once, into the table and the head-to-head records, where it counts as a meeting to come.  With
        `reweight` (default True) and L > 0 the draws are weighted by the joint likelihood of all the states, a
        `log_weights` (float64 [draws], finite: a row of `sequential_scores(return_weights=True)["log_weights"]`,
        say) is added to the log weights, with `in_play=None` and without groups too: the tournament updated without
        a refit.  With weights in force simulation j plays every match on the draw that systematic resampling
        selects (`simulate_season`'s formula and random block); otherwise on draw j mod draws.  All modes compose:
        both tie-breaks, both knockout rules, with and without `best_allocation`.  The result gains "ess" and
        "log_evidence" (`simulate_season`'s definitions: the number of draws and 0.0 / NaN without weights in
        force); with return_stages "draw" int32 [num_simulations] and "in_play_home_goals" / "in_play_away_goals"
        uint8 [num_simulations, L] (FINAL scores of the listed sides); with `return_weights` "log_weights" = L - max
        L, which `predict_in_play(reweight=False, log_weights=...)` takes.  ValueError, before any device call, for a
        malformed `in_play` (in `simulate_season`'s words), `in_play` without `groups` or an explicit
        `group_fixtures`, two sides of different groups, more than 2**20 fixtures and matches in play together, and
        `log_weights` of another shape or not finite.  `tournament_paths`, `tournament_scenarios` and
        `tournament_points` take the same three keywords and play the same simulations.  Not modelled: knockout
        matches in play; the dynamic and league classes; a joint update across tournaments."""
        live = in_play is not None or log_weights is not None or bool(return_weights)
        inp, call = self._tournament_call(knockout, groups, advance, best_of_rest, group_fixtures, current_table, hosts,
                                          points, num_simulations, random_state, team_conf, tiebreak, played,
                                          knockout_rule, legs, extra_time_scale, shootout, away_goals, best_allocation,
                                          in_play, log_weights, live)
        if not live:
            raw = self._device().simulate_tournament(*call["args"], return_stages=return_stages, **call["kwargs"])
            return tournament_result(inp, raw)
        raw = self._device().simulate_tournament_live(*call["args"], return_stages=return_stages,
                                                      reweight=bool(reweight), return_weights=bool(return_weights),
                                                      **call["kwargs"])
        return tournament_live_result(inp, raw, bool(return_weights))


    # pylint: disable=too-many-arguments
    def tournament_paths(self, knockout, groups: Optional[Dict] = None, advance: int = 2, best_of_rest: int = 0,
                         group_fixtures=None, current_table: Optional[Dict] = None, hosts=None,
                         points: Tuple[int, int, int] = (3, 1, 0), num_simulations: int = 10_000,
                         random_state: int = None, team_conf: Optional[Dict] = None, tiebreak: str = "overall",
                         played: Optional[Dict] = None, knockout_rule: str = "redraw", legs=None,
                         extra_time_scale: float = EXTRA_TIME_SCALE, shootout: Optional[Dict] = None,
                         away_goals: bool = False, return_records: bool = False,
                         best_allocation=None, in_play: Optional[Dict] = None, reweight: bool = True,
                         log_weights=None) -> Dict[str, np.ndarray]:
        """Who a team meets in each knockout round, what a group place is worth and which group match matters,
        from `simulate_tournament`'s simulations (no reference counterpart).

        Every argument but `return_records` is `simulate_tournament`'s, checked by the same code (ValueError as
        there, before any device call; the World-Cup class takes `team_conf`).  Under one `random_state`
        simulation j here is simulation j there -- the same posterior draw, scorelines, ranking, bracket and
        winners, under either tie-break and either knockout rule -- so "round_proba", "group_position_proba" and
        "decided_proba" are `simulate_tournament`'s arrays bit for bit.  The simulations are cross-tabulated on the
        device (csrc/dc_paths.hip.h); the floats are formed on the host from the integer tables (bpl/paths.py,
        which also has `opponents` and `format_table` to read a result).

        With n slots in the order of "teams", R knockout rounds, K = R + 1 targets "targets" ("round_0" ..: plays
        that knockout round; "winner"), P the largest group and nf group fixtures, returns int64 tables
        "stage_count" [n, R + 2] (furthest stage, 0 = out in the groups), "meet_count" [R, n, n] (t and u play
        each other in round r; a two-legged tie is one meeting; the last round's table is the table of finals),
        "advance_count" [R, n, n] (t goes through against u; meet = advance + its transpose), with groups
        "position_stage_count" [n, P, R + 2], and with group fixtures "outcome_count" [nf, 3], "target_count"
        [n, K] and "joint_count" [nf, 3, n, K], `match_leverage`'s tables with the outcome in the LISTED order of
        the fixture ("fixtures" [nf, 2], slots: 0 = the first-listed side wins, 1 = draw, 2 = the second-listed
        wins -- also when a host listed second plays at home).  Floats: "meet_proba"; "opponent_proba" [R, n, n]
        = P(u is the opponent | t plays round r), NaN where t never does; "advance_given_meet" [R, n, n], NaN where
        the two never met -- the posterior-predictive head-to-head in the round the bracket lets them meet;
        "round_proba_given_position" [n, P, K] = P(t plays round k | t finishes p-th in its group), NaN where that
        never happened; and for the group fixtures "outcome_proba", "target_proba", "conditional_proba",
        "conditional_se" and "leverage" [nf, n, K] as in `match_leverage`.  Keys that need groups, or group
        fixtures, are absent without them.

        `return_records=True` adds the per-simulation records the tables were counted from, uint8: "stage"
        [N, n], "position" [N, n] (with groups), "group_outcome" [N, nf] (0 / 1 / 2), "pair" [N, 2**R - 1, 2] (the
        two slots of every knockout match in listed order, matches numbered over the rounds, first round first),
        "winner" [N, 2**R - 1] and under "extra_time" "decided" as in `simulate_tournament`.

        `in_play`, `reweight` and `log_weights` are `simulate_tournament`'s, with its meaning, checks and errors
        (csrc/dc_tournament_live_queries.hip.h); at their defaults nothing changes: the same kernels, results and
        keys.  Live -- `in_play` or `log_weights` given -- simulation j is simulation j of the live
        `simulate_tournament`: the same draw (systematic resampling when weights are in force), ordinary fixtures,
        conditional final scores, ranking, allocation fill and knockout, so "round_proba", "group_position_proba" and
        "decided_proba" are its arrays bit for bit.  The group-fixture axis becomes the concatenated list, the F
        fixtures of `group_fixtures` still to kick off and then the L matches in play (F + L at most 4096): "fixtures",
        "outcome_count", "joint_count", "conditional_proba", "conditional_se" and "leverage" have F + L rows, a match
        in play classed by its FINAL score in the listed order, and "in_play" int64 [L] names the rows F..F+L-1, as
        in `match_leverage`.  The result gains "ess" and "log_evidence", and with `return_records` "draw" int32 [N],
        "in_play_home_goals" / "in_play_away_goals" uint8 [N, L] (final scores, listed order) and L more columns of
        "group_outcome".  `log_weights` alone is allowed on a knockout-only bracket.

        Not modelled: a third-place match; the legs' individual scorelines; knockout matches in play; and nothing
        beyond `simulate_tournament`'s own limits (at most 4096 group fixtures here, those in play included).
        `tournament_scenarios` is the counterpart of `match_scenarios`, `tournament_points` that of `points_needed`."""
        live = in_play is not None or log_weights is not None
        inp, call = self._tournament_call(knockout, groups, advance, best_of_rest, group_fixtures, current_table, hosts,
                                          points, num_simulations, random_state, team_conf, tiebreak, played,
                                          knockout_rule, legs, extra_time_scale, shootout, away_goals, best_allocation,
                                          in_play, log_weights, live)
        if not isinstance(return_records, (bool, np.bool_)):
            raise ValueError("return_records must be True or False")
        if not live:
            raw = self._device().tournament_paths(*call["args"], return_records=bool(return_records), **call["kwargs"])
            return paths_result(inp, raw)
        if inp["fix_p"].size + inp["in_play"][0].size > LEVERAGE_MAX_FIXTURES:
            raise ValueError(f"at most {LEVERAGE_MAX_FIXTURES} group fixtures, those in play included")
        raw = self._device().tournament_paths_live(*call["args"], return_records=bool(return_records),
                                                   reweight=bool(reweight), **call["kwargs"])
        return paths_result(live_inputs(inp), raw)

    # pylint: disable=too-many-arguments
    def tournament_scenarios(self, knockout, fixtures, groups: Optional[Dict] = None, advance: int = 2,
                             best_of_rest: int = 0, group_fixtures=None, current_table: Optional[Dict] = None,
                             hosts=None, points: Tuple[int, int, int] = (3, 1, 0), num_simulations: int = 10_000,
                             random_state: int = None, team_conf: Optional[Dict] = None, tiebreak: str = "overall",
                             played: Optional[Dict] = None, knockout_rule: str = "redraw", legs=None,
                             extra_time_scale: float = EXTRA_TIME_SCALE, shootout: Optional[Dict] = None,
                             away_goals: bool = False, margin_cap=1,
                             return_records: bool = False, best_allocation=None, in_play: Optional[Dict] = None,
                             reweight: bool = True, log_weights=None) -> Dict[str, np.ndarray]:
        """The joint result of a few chosen group matches against every team's knockout targets: "we go through if
        we win, or if we draw and they lose by two; we win the group only if ...", over `simulate_tournament`'s
        simulations (no reference counterpart; the tournament form of `match_scenarios`).

        Every argument but `fixtures`, `margin_cap` and `return_records` is `simulate_tournament`'s, checked by the
        same code (ValueError as there, before any device call; the World-Cup class takes `team_conf`).  Under one
        `random_state` simulation j here IS simulation j of `simulate_tournament` and `tournament_paths` -- the same
        posterior draw, scorelines, ranking, bracket and winners, under either tie-break and either knockout rule.
        `fixtures` names the key fixtures as positions in the group-fixture list -- `group_fixtures` as given, or
        the default round robin in its documented order: the list `tournament_paths` returns as "fixtures" -- 1..8
        distinct integers; `margin_cap` is an integer c in 1..3, or one per key (both checked by
        `bpl.scenarios.check_keys`).  Without groups, or with an empty group-fixture list, there is nothing to key
        on: ValueError.  A key fixture with cap c has 2 c + 1 classes, class = c - clip(first-listed goals -
        second-listed goals, -c, c): the LISTED orientation, as in `tournament_paths`, also when a host listed
        second plays at home; with c = 1 the classes are `tournament_paths`' outcomes 0 / 1 / 2.  A scenario is one
        class per key, indexed row-major in the order given; more than 6561 scenarios raise ValueError.

        The K = R + 2 targets are `tournament_paths`' "round_0" .. "round_{R-1}" (plays that knockout round) and
        "winner", plus "group_winner" (first in its group).  The result has `match_scenarios`' keys, so
        `bpl.scenarios`' `marginal`, `coarsen`, `requirements` and `format_table` take it unchanged: "teams" [n]
        (slot order); "targets" [K]; "fixtures" int64 [k] (the key positions) with "home" and "away" [k], where
        "home" reads "first-listed" and "away" "second-listed" (margins and classes follow the listing, not the
        venue); "margin_cap", "shape", "margins"; the integer tables counted on the device
        (csrc/dc_tscen.hip.h), int64: "scenario_count" [M] and "joint_count" [M, n, K]; and from those integers
        "scenario_proba", "target_count" [n, K], "target_proba", "conditional_proba" and "conditional_se" [M, n, K]
        (NaN exactly where the scenario never occurred), "settled" int8 [M, n, K] and "leverage" [n, K], all as in
        `match_scenarios`; "round_proba" [n, R + 1] = target_count[:, :R + 1] / N, `simulate_tournament`'s array
        bit for bit; under "extra_time" "decided_proba" as there.  `return_records=True` adds the per-simulation
        "scenario" uint32 [N] (the scenario index) and "target_set" uint8 [N, n] (bit k: inside target k).

        "settled" is about the SIMULATED tournaments, not mathematical certainty, and the conditional is the
        posterior-predictive one, as in `match_scenarios`.

        `in_play`, `reweight` and `log_weights` are `simulate_tournament`'s, with its meaning, checks and errors
        (csrc/dc_tournament_live_queries.hip.h) -- the question is asked on the last group matchday, at 1-0 after an
        hour; at their defaults nothing changes: the same kernels, results and keys.  Live -- `in_play` or
        `log_weights` given -- simulation j is simulation j of the live `simulate_tournament` and `tournament_paths`.
        `fixtures` then indexes the concatenated list, the F fixtures of `group_fixtures` still to kick off and then
        the L matches in play: F + m names match m in play, whose class is formed from its FINAL score in the listed
        order, so a class the current score has ruled out has "scenario_count" 0 and NaN conditionals; "home" and
        "away" come from that list.  The result gains "ess" and "log_evidence", and with `return_records` "draw"
        int32 [N] and "in_play_home_goals" / "in_play_away_goals" uint8 [N, L].

        Not modelled: keys among the knockout matches (the match in a given bracket position is a different
        pairing in every simulation); margins beyond +-3, or more than 8 keys; group places other than first as
        targets (`tournament_paths`' "round_proba_given_position" covers what a place is worth); and knockout matches
        in play.  Group points and goal difference against the same targets are `tournament_points`'."""
        live = in_play is not None or log_weights is not None
        inp, call = self._tournament_call(knockout, groups, advance, best_of_rest, group_fixtures, current_table, hosts,
                                          points, num_simulations, random_state, team_conf, tiebreak, played,
                                          knockout_rule, legs, extra_time_scale, shootout, away_goals, best_allocation,
                                          in_play, log_weights, live)
        shown = live_inputs(inp) if live else inp   # (the concatenated list)
        if inp["group"] is None or shown["fix_p"].size == 0:
            raise ValueError("tournament_scenarios needs groups and at least one group fixture: there is nothing to "
                             "key on (knockout matches cannot be keys)")
        keys, caps = _scenarios.check_keys(fixtures, margin_cap, shown["fix_p"].size)
        if not isinstance(return_records, (bool, np.bool_)):
            raise ValueError("return_records must be True or False")
        if not live:
            raw = self._device().tournament_scenarios(*call["args"], return_records=bool(return_records),
                                                      key_fixture=keys, key_cap=caps, **call["kwargs"])
            return scenarios_result(inp, keys, caps, raw)
        raw = self._device().tournament_scenarios_live(*call["args"], return_records=bool(return_records),
                                                       key_fixture=keys, key_cap=caps, reweight=bool(reweight),
                                                       **call["kwargs"])
        return scenarios_result(shown, keys, caps, raw)

    # pylint: disable=too-many-arguments
    def tournament_points(self, knockout, groups: Optional[Dict] = None, advance: int = 2, best_of_rest: int = 0,
                          group_fixtures=None, current_table: Optional[Dict] = None, hosts=None,
                          points: Tuple[int, int, int] = (3, 1, 0), num_simulations: int = 10_000,
                          random_state: int = None, team_conf: Optional[Dict] = None, tiebreak: str = "overall",
                          played: Optional[Dict] = None, knockout_rule: str = "redraw", legs=None,
                          extra_time_scale: float = EXTRA_TIME_SCALE, shootout: Optional[Dict] = None,
                          away_goals: bool = False, levels=(0.5, 0.9, 0.99), gd_cap: int = 3,
                          best_allocation=None, in_play: Optional[Dict] = None, reweight: bool = True,
                          log_weights=None) -> Dict[str, np.ndarray]:
        """How many group points it takes: every team's group-stage points cross-tabulated against its knockout
        targets and its group place, the points of every group place, and the points and goal difference of the
        teams placed advance + 1 against their rank across the groups -- "are four points enough", "what does the
        last third-placed team that goes through usually have" -- over `simulate_tournament`'s simulations (no
        reference counterpart; the tournament form of `points_needed`).

        Every argument but `levels` and `gd_cap` is `simulate_tournament`'s, checked by the same code (ValueError as
        there, before any device call; the World-Cup class takes `team_conf`).  Under one `random_state` simulation j
        here IS simulation j of `simulate_tournament`, `tournament_paths` and `tournament_scenarios` -- the same
        posterior draw, scorelines, ranking, bracket and winners, under either tie-break and either knockout rule.
        `levels` is `points_needed`'s (non-empty, every value in (0, 1]); `gd_cap` is an integer c in 0..8.  Without
        `groups` there are no group points: ValueError.  An empty `group_fixtures` list with a `current_table` is
        allowed: the group stage is then the same in every simulation.

        The axes: "points" [P], `points_needed`'s axis over the slots (a team with m group fixtures ends on its
        current points + m min(points) .. + m max(points)), more than 256 bins raise ValueError; "goal_difference"
        [D = 2 c + 1], the values -c .. c of a team's overall group goal difference (current table plus simulated
        matches) clipped to +-c, so the end bins read "c or more" in size.  The K = R + 2 "targets" are
        `tournament_scenarios`': "round_0" .. "round_{R-1}" (plays that knockout round; "round_0" = gets out of the
        group), "winner" and "group_winner".  With n slots in "teams" order, Gn groups ("groups") of at most Z teams,
        B groups with a place advance + 1, L levels and N simulations, the integer tables counted on the device
        (csrc/dc_group_points.hip.h), int64: "team_points_count" [n, P]; "team_target_count" [n, P, K];
        "team_place_count" [n, P, Z] (place z of its group, 0 = top); "place_points_count" [Gn, Z, P] (the team on
        place z of group g had p points; zero for a place a smaller group lacks); "place_gap_count" [Gn, Z - 1, P]
        (the points of place z minus those of place z + 1, column 0 = level on points: decided by the tie-break);
        and with `best_of_rest` > 0 "rest_count" and "rest_through_count" [P, D] (the teams placed advance + 1,
        pooled over groups and simulations; those of them among the best `best_of_rest`) and "rest_rank_count"
        [B, P, D] (the k-th best of them, ranked as the bracket ranks them; row best_of_rest - 1 is the cut line).

        From those integers (bpl/group_points.py, which also has `cut_line` and `format_table`): "team_points_proba";
        "target_count" [n, K] and "target_proba"; "round_proba" [n, R + 1] and "group_position_proba" [n, Z],
        `simulate_tournament`'s arrays bit for bit; "proba_given_points", "se_given_points", "proba_given_at_least"
        [n, P, K] and "points_needed" [n, K, L] as in `points_needed`; "place_given_points" [n, P, Z];
        "place_points_mean" [Gn, Z] (NaN for a place the group lacks) and "place_points_quantile" int64 [L, Gn, Z]
        (the inverted CDF, no interpolation; -1 for such a place); "level_proba" [Gn, Z - 1]; with a best of the
        rest "rest_proba" [P, D] (NaN where the cell never occurred), "rest_proba_given_at_least" [P] (pooled over
        the goal difference), "rest_points_needed" [L] (under `points_needed`'s "reached at least once" rule),
        "cut_points_proba" [P] and "cut_proba" [P, D]; under "extra_time" "decided_proba" as in
        `simulate_tournament`.  Every conditional is the posterior-predictive one, as in `points_needed`.

        `in_play`, `reweight` and `log_weights` are `simulate_tournament`'s, with its meaning, checks and errors
        (csrc/dc_tournament_live_queries.hip.h); at their defaults nothing changes: the same kernels, results and
        keys.  Live -- `in_play` or `log_weights` given -- simulation j is simulation j of the live
        `simulate_tournament`, `tournament_paths` and `tournament_scenarios`; the matches in play are matches to come
        on the points axis (its bounds are formed from the meetings of `group_fixtures` and `in_play` together), the
        tables keep their shapes and meaning, and the result gains "ess" and "log_evidence".

        Not modelled: knockout matches in play; rest tables per team; a goal-difference axis for anything but the
        rest tables; knockout-stage statistics beyond the targets; and the league and dynamic classes."""
        live = in_play is not None or log_weights is not None
        inp, call = self._tournament_call(knockout, groups, advance, best_of_rest, group_fixtures, current_table, hosts,
                                          points, num_simulations, random_state, team_conf, tiebreak, played,
                                          knockout_rule, legs, extra_time_scale, shootout, away_goals, best_allocation,
                                          in_play, log_weights, live)
        if inp["group"] is None:
            raise ValueError("tournament_points needs groups: without them there are no group points")
        levels = check_levels(levels)
        gd_cap = _group_points.check_gd_cap(gd_cap)
        shown = live_inputs(inp) if live else inp   # (the concatenated list)
        points_min, n_bins = points_axis(inp["table"][:, 0], shown["fix_p"], shown["fix_q"], inp["points"])
        if n_bins > _group_points.MAX_BINS:
            raise ValueError(f"the points axis would have {n_bins} bins ({points_min}..{points_min + n_bins - 1} "
                             f"points); at most {_group_points.MAX_BINS}")
        if not live:
            raw = self._device().tournament_points(*call["args"], points_min=points_min, n_bins=n_bins, gd_cap=gd_cap,
                                                   **call["kwargs"])
            return points_result(inp, raw, points_min, levels)
        raw = self._device().tournament_points_live(*call["args"], points_min=points_min, n_bins=n_bins, gd_cap=gd_cap,
                                                    reweight=bool(reweight), **call["kwargs"])
        return points_result(inp, raw, points_min, levels)


def tournament_result(inp, raw) -> Dict[str, np.ndarray]:
    """simulate_tournament's dict from the raw integer counts (device or restatement)."""
    counts = raw["stage_counts"].astype(np.int64)
    n_sims = inp["num_simulations"]
    reached = np.cumsum(counts[:, ::-1], axis=1)[:, ::-1]   # [n, R + 2]: stage >= k
    out = {"teams": inp["teams"], "round_proba": reached[:, 1:] / n_sims}
    if inp["group"] is not None:
        out["group_position_proba"] = raw["position_counts"][:, :inp["group_size"]].astype(np.int64) / n_sims
    if "decided_counts" in raw:
        # round r has 2^(R - 1 - r) matches per simulation
        matches = n_sims * (1 << np.arange(inp["rounds"] - 1, -1, -1, dtype=np.int64))
        out["decided_proba"] = raw["decided_counts"].astype(np.int64) / matches[:, None]
    if "stage" in raw:
        out["stage"] = raw["stage"]
    if "decided" in raw:
        out["decided"] = raw["decided"]
    if "slot_counts" in raw:
        out["best_slot_count"] = raw["slot_counts"].astype(np.int64)
        out["best_slot_proba"] = out["best_slot_count"] / n_sims
    return out


def tournament_live_result(inp, raw, return_weights: bool) -> Dict[str, np.ndarray]:
    """simulate_tournament's dict under `in_play` / `log_weights` from the raw results (device or restatement)."""
    out = tournament_result(inp, raw)
    out.update(ess=float(raw["ess"]), log_evidence=float(raw["log_evidence"]))
    for key in ("draw", "in_play_home_goals", "in_play_away_goals"):
        if key in raw:
            out[key] = raw[key]
    if return_weights:
        out["log_weights"] = raw["L"] - raw["L"].max()
    return out


def live_inputs(inp):
    """The checked inputs of a live query with the group-fixture list CONCATENATED: the fixtures still to kick off,
    then the matches in play (inp["in_play"], _tournament_in_play's columns)."""
    ip = inp["in_play"]
    return dict(inp, fix_p=np.concatenate([inp["fix_p"], ip[0]]), fix_q=np.concatenate([inp["fix_q"], ip[1]]))


def _live_keys(inp, raw, out):
    """What a live query's result gains (raw["ess"] is there exactly when the call was live)."""
    if "ess" in raw:
        out.update(ess=float(raw["ess"]), log_evidence=float(raw["log_evidence"]))
        for key in ("draw", "in_play_home_goals", "in_play_away_goals"):
            if key in raw:
                out[key] = raw[key]


def paths_result(inp, raw) -> Dict[str, np.ndarray]:
    """tournament_paths' dict from the raw integer tables and records (device or restatement); live: `inp` is
    live_inputs' and raw has "ess"."""
    n_sims, rounds, size = inp["num_simulations"], inp["rounds"], inp["group_size"]
    grouped = inp["group"] is not None
    records = {k: raw[k] for k in ("position", "group_outcome", "pair", "winner") if k in raw}
    out = tournament_result(inp, raw)
    out["targets"] = _paths.target_names(rounds)
    ps = raw["position_stage"][:, :size, :rounds + 2] if grouped else None
    out.update(_paths.from_counts(raw["stage_counts"], raw["advance"], n_sims, ps))
    if grouped:
        out["fixtures"] = np.stack([inp["fix_p"], inp["fix_q"]], axis=1).astype(np.int64)
    if "joint" in raw:
        out.update(leverage_from_counts(raw["outcome"], raw["target"], raw["joint"], n_sims))
    out.update(records)
    if "ess" in raw:
        n_live = inp["in_play"][0].size
        out["in_play"] = np.arange(inp["fix_p"].size - n_live, inp["fix_p"].size, dtype=np.int64)
        _live_keys(inp, raw, out)
    return out


def scenarios_result(inp, keys, caps, raw) -> Dict[str, np.ndarray]:
    """tournament_scenarios' dict from the raw integer tables and records (device or restatement)."""
    n_sims, rounds = inp["num_simulations"], inp["rounds"]
    first, second = inp["fix_p"][keys].astype(np.int64), inp["fix_q"][keys].astype(np.int64)
    out = {"teams": inp["teams"], "targets": np.append(_paths.target_names(rounds), "group_winner"),
           "fixtures": keys, "home": inp["teams"][first], "away": inp["teams"][second], "margin_cap": caps,
           "shape": _scenarios.scenario_shape(caps), "margins": _scenarios.scenario_margins(caps)}
    out.update(_scenarios.scenario_from_counts(raw["scenario"], raw["joint"], n_sims))
    out["round_proba"] = out["target_count"][:, :rounds + 1] / n_sims
    if "decided_counts" in raw:
        # round r has 2^(R - 1 - r) matches per simulation
        matches = n_sims * (1 << np.arange(rounds - 1, -1, -1, dtype=np.int64))
        out["decided_proba"] = raw["decided_counts"].astype(np.int64) / matches[:, None]
    if "sim_scenario" in raw:
        out["scenario"], out["target_set"] = raw["sim_scenario"], raw["sim_tset"]
    _live_keys(inp, raw, out)
    return out


def points_result(inp, raw, points_min: int, levels) -> Dict[str, np.ndarray]:
    """tournament_points' dict from the raw integer tables (device or restatement)."""
    n_sims, rounds, size, best = inp["num_simulations"], inp["rounds"], inp["group_size"], inp["best_of_rest"]
    out = {"teams": inp["teams"], "groups": np.asarray(inp["group_names"]),
           "targets": np.append(_paths.target_names(rounds), "group_winner")}
    out.update(_group_points.from_counts(
        raw["team_points"], raw["team_target"], raw["team_place"][:, :, :size], raw["place_points"][:, :size],
        raw["place_gap"][:, :size - 1], points_min, n_sims, levels, raw.get("rest_count"), raw.get("rest_through"),
        raw.get("rest_rank"), best))
    if "decided_counts" in raw:
        # round r has 2^(R - 1 - r) matches per simulation
        matches = n_sims * (1 << np.arange(rounds - 1, -1, -1, dtype=np.int64))
        out["decided_proba"] = raw["decided_counts"].astype(np.int64) / matches[:, None]
    _live_keys(inp, raw, out)
    return out
