"""bpl -- MI355X-native drop-in for anguswilliams91/bpl-next's Dixon-Coles predictors.

Same public surface as the reference's bpl/__init__.py:4-7 for the models on the hot
path; the numpyro/JAX machinery underneath is replaced by libbplhip.so (HIP, gfx950).
"""
__version__ = "0.2.0"

from bpl import diagnostics, group_points, markets, paths, periods, ratings, scenarios, sensitivity, slate
from bpl.diagnostics import mcmc_diagnostics
from bpl.dixon_coles import DixonColesMatchPredictor
from bpl.elpd import compare_elpd
from bpl.extended_dixon_coles import ExtendedDixonColesMatchPredictor
from bpl.neutral_dixon_coles import NeutralDixonColesMatchPredictor
from bpl.neutral_dixon_coles_WC import NeutralDixonColesMatchPredictorWC
from bpl.scoring import compare_scores
from bpl.sensitivity import powerscale_sensitivity

__all__ = ["DixonColesMatchPredictor", "ExtendedDixonColesMatchPredictor",
           "NeutralDixonColesMatchPredictor", "NeutralDixonColesMatchPredictorWC", "compare_elpd",
           "compare_scores", "diagnostics", "group_points", "markets", "mcmc_diagnostics", "paths", "periods", "powerscale_sensitivity", "ratings",
           "scenarios", "sensitivity", "slate"]
