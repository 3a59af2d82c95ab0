"""ctypes binding of libbplhip.so (include/bplhip.h) and a thin context wrapper.

Python holds the device buffers (torch-ROCm tensors) and passes raw device pointers
and the current HIP stream across the C-ABI.  There is NO CPU fallback: if the shared
library is missing, or there is no GPU, constructing a `HipContext` raises.
"""

from __future__ import annotations

import contextlib
import ctypes as C
import os
from typing import Optional, Sequence, Tuple

import numpy as np

MODEL_BASIC = 0
MODEL_EXTENDED = 1
MODEL_DYNAMIC = 2
MODEL_NEUTRAL = 3
# error codes of include/bplhip.h
BPLHIP_EINVAL, BPLHIP_ESTATE, BPLHIP_EHIP, BPLHIP_ENOMEM, BPLHIP_EUNSUPPORTED, BPLHIP_ENUMERIC = -1, -2, -3, -4, -5, -6
# BPLHIP_PATH_* of include/bplhip.h (HipContext.last_eval_path)
(PATH_NONE, PATH_LEAGUE, PATH_NEU_FUSED, PATH_NEU_BIG_RUNS, PATH_NEU_BIG_FIXTURE, PATH_NEU_MULTI,
 PATH_DYN_FUSED_GATHER, PATH_DYN_FUSED_ATOMICS, PATH_DYN_SLICED, PATH_DYN_MULTI) = range(10)
PATH_NAMES = ("NONE", "LEAGUE", "NEU_FUSED", "NEU_BIG_RUNS", "NEU_BIG_FIXTURE", "NEU_MULTI",
              "DYN_FUSED_GATHER", "DYN_FUSED_ATOMICS", "DYN_SLICED", "DYN_MULTI")
# BPLHIP_ENGINE_* of include/bplhip.h (HipContext.last_nuts_engine)
ENGINE_NAMES = ("NONE", "HOST_TREE", "DEVICE_TREE", "LOOP_LNE1", "LOOP_LNE2", "PERSIST_TAIL", "PERSIST_GRIDY",
                "PERSIST_VEC", "PERSIST_KP_LEAF", "PERSIST_KW_LEAF", "LOCKSTEP_VEC", "PERSIST_NEU_FUSED")
(ENGINE_NONE, ENGINE_HOST_TREE, ENGINE_DEVICE_TREE, ENGINE_LOOP_LNE1, ENGINE_LOOP_LNE2, ENGINE_PERSIST_TAIL,
 ENGINE_PERSIST_GRIDY, ENGINE_PERSIST_VEC, ENGINE_PERSIST_KP_LEAF, ENGINE_PERSIST_KW_LEAF, ENGINE_LOCKSTEP_VEC,
 ENGINE_PERSIST_NEU_FUSED) = range(len(ENGINE_NAMES))

_LIB_NAME = os.environ.get("BPLHIP_LIB", "libbplhip.so")  # override: diagnostic builds only
_lib = None

class BplHipError(RuntimeError):
    """A libbplhip call failed (code < 0); the message is bplhip_last_error()."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"libbplhip error {code}: {msg}")
        self.code = code


class NutsCfg(C.Structure):
    _fields_ = [
        ("num_warmup", C.c_int32),
        ("num_samples", C.c_int32),
        ("max_tree_depth", C.c_int32),
        ("adapt_step_size", C.c_int32),
        ("adapt_mass_matrix", C.c_int32),
        ("thinning", C.c_int32),
        ("step_size", C.c_double),
        ("target_accept_prob", C.c_double),
        ("init_radius", C.c_double),
        ("max_delta_energy", C.c_double),
    ]


class NutsStats(C.Structure):
    _fields_ = [
        ("potential_energy", C.POINTER(C.c_double)),
        ("accept_prob", C.POINTER(C.c_double)),
        ("step_size", C.POINTER(C.c_double)),
        ("num_steps", C.POINTER(C.c_int32)),
        ("diverging", C.POINTER(C.c_int32)),
        ("corr_coef", C.POINTER(C.c_double)),
        ("final_step_size", C.c_double),
        ("mean_accept_prob", C.c_double),
        ("total_leapfrogs", C.c_int64),
        ("total_divergences", C.c_int64),
        ("wall_seconds", C.c_double),
        ("inverse_mass_matrix", C.POINTER(C.c_double)),
    ]


class Fixtures(C.Structure):
    """bplhip_fixtures of include/bplhip.h: the fixture columns of one posterior query.  Build it with
    `fixtures()`, which keeps the arrays the record points into alive on the record itself."""
    _fields_ = [
        ("m", C.c_int64),
        ("venue", C.c_int32),
        ("home_idx", C.c_void_p),
        ("away_idx", C.c_void_p),
        ("home_goals", C.c_void_p),
        ("away_goals", C.c_void_p),
        ("neutral_venue", C.c_void_p),
        ("home_conf", C.c_void_p),
        ("away_conf", C.c_void_p),
    ]


def fixtures(home_idx, away_idx, home_goals=None, away_goals=None, neutral=None, conf=None) -> Fixtures:
    """The query record of m fixtures.  `neutral` (0/1 per fixture, or one value for all) selects the venue
    form, `conf` = (home, away confederation indices) goes with it; both are broadcast to [m].  The record
    holds the converted arrays in `.arrays`: they live as long as it does."""
    cols = {"home_idx": home_idx, "away_idx": away_idx, "home_goals": home_goals, "away_goals": away_goals}
    arrays = {k: np.ascontiguousarray(v, dtype=np.uint16) for k, v in cols.items() if v is not None}
    m = arrays["home_idx"].size
    if any(a.size != m for a in arrays.values()):
        raise ValueError("query arrays must have equal length")
    if neutral is not None:
        venue = {"neutral_venue": (neutral, np.uint8)}
        if conf is not None:
            venue.update(home_conf=(conf[0], np.uint16), away_conf=(conf[1], np.uint16))
        for k, (v, dt) in venue.items():
            arrays[k] = np.ascontiguousarray(np.broadcast_to(np.asarray(v), (m,)), dtype=dt)
    q = Fixtures(m=m, venue=int(neutral is not None), **{k: a.ctypes.data for k, a in arrays.items()})
    q.arrays = arrays
    return q


_vp, _i32, _i64, _u32, _f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_double
_fx = C.POINTER(Fixtures)
_nuts = [_vp, C.POINTER(NutsCfg)]
# what the season family's symbols take first (context, fixtures, table, points, n_sims, key), then simulate_season's
# outputs and stream, or the targets and chunk_sims; likewise simulate_tournament's parameters, which its forms extend
_season = [_vp, _i64, _vp, _vp, _i32] + [_vp] * 4 + [_i32, _i32, _i32, _i64, _u32, _u32]
_season_sim, _season_targets = _season + [_vp] * 8, _season + [_i32, _vp, _i64]
# the live request as the three live queries take it after pair_init: n_in_play, the five in-play columns, reweight,
# log_weights, ess, log_evidence
_live_request = [_i32] + [_vp] * 5 + [_i32] + [_vp] * 3
_tournament = ([_vp, _i32, _vp, _vp, _vp, _i32] + [_vp] * 4
               + [_i64, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _i64, _u32, _u32] + [_vp] * 4)
# every symbol include/bplhip.h declares: name -> (restype, argtypes) (checked by tests/test_abi.py without a GPU)
_SIGNATURES = {
    "bplhip_abi_version": (C.c_int, []),
    "bplhip_create": (C.c_int, [C.POINTER(_vp), C.c_int]),
    "bplhip_destroy": (None, [_vp]),
    "bplhip_last_error": (C.c_char_p, [_vp]),
    "bplhip_set_fixtures": (C.c_int, [_vp, C.c_int, _i64, _i32] + [_vp] * 6 + [_i32, _vp]),
    "bplhip_set_fixtures_dynamic": (C.c_int, [_vp, _i64, _i32, _i32] + [_vp] * 7 + [_i32, _i32, _vp]),
    "bplhip_set_fixtures_neutral": (C.c_int, [_vp, _i64, _i32] + [_vp] * 7 + [_i32, _vp, _vp, _i32, _vp]),
    "bplhip_constrain_dynamic": (C.c_int, [_vp, _vp, _i64] + [_vp] * 6),
    "bplhip_set_option": (C.c_int, [_vp, C.c_char_p, C.c_int]),
    "bplhip_latent_dim": (C.c_int, [_vp]),
    "bplhip_last_eval_path": (C.c_int, [_vp]),
    "bplhip_last_nuts_engine": (C.c_int, [_vp]),
    "bplhip_logp_grad": (C.c_int, [_vp] * 6),
    "bplhip_logp_grad_batched": (C.c_int, [_vp, _i32] + [_vp] * 5),
    "bplhip_logp_grad_graph": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp, _i32, _vp]),
    "bplhip_nuts_default_cfg": (None, [C.POINTER(NutsCfg)]),
    "bplhip_nuts_run": (C.c_int, _nuts + [_vp, _u32, _u32, _vp, C.POINTER(NutsStats), _vp]),
    "bplhip_nuts_run_chains": (C.c_int, _nuts + [_i32, _vp, _vp, _vp, C.POINTER(NutsStats), _vp]),
    "bplhip_constrain": (C.c_int, [_vp, _vp, _i64] + [_vp] * 4),
    "bplhip_predict_set_posterior": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp, _i32, _vp]),
    "bplhip_predict_set_posterior_venue": (C.c_int, [_vp, _i32, _i32] + [_vp] * 6 + [_i32, _vp, _vp]),
    "bplhip_predict_score_proba": (C.c_int, [_vp, _fx, _vp, _vp]),
    "bplhip_predict_score_grid": (C.c_int, [_vp, _fx, _i32, _vp, _vp]),
    "bplhip_predict_score_grid_f32": (C.c_int, [_vp, _fx, _i32, _vp, _vp]),
    "bplhip_simulate_season": (C.c_int, _season_sim),
    "bplhip_match_leverage": (C.c_int, _season_targets + [_vp] * 4),
    "bplhip_simulate_tournament": (C.c_int, _tournament),
    "bplhip_simulate_season_h2h": (C.c_int, _season_sim + [_vp]),
    "bplhip_simulate_season_playoff": (C.c_int, _season_sim + [_vp] + [_i32, _i32, _vp, _vp, _i32, _u32, _u32, _f64, _i32]
                                       + [_vp] * 5),
    "bplhip_simulate_season_live": (C.c_int, _season_sim + [_vp] + [_i32, _i32] + [_vp] * 5 + [_i32] + [_vp] * 6),
    "bplhip_match_leverage_h2h": (C.c_int, _season_targets + [_vp] * 5),
    "bplhip_season_points": (C.c_int, _season_targets + [_i32, _i32] + [_vp] * 6),
    "bplhip_season_scenarios": (C.c_int, _season_targets + [_i32] + [_vp] * 6),
    "bplhip_match_leverage_live": (C.c_int, _season_targets + [_vp] * 5 + _live_request),
    "bplhip_season_points_live": (C.c_int, _season_targets + [_i32, _i32] + [_vp] * 6 + _live_request),
    "bplhip_season_scenarios_live": (C.c_int, _season_targets + [_i32] + [_vp] * 6 + _live_request),
    "bplhip_season_trajectory": (C.c_int, _season_targets + [_i32, _i32] + [_i32, _vp, _vp] + [_vp] * 10),
    "bplhip_simulate_tournament_h2h": (C.c_int, _tournament + [_vp]),
    "bplhip_simulate_tournament_knockout": (C.c_int, _tournament + [_vp] + [_i32, _u32, _f64, _i32, _vp, _vp, _vp]),
    "bplhip_tournament_paths": (C.c_int, _tournament + [_vp] + [_i32, _i32, _u32, _f64, _i32, _vp, _vp, _vp]
                                + [_i64] + [_vp] * 9),
    "bplhip_tournament_scenarios": (C.c_int, _tournament[:-3] + [_vp, _i32, _i32, _u32, _f64, _i32, _vp, _vp]
                                    + [_i64, _i32] + [_vp] * 6),
    "bplhip_tournament_points": (C.c_int, _tournament[:-3] + [_vp, _i32, _i32, _u32, _f64, _i32, _vp, _vp]
                                 + [_i64, _i32, _i32, _i32] + [_vp] * 8),
    "bplhip_tournament_set_allocation": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp]),
    "bplhip_simulate_tournament_alloc": (C.c_int, _tournament + [_vp] + [_i32, _i32, _u32, _f64, _i32, _vp, _vp, _vp, _vp]),
    "bplhip_simulate_tournament_live": (C.c_int, _tournament + [_vp] + [_i32, _i32, _u32, _f64, _i32, _vp, _vp, _vp, _vp]
                                        + _live_request + [_vp] * 5),
    "bplhip_tournament_paths_live": (C.c_int, _tournament + [_vp] + [_i32, _i32, _u32, _f64, _i32, _vp, _vp, _vp]
                                     + [_i64] + [_vp] * 9 + _live_request + [_vp] * 3),
    "bplhip_tournament_scenarios_live": (C.c_int, _tournament[:-3] + [_vp, _i32, _i32, _u32, _f64, _i32, _vp, _vp]
                                         + [_i64, _i32] + [_vp] * 6 + _live_request + [_vp] * 3),
    "bplhip_tournament_points_live": (C.c_int, _tournament[:-3] + [_vp, _i32, _i32, _u32, _f64, _i32, _vp, _vp]
                                      + [_i64, _i32, _i32, _i32] + [_vp] * 8 + _live_request),
    "bplhip_loglik_matrix": (C.c_int, [_vp, _fx, _vp, _vp]),
    "bplhip_loglik_summary": (C.c_int, [_vp, _fx, _f64, _i32] + [_vp] * 7),
    "bplhip_outcome_scores": (C.c_int, [_vp, _fx, _i32, _vp, _vp, _vp]),
    "bplhip_loo_scores": (C.c_int, [_vp, _fx, _f64, _i32] + [_vp] * 8),
    "bplhip_block_loglik": (C.c_int, [_vp, _fx, _vp, _i32, _vp, _vp]),
    "bplhip_psis_weights": (C.c_int, [_vp, _i32, _i32, _vp, _f64] + [_vp] * 5),
    "bplhip_weighted_scores": (C.c_int, [_vp, _fx, _vp, _i32, _vp, _i32, _vp, _vp, _vp]),
    "bplhip_market_summary": (C.c_int, [_vp, _fx, _i32, _i32, _vp, _i32] + [_vp] * 5 + [_i64, _vp]),
    "bplhip_slate_summary": (C.c_int, [_vp, _fx, _i32, _i32, _vp, _i32, _vp, _vp, _i32] + [_vp] * 6 + [_i64, _vp]),
    "bplhip_team_ratings": (C.c_int, [_vp, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _vp, _i32, _i32] + [_vp] * 8
                            + [_i64, _vp]),
    "bplhip_inplay_summary": (C.c_int, [_vp, _fx, _vp, _i32, _i32, _vp, _i32, _vp, _i32] + [_vp] * 8 + [_i64, _vp]),
    "bplhip_period_summary": (C.c_int, [_vp, _fx, _vp, _i32, _i32, _vp, _i32] + [_vp] * 5 + [_i64, _vp]),
    "bplhip_mcmc_diagnostics": (C.c_int, [_vp, _i32, _i32, _i64, _vp, _i32, _vp, _i64] + [_vp] * 8),
    "bplhip_weighted_shift": (C.c_int, [_vp, _i32, _i64, _vp, _i32, _vp, _f64, _i64] + [_vp] * 8),
    "bplhip_ppc": (C.c_int, [_vp, _fx, _vp, _vp, _vp, _i32, _i32, _i64, _u32, _u32] + [_vp] * 7),
    "bplhip_selftest_math": (C.c_int, [_vp, _i32, _i64, _vp, _vp]),
    "bplhip_selftest_lanes": (C.c_int, [_vp, _i32, _i32] + [_vp] * 6),
    "bplhip_threefry_split": (None, [_u32, _u32, _i32, C.POINTER(_u32)]),
    "bplhip_threefry_bits": (None, [_u32, _u32, _i32, C.POINTER(_u32)]),
}
ABI_SYMBOLS = tuple(_SIGNATURES)
# bplhip_selftest_lanes (include/bplhip.h): channels per wave and type, the counted-row probe, its words per row
SELFTEST_CHANNELS, SELFTEST_COUNTED_ROWS, SELFTEST_GA_WORDS = 16, 29, 32
ABI_VERSION = 2
# bplhip_season_scenarios (include/bplhip.h BPLHIP_SCENARIO_*): key fixtures, margin cap, scenarios
SCENARIO_MAX_KEYS, SCENARIO_MAX_CAP, SCENARIO_MAX_CELLS = 8, 3, 6561
# bplhip_tournament_points (include/bplhip.h BPLHIP_GROUP_POINTS_*): points bins, goal-difference cap
GROUP_POINTS_MAX_BINS, GROUP_POINTS_MAX_GD_CAP = 256, 8


def lib_path() -> str:
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), _LIB_NAME)


def load_library():
    """dlopen libbplhip.so (built in-tree by `make -C bpl-next_amd/csrc`)."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C bpl-next_amd/csrc)"
        )
    lib = C.CDLL(path)
    for name, (restype, argtypes) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.bplhip_abi_version() != ABI_VERSION:
        raise ImportError(f"{path}: ABI version {lib.bplhip_abi_version()} != {ABI_VERSION}")
    _lib = lib
    return lib


def default_nuts_cfg() -> NutsCfg:
    cfg = NutsCfg()
    load_library().bplhip_nuts_default_cfg(C.byref(cfg))
    return cfg


def prng_key(seed: int) -> Tuple[int, int]:
    """jax.random.PRNGKey(seed) -> (hi, lo)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return (seed >> 32) & 0xFFFFFFFF, seed & 0xFFFFFFFF


def threefry_split(key: Tuple[int, int], n: int):
    """jax.random.split(key, n) -> list of (hi, lo)."""
    out = (C.c_uint32 * (2 * n))()
    load_library().bplhip_threefry_split(key[0], key[1], n, out)
    return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n)]


def threefry_bits(key: Tuple[int, int], n: int) -> np.ndarray:
    out = (C.c_uint32 * n)()
    load_library().bplhip_threefry_bits(key[0], key[1], n, out)
    return np.frombuffer(out, dtype=np.uint32).copy()


def _np_ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class HipContext:
    """One libbplhip context on one GPU.  All tensors are torch CUDA(=HIP) tensors."""

    def __init__(self, device_index: int = 0):
        import torch

        self._torch = torch
        self._lib = load_library()
        if not torch.cuda.is_available():
            raise RuntimeError(
                "bpl (MI355X build) needs a HIP GPU: torch.cuda.is_available() is False "
                "and there is no CPU fallback"
            )
        self.device = torch.device("cuda", device_index)
        h = C.c_void_p()
        rc = self._lib.bplhip_create(C.byref(h), device_index)
        if rc != 0:
            raise BplHipError(rc, self._lib.bplhip_last_error(None).decode())
        self._h = h
        self.dim = 0
        self.n_teams = 0
        self.model = None

    # -- plumbing
    def close(self):
        if getattr(self, "_h", None):
            self._lib.bplhip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # pylint: disable=broad-except
            pass

    def _check(self, rc: int):
        if rc != 0:
            raise BplHipError(rc, self._lib.bplhip_last_error(self._h).decode())

    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def set_option(self, name: str, value: int):
        self._check(self._lib.bplhip_set_option(self._h, name.encode(), int(value)))

    def last_eval_path(self) -> int:
        """PATH_* of the evaluation enqueued last (host bookkeeping: no synchronisation)."""
        return int(self._lib.bplhip_last_eval_path(self._h))

    def last_nuts_engine(self) -> int:
        """ENGINE_* of the sampler run dispatched last (host bookkeeping: no synchronisation)."""
        return int(self._lib.bplhip_last_nuts_engine(self._h))

    # -- model arguments
    def _dev(self, a, np_dtype):
        """A fixture array on this device: a numpy array (or anything np.asarray takes) is cast and
        uploaded, uint16 as int16 bit patterns; a torch tensor must already be what the upload gives."""
        torch = self._torch
        t_dtype = {np.uint16: torch.int16, np.uint8: torch.uint8, np.float32: torch.float32}[np_dtype]
        if isinstance(a, torch.Tensor):
            if a.dtype != t_dtype or a.device != self.device or not a.is_contiguous():
                raise ValueError(f"tensor must be contiguous {t_dtype} on {self.device}")
            return a
        arr = np.ascontiguousarray(np.asarray(a).astype(np_dtype))
        return torch.from_numpy(arr.view(np.int16) if np_dtype == np.uint16 else arr).to(self.device)

    def set_fixtures(
        self,
        model: int,
        home_idx,
        away_idx,
        home_goals,
        away_goals,
        n_teams: int,
        weights=None,
        covariates_std: Optional[np.ndarray] = None,
    ):
        """Bind fixtures.  Index/goal arrays: torch tensors on this device (uint16 is
        stored as int16 bit patterns / uint8) or numpy arrays (uploaded here)."""
        h, a = self._dev(home_idx, np.uint16), self._dev(away_idx, np.uint16)
        x, y = self._dev(home_goals, np.uint8), self._dev(away_goals, np.uint8)
        n = h.numel()
        if not (a.numel() == x.numel() == y.numel() == n):
            raise ValueError("fixture arrays must have equal length")
        w = None
        if weights is not None:
            w = self._dev(weights, np.float32)
            if w.numel() != n:
                raise ValueError("weights must have one entry per fixture")
        cov = None
        k = 0
        if covariates_std is not None:
            cov = np.ascontiguousarray(covariates_std, dtype=np.float64)
            if cov.ndim != 2 or cov.shape[0] != n_teams:
                raise ValueError("covariates must be [n_teams, k]")
            k = cov.shape[1]
        with self._torch.cuda.device(self.device):
            self._check(
                self._lib.bplhip_set_fixtures(
                    self._h, model, n, n_teams,
                    h.data_ptr(), a.data_ptr(), x.data_ptr(), y.data_ptr(),
                    None if w is None else w.data_ptr(), _np_ptr(cov), k, self._stream(),
                )
            )
        self.dim = self._lib.bplhip_latent_dim(self._h)
        self.n_teams = n_teams
        self.model = model
        self.n = n
        return self

    def set_fixtures_dynamic(self, home_idx, away_idx, home_goals, away_goals, gameweek,
                             neutral_venue, n_teams: int, n_gameweeks: int,
                             covariates_std: Optional[np.ndarray] = None, random_walk: bool = True):
        """Bind the dynamic (time-varying) model (bpl/dynamic_dixon_coles.py)."""
        dev, torch = self._dev, self._torch
        h, a, g = dev(home_idx, np.uint16), dev(away_idx, np.uint16), dev(gameweek, np.uint16)
        x, y, nv = dev(home_goals, np.uint8), dev(away_goals, np.uint8), dev(neutral_venue, np.uint8)
        n = h.numel()
        if not (a.numel() == g.numel() == x.numel() == y.numel() == nv.numel() == n):
            raise ValueError("fixture arrays must have equal length")
        cov, k = None, 0
        if covariates_std is not None:
            cov = np.ascontiguousarray(covariates_std, dtype=np.float64)
            k = cov.shape[1]
        with torch.cuda.device(self.device):
            self._check(self._lib.bplhip_set_fixtures_dynamic(
                self._h, n, n_teams, n_gameweeks, h.data_ptr(), a.data_ptr(), x.data_ptr(),
                y.data_ptr(), g.data_ptr(), nv.data_ptr(), _np_ptr(cov), k, int(random_walk),
                self._stream()))
        self.dim = self._lib.bplhip_latent_dim(self._h)
        self.n_teams, self.n_gameweeks, self.model, self.n = n_teams, n_gameweeks, MODEL_DYNAMIC, n
        return self

    def set_fixtures_neutral(self, home_idx, away_idx, home_goals, away_goals, neutral_venue,
                             n_teams: int, weights=None, covariates_std: Optional[np.ndarray] = None,
                             home_conf=None, away_conf=None, n_conf: int = 0):
        """Bind the neutral-venue model (bpl/neutral_dixon_coles.py).  `weights`: the final
        per-fixture weights (time decay x game weights) or None.  `home_conf`, `away_conf`,
        `n_conf`: confederation indices of the World-Cup variant."""
        dev, torch = self._dev, self._torch
        h, a = dev(home_idx, np.uint16), dev(away_idx, np.uint16)
        x, y, nv = dev(home_goals, np.uint8), dev(away_goals, np.uint8), dev(neutral_venue, np.uint8)
        n = h.numel()
        if not (a.numel() == x.numel() == y.numel() == nv.numel() == n):
            raise ValueError("fixture arrays must have equal length")
        w = None
        if weights is not None:
            w = dev(weights, np.float32)
            if w.numel() != n:
                raise ValueError("weights must have one entry per fixture")
        cov, k = None, 0
        if covariates_std is not None:
            cov = np.ascontiguousarray(covariates_std, dtype=np.float64)
            k = cov.shape[1]
        hc = ac = None
        if n_conf:
            hc, ac = dev(home_conf, np.uint8), dev(away_conf, np.uint8)
            if hc.numel() != n or ac.numel() != n:
                raise ValueError("confederation arrays must have one entry per fixture")
        with torch.cuda.device(self.device):
            self._check(self._lib.bplhip_set_fixtures_neutral(
                self._h, n, n_teams, h.data_ptr(), a.data_ptr(), x.data_ptr(), y.data_ptr(),
                nv.data_ptr(), None if hc is None else hc.data_ptr(),
                None if ac is None else ac.data_ptr(), int(n_conf),
                None if w is None else w.data_ptr(), _np_ptr(cov), k, self._stream()))
        self.dim = self._lib.bplhip_latent_dim(self._h)
        self.n_teams, self.model, self.n = n_teams, MODEL_NEUTRAL, n
        return self

    def constrain_dynamic(self, z_draws: np.ndarray):
        z = np.ascontiguousarray(z_draws, dtype=np.float64)
        s, g, t = z.shape[0], self.n_gameweeks, self.n_teams
        names = ("attack", "defence", "home_attack", "away_attack", "home_defence", "away_defence")
        out = {nm: np.empty((s, g, t)) for nm in names}
        self._check(self._lib.bplhip_constrain_dynamic(self._h, _np_ptr(z), s,
                                                       *[_np_ptr(out[nm]) for nm in names]))
        return out

    # -- the hot path
    def logp_grad(self, z, potential=None, grad=None, aux=None):
        """U(z), dU/dz for z [D] or [C, D] (float64 tensors on this device)."""
        torch = self._torch
        if z.dtype != torch.float64 or not z.is_contiguous() or z.device != self.device:
            raise ValueError("z must be a contiguous float64 tensor on the context device")
        batched = z.dim() == 2
        c = z.shape[0] if batched else 1
        if z.shape[-1] != self.dim:
            raise ValueError(f"z has {z.shape[-1]} columns, model has D={self.dim}")
        if potential is None:
            potential = torch.empty(c, dtype=torch.float64, device=self.device)
        if grad is None:
            grad = torch.empty_like(z)
        if aux is None:
            aux = torch.empty((c, 4), dtype=torch.float64, device=self.device)
        self._check(
            self._lib.bplhip_logp_grad_batched(
                self._h, c, z.data_ptr(), potential.data_ptr(), grad.data_ptr(),
                aux.data_ptr(), self._stream(),
            )
        )
        return potential, grad, aux

    def logp_grad_graph(self, count: int, z, potential, grad, replays: int = 1):
        """Replay a captured chain of `count` evaluations over the rows of z [n_z, D]."""
        self._check(
            self._lib.bplhip_logp_grad_graph(
                self._h, count, z.shape[0], z.data_ptr(), potential.data_ptr(),
                grad.data_ptr(), replays, self._stream(),
            )
        )

    def graph_replayer(self, count: int, z, potential, grad):
        """`logp_grad_graph` with its arguments marshalled once: returns `replay(replays=1)` for the
        current stream (the per-call Python cost -- stream lookup, three data_ptr(), argument
        conversion -- is ~5 us, which a caller replaying short graphs back to back can skip)."""
        fn, check = self._lib.bplhip_logp_grad_graph, self._check
        args = (self._h, C.c_int32(count), C.c_int32(z.shape[0]), C.c_void_p(z.data_ptr()),
                C.c_void_p(potential.data_ptr()), C.c_void_p(grad.data_ptr()))
        stream = self._stream()
        keep = (z, potential, grad)

        def replay(replays: int = 1, _keep=keep):
            check(fn(*args, replays, stream))

        return replay

    # -- predict path on the device
    def predict_set_posterior(self, attack, defence, home_advantage, corr_coef):
        att = np.ascontiguousarray(attack, dtype=np.float64)
        dfn = np.ascontiguousarray(defence, dtype=np.float64)
        ha = np.ascontiguousarray(home_advantage, dtype=np.float64)
        cc = np.ascontiguousarray(corr_coef, dtype=np.float64)
        s, t = att.shape
        if dfn.shape != (s, t) or cc.shape != (s,) or ha.shape not in ((s,), (s, t)):
            raise ValueError("posterior arrays have inconsistent shapes")
        with self._torch.cuda.device(self.device):
            self._check(self._lib.bplhip_predict_set_posterior(
                self._h, s, t, _np_ptr(att), _np_ptr(dfn), _np_ptr(ha), int(ha.ndim == 2), _np_ptr(cc)))
        self.pred_draws = s

    def predict_set_posterior_venue(self, attack, defence, home_attack, away_attack, home_defence,
                                    away_defence, corr_coef, confederation_strength=None):
        """Posterior of the neutral-venue family (six [draws, teams] tables, optional
        [draws, confederations] strengths); queries then take `neutral` (and `conf`)."""
        tabs = [np.ascontiguousarray(t, dtype=np.float64)
                for t in (attack, defence, home_attack, away_attack, home_defence, away_defence)]
        cc = np.ascontiguousarray(corr_coef, dtype=np.float64)
        s, t = tabs[0].shape
        if any(x.shape != (s, t) for x in tabs) or cc.shape != (s,):
            raise ValueError("posterior arrays have inconsistent shapes")
        conf = None
        if confederation_strength is not None:
            conf = np.ascontiguousarray(confederation_strength, dtype=np.float64)
            if conf.ndim != 2 or conf.shape[0] != s:
                raise ValueError("confederation_strength must be [draws, confederations]")
        with self._torch.cuda.device(self.device):
            self._check(self._lib.bplhip_predict_set_posterior_venue(
                self._h, s, t, *(_np_ptr(x) for x in tabs), 0 if conf is None else conf.shape[1],
                None if conf is None else _np_ptr(conf), _np_ptr(cc)))
        self.pred_draws = s

    def predict_score_proba(self, home_idx, away_idx, home_goals, away_goals, neutral=None,
                            conf=None) -> np.ndarray:
        """Mean over the draws of tau * Poisson * Poisson per query.  `neutral` (0/1 per query) and
        `conf` = (home, away confederation indices) select the venue-aware rates and must be given
        exactly when the posterior was set with predict_set_posterior_venue."""
        q = fixtures(home_idx, away_idx, home_goals, away_goals, neutral, conf)
        out = np.empty(q.m, dtype=np.float64)
        with self._torch.cuda.device(self.device):
            self._check(self._lib.bplhip_predict_score_proba(self._h, C.byref(q), _np_ptr(out), self._stream()))
        return out

    def predict_score_grid(self, home_idx, away_idx, max_goals: int, neutral=None, conf=None,
                           dtype=np.float64) -> np.ndarray:
        """[m, max_goals+1, max_goals+1] scoreline probabilities of the m fixtures; dtype float64 (default) or
        float32 (the reference's own: half the bytes over PCIe)."""
        q = fixtures(home_idx, away_idx, neutral=neutral, conf=conf)
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise ValueError("predict_score_grid: dtype is float64 or float32")
        fn = self._lib.bplhip_predict_score_grid_f32 if dtype == np.float32 else self._lib.bplhip_predict_score_grid
        g1 = int(max_goals) + 1
        out = np.empty((q.m, g1, g1), dtype=dtype)
        with self._torch.cuda.device(self.device):
            self._check(fn(self._h, C.byref(q), int(max_goals), _np_ptr(out), self._stream()))
        return out

    @staticmethod
    def _pair_init(pair_init, n: int, zeros: bool = False):
        """pair_init as the head-to-head entry points take it: contiguous u32 [n, n], or None (all zero).  zeros:
        for an entry point that reads a non-null pair_init as the request for the head-to-head order, None becomes
        the all-zero matrix (no matches played)."""
        if pair_init is None:
            return np.zeros((n, n), dtype=np.uint32) if zeros else None
        pair = np.ascontiguousarray(pair_init, dtype=np.uint32)
        if pair.shape != (n, n):
            raise ValueError(f"pair_init must be [{n}, {n}], not {list(pair.shape)}")
        return pair

    def _season_head(self, home_idx, away_idx, table_idx, table, points, n_sims: int, key: Tuple[int, int]):
        """What every entry point of the season family takes first.  Returns (n, nf, head, keep): the table's and the
        fixtures' sizes, the arguments from the context to key_lo, and the converted arrays `head` points into, which
        the caller holds until its call has returned."""
        h = np.ascontiguousarray(home_idx, dtype=np.uint16)
        a = np.ascontiguousarray(away_idx, dtype=np.uint16)
        ti = np.ascontiguousarray(table_idx, dtype=np.uint16)
        tab = np.asarray(table, dtype=np.int64).reshape(ti.size, 3)
        keep = [h, a, ti] + [np.ascontiguousarray(tab[:, i], dtype=np.int32) for i in range(3)]
        if h.size != a.size:
            raise ValueError("home and away index arrays must have equal length")
        win, draw, loss = (int(p) for p in points)
        head = (self._h, h.size, _np_ptr(h), _np_ptr(a), ti.size, *(_np_ptr(x) for x in keep[2:]),
                win, draw, loss, int(n_sims), int(key[0]), int(key[1]))
        return ti.size, h.size, head, keep

    @staticmethod
    def _target_masks(target_masks) -> np.ndarray:
        """One u64 per target, bit p = finishing position p."""
        return np.array([int(m) for m in target_masks], dtype=np.uint64)

    def simulate_season(self, home_idx, away_idx, table_idx, table, points, n_sims: int, key: Tuple[int, int],
                        return_tables: bool = False, return_scores: bool = False, pair_init=None,
                        head_to_head: bool = False, playoff=None) -> dict:
        """The rest of a season, n_sims times, jointly over the posterior (csrc/dc_season.hip.h).
        home_idx / away_idx: the fixtures' model indices; table_idx: the table's model indices (slot
        order); table: [n, 3] current (points, goals for, goals against); points: (win, draw, loss);
        key: the threefry key (hi, lo).  Returns the raw integer results: "counts" u64 [n, n]
        (slot, position), "points_sum" / "gd_sum" i64 [n], and when asked "points" i32 / "position"
        u8 [n_sims, n], "home_goals" / "away_goals" u8 [n_sims, fixtures].  head_to_head: the table is
        ordered by the head-to-head rule (csrc/dc_h2h.hip.h, bplhip_simulate_season_h2h) on top of
        pair_init u32 [n, n] (points << 16 | goals of row against column; None: zero); without it pair_init is
        not read and the call is bplhip_simulate_season's.  playoff: None, or a bracket played after the table
        (bplhip_simulate_season_playoff, csrc/dc_playoff.hip.h) as a dict with "guests" (model indices outside
        the table), "bracket" (u16 codes: a position, PLAYOFF_GUEST | i, PLAYOFF_BYE), "legs_mask",
        "neutral_mask", "scale", "away_goals" and "strength" (f64 per slot, table rows then guests, or None); it
        adds "stage_counts" u64 [n + guests, R + 2], "decided_counts" u64 [R, 4] and, with return_tables,
        "playoff_stage" u8 [n_sims, n + guests] and "playoff_decided" u8 [n_sims, 2^R - 1]."""
        n, nf, head, _keep = self._season_head(home_idx, away_idx, table_idx, table, points, n_sims, key)
        n_sims = int(n_sims)
        out = {"counts": np.zeros((n, n), dtype=np.uint64), "points_sum": np.zeros(n, dtype=np.int64),
               "gd_sum": np.zeros(n, dtype=np.int64)}
        if return_tables:
            out["points"] = np.empty((n_sims, n), dtype=np.int32)
            out["position"] = np.empty((n_sims, n), dtype=np.uint8)
        if return_scores:
            out["home_goals"] = np.empty((n_sims, nf), dtype=np.uint8)
            out["away_goals"] = np.empty((n_sims, nf), dtype=np.uint8)
        pair = self._pair_init(pair_init, n) if head_to_head else None
        fn = self._lib.bplhip_simulate_season_h2h if head_to_head else self._lib.bplhip_simulate_season
        tail = (_np_ptr(pair),) if head_to_head else ()
        if playoff is not None:
            guests = np.ascontiguousarray(playoff.get("guests", ()), dtype=np.uint16)
            br = np.ascontiguousarray(playoff["bracket"], dtype=np.uint16)
            rounds = max(int(br.size).bit_length() - 1, 0)
            if br.size != 1 << rounds:
                raise ValueError("the bracket must have 2**R entries")
            nt = n + guests.size
            strength = playoff.get("strength")
            if strength is not None:
                strength = np.ascontiguousarray(strength, dtype=np.float64)
                if strength.shape != (nt,):
                    raise ValueError("strength must have one entry per slot")
            out["stage_counts"] = np.zeros((nt, rounds + 2), dtype=np.uint64)
            out["decided_counts"] = np.zeros((rounds, 4), dtype=np.uint64)
            if return_tables:
                out["playoff_stage"] = np.empty((n_sims, nt), dtype=np.uint8)
                out["playoff_decided"] = np.empty((n_sims, max(br.size - 1, 0)), dtype=np.uint8)
            fn = self._lib.bplhip_simulate_season_playoff
            tail = (_np_ptr(pair), int(bool(head_to_head)), guests.size, _np_ptr(guests) if guests.size else None,
                    _np_ptr(br), rounds, int(playoff["legs_mask"]), int(playoff["neutral_mask"]),
                    float(playoff["scale"]), int(playoff["away_goals"]), _np_ptr(strength),
                    _np_ptr(out["stage_counts"]), _np_ptr(out["decided_counts"]), _np_ptr(out.get("playoff_stage")),
                    _np_ptr(out.get("playoff_decided")))
        with self._torch.cuda.device(self.device):
            self._check(fn(
                *head, _np_ptr(out["counts"]), _np_ptr(out["points_sum"]), _np_ptr(out["gd_sum"]),
                _np_ptr(out.get("points")), _np_ptr(out.get("position")),
                _np_ptr(out.get("home_goals")), _np_ptr(out.get("away_goals")), self._stream(), *tail))
        return out

    def simulate_season_live(self, home_idx, away_idx, table_idx, table, points, n_sims: int, key: Tuple[int, int],
                             in_play=None, reweight: bool = True, log_weights=None, return_tables: bool = False,
                             return_scores: bool = False, return_weights: bool = False, pair_init=None,
                             head_to_head: bool = False) -> dict:
        """`simulate_season` with matches in progress and weighted draws (csrc/dc_live.hip.h,
        bplhip_simulate_season_live).  The arguments up to `key`, return_tables, return_scores, pair_init and
        head_to_head are simulate_season's.  in_play: None, or (home model indices, away model indices, home goals,
        away goals, elapsed) of the L matches in progress; log_weights: None or f64 [draws].  Returns
        simulate_season's raw results with "home_goals" / "away_goals" u8 [n_sims, fixtures] for the fixtures still to
        kick off, plus "ess" and "log_evidence" (floats), with return_tables "draw" i32 [n_sims], with return_scores
        "in_play_home_goals" / "in_play_away_goals" u8 [n_sims, L] (final scores), and with return_weights "L" and
        "L0" f64 [draws]: the draws' log weights and the states' log likelihood per draw."""
        n, nf, head, _keep = self._season_head(home_idx, away_idx, table_idx, table, points, n_sims, key)
        live = self._live_request(in_play, reweight, log_weights)
        n_live, tail, n_sims = live[0], live[1], int(n_sims)
        out = {"counts": np.zeros((n, n), dtype=np.uint64), "points_sum": np.zeros(n, dtype=np.int64),
               "gd_sum": np.zeros(n, dtype=np.int64)}
        if return_tables:
            out["points"] = np.empty((n_sims, n), dtype=np.int32)
            out["position"] = np.empty((n_sims, n), dtype=np.uint8)
            out["draw"] = np.empty(n_sims, dtype=np.int32)
        scores = [np.empty((n_sims, nf + n_live), dtype=np.uint8) for _ in range(2)] if return_scores else [None, None]
        self._draw_weight_outputs(out, return_weights)
        pair = self._pair_init(pair_init, n) if head_to_head else None
        with self._torch.cuda.device(self.device):
            self._check(self._lib.bplhip_simulate_season_live(
                *head, _np_ptr(out["counts"]), _np_ptr(out["points_sum"]), _np_ptr(out["gd_sum"]),
                _np_ptr(out.get("points")), _np_ptr(out.get("position")), _np_ptr(scores[0]), _np_ptr(scores[1]),
                self._stream(), _np_ptr(pair), int(bool(head_to_head)), *tail, _np_ptr(out.get("draw")),
                _np_ptr(out.get("L")), _np_ptr(out.get("L0"))))
        self._live_figures(out, live)
        if return_scores:
            out["home_goals"], out["away_goals"] = (v[:, :nf] for v in scores)
            out["in_play_home_goals"], out["in_play_away_goals"] = (v[:, nf:] for v in scores)
        return out

    def match_leverage(self, home_idx, away_idx, table_idx, table, points, n_sims: int, key: Tuple[int, int],
                       target_masks, chunk_sims: int = 0, pair_init=None, head_to_head: bool = False, live=None) -> dict:
        """simulate_season's simulations cross-tabulated on the device (csrc/dc_leverage.hip.h): the
        arguments up to `key` are simulate_season's; target_masks: one integer per target, bit p =
        finishing position p; chunk_sims: simulations per pass through the device workspace (0 = the
        library's choice; the results do not depend on it).  Returns the raw counts, o = 0 home win,
        1 draw, 2 away win: "outcome" u64 [fixtures, 3], "target" u64 [n, K], "joint" u64
        [fixtures, 3, n, K].  pair_init / head_to_head: as for simulate_season (bplhip_match_leverage_h2h).
        live: None (this entry), or `_live_request`'s result (match_leverage_live: the fixture axis is then the
        concatenated list)."""
        n, nf, head, _keep = self._season_head(home_idx, away_idx, table_idx, table, points, n_sims, key)
        masks = self._target_masks(target_masks)
        k, rows = masks.size, nf + (0 if live is None else live[0])
        out = {"outcome": np.zeros((rows, 3), dtype=np.uint64), "target": np.zeros((n, k), dtype=np.uint64),
               "joint": np.zeros((rows, 3, n, k), dtype=np.uint64)}
        if live is None:
            pair = self._pair_init(pair_init, n) if head_to_head else None
            fn = self._lib.bplhip_match_leverage_h2h if head_to_head else self._lib.bplhip_match_leverage
            tail = (_np_ptr(pair),) if head_to_head else ()
        else:
            # (the entry point reads a non-null pair_init as the head-to-head order)
            pair = self._pair_init(pair_init, n, zeros=True) if head_to_head else None
            fn, tail = self._lib.bplhip_match_leverage_live, (_np_ptr(pair), *live[1])
        with self._torch.cuda.device(self.device):
            self._check(fn(
                *head, k, _np_ptr(masks), int(chunk_sims), _np_ptr(out["outcome"]), _np_ptr(out["target"]),
                _np_ptr(out["joint"]), self._stream(), *tail))
        return self._live_figures(out, live)

    def season_points(self, home_idx, away_idx, table_idx, table, points, n_sims: int, key: Tuple[int, int],
                      target_masks, points_min: int, n_bins: int, chunk_sims: int = 0, pair_init=None,
                      head_to_head: bool = False, live=None) -> dict:
        """simulate_season's simulations, their points totals cross-tabulated on the device (csrc/dc_points.hip.h,
        bplhip_season_points): the arguments up to `target_masks` and chunk_sims, pair_init and head_to_head are
        match_leverage's; points_min, n_bins: the points axis, bin b = points_min + b points (the library refuses
        an axis a simulated total could leave).  Returns the raw counts: "team_points" u64 [n, n_bins],
        "team_target" u64 [n, n_bins, K], "position_points" u64 [n, n_bins], "gap" u64 [n - 1, n_bins].  live: as in
        match_leverage (season_points_live)."""
        n, nf, head, _keep = self._season_head(home_idx, away_idx, table_idx, table, points, n_sims, key)
        masks = self._target_masks(target_masks)
        k, p = masks.size, max(int(n_bins), 0)
        out = {"team_points": np.zeros((n, p), dtype=np.uint64), "team_target": np.zeros((n, p, k), dtype=np.uint64),
               "position_points": np.zeros((n, p), dtype=np.uint64),
               "gap": np.zeros((max(n - 1, 0), p), dtype=np.uint64)}
        # (the entry point reads a non-null pair_init as the head-to-head order)
        pair = self._pair_init(pair_init, n, zeros=True) if head_to_head else None
        fn, tail = self._lib.bplhip_season_points, ()
        if live is not None:
            fn, tail = self._lib.bplhip_season_points_live, live[1]
        with self._torch.cuda.device(self.device):
            self._check(fn(
                *head, k, _np_ptr(masks), int(chunk_sims), int(points_min), int(n_bins),
                _np_ptr(out["team_points"]), _np_ptr(out["team_target"]),
                _np_ptr(out["position_points"]), _np_ptr(out["gap"]) if n > 1 else None, self._stream(),
                _np_ptr(pair), *tail))
        return self._live_figures(out, live)

    @staticmethod
    def _scenario_keys(key_fixture, key_cap):
        """The scenario keys as the entry points take them, i32 [k] each, and the number of scenarios they span (1
        outside the library's range: it refuses the call before it writes an output)."""
        kf = np.ascontiguousarray(key_fixture, dtype=np.int32)
        kc = np.ascontiguousarray(key_cap, dtype=np.int32)
        if kf.ndim != 1 or kf.shape != kc.shape:
            raise ValueError("key_fixture and key_cap must be one-dimensional and of equal length")
        cells = 1
        for cap in kc.tolist():
            cells *= 2 * cap + 1
        return kf, kc, cells if 1 <= cells <= SCENARIO_MAX_CELLS else 1

    def season_scenarios(self, home_idx, away_idx, table_idx, table, points, n_sims: int, key: Tuple[int, int],
                         target_masks, key_fixture, key_cap, chunk_sims: int = 0, pair_init=None,
                         head_to_head: bool = False, live=None) -> dict:
        """simulate_season's simulations, the joint class of the key fixtures cross-tabulated against the targets on
        the device (csrc/dc_scenario.hip.h, bplhip_season_scenarios): the arguments up to `target_masks` and
        chunk_sims, pair_init and head_to_head are season_points'; key_fixture [k]: the key fixtures' positions in
        the fixture list; key_cap [k]: their margin caps c, 2 c + 1 classes each (class = c - clipped margin).  A
        scenario is one class per key, row-major in the order given, M = the product of the class counts (the
        library refuses more than SCENARIO_MAX_CELLS).  Returns the raw counts: "scenario" u64 [M], "joint" u64
        [M, n, K].  live: as in match_leverage (season_scenarios_live: the keys index the concatenated list)."""
        n, nf, head, _keep = self._season_head(home_idx, away_idx, table_idx, table, points, n_sims, key)
        masks = self._target_masks(target_masks)
        kf, kc, cells = self._scenario_keys(key_fixture, key_cap)
        k = masks.size
        out = {"scenario": np.zeros(cells, dtype=np.uint64), "joint": np.zeros((cells, n, k), dtype=np.uint64)}
        # (the entry point reads a non-null pair_init as the head-to-head order)
        pair = self._pair_init(pair_init, n, zeros=True) if head_to_head else None
        fn, tail = self._lib.bplhip_season_scenarios, ()
        if live is not None:
            fn, tail = self._lib.bplhip_season_scenarios_live, live[1]
        with self._torch.cuda.device(self.device):
            self._check(fn(
                *head, k, _np_ptr(masks), int(chunk_sims), kf.size, _np_ptr(kf), _np_ptr(kc),
                _np_ptr(out["scenario"]), _np_ptr(out["joint"]), self._stream(), _np_ptr(pair), *tail))
        return self._live_figures(out, live)

    def _live_request(self, in_play, reweight, log_weights, sides=np.uint16):
        """The live request as the live entry points take it (simulate_season_live after head_to_head, the three
        live queries after pair_init, simulate_tournament_live after slot_counts and the three live tournament
        queries after their kick-off lists with `sides` = np.uint8: their two sides are slots).  Returns (L, tail, ess, log_evidence,
        keep): the number of matches in play, the arguments from n_in_play to log_evidence, the two c_double the
        library writes, and the converted arrays `tail` points into, which the caller holds until its call has
        returned."""
        if in_play is None:
            in_play = ((), (), (), (), ())
        ih, ia = (np.ascontiguousarray(v, dtype=sides) for v in in_play[:2])
        ix, iy = (np.ascontiguousarray(v, dtype=np.uint8) for v in in_play[2:4])
        it = np.ascontiguousarray(in_play[4], dtype=np.float64)
        if not ih.size == ia.size == ix.size == iy.size == it.size:
            raise ValueError("the in-play columns must have equal length")
        lw = None if log_weights is None else np.ascontiguousarray(log_weights, dtype=np.float64)
        draws = int(getattr(self, "pred_draws", 0))
        if lw is not None and draws and lw.shape != (draws,):
            raise ValueError(f"log_weights must have shape ({draws},), one value per posterior draw")
        ess, logev = C.c_double(0.0), C.c_double(0.0)
        tail = (ih.size, _np_ptr(ih), _np_ptr(ia), _np_ptr(ix), _np_ptr(iy), _np_ptr(it), int(bool(reweight)),
                _np_ptr(lw), C.cast(C.pointer(ess), C.c_void_p), C.cast(C.pointer(logev), C.c_void_p))
        return ih.size, tail, ess, logev, (ih, ia, ix, iy, it, lw)

    @staticmethod
    def _live_figures(out: dict, live) -> dict:
        """`out` with "ess" and "log_evidence" as the library wrote them into the two c_double of `live`
        (`_live_request`'s result); unchanged for a kick-off call (live None)."""
        if live is not None:
            out["ess"], out["log_evidence"] = float(live[2].value), float(live[3].value)
        return out

    def _draw_weight_outputs(self, out: dict, return_weights: bool) -> None:
        """What return_weights adds to a live simulator's outputs: "L" and "L0" f64 [draws]."""
        if not return_weights:
            return
        draws = int(getattr(self, "pred_draws", 0))
        if not draws:
            raise ValueError("return_weights needs a posterior set through this context")
        out["L"] = np.empty(draws, dtype=np.float64)
        out["L0"] = np.empty(draws, dtype=np.float64)

    def match_leverage_live(self, home_idx, away_idx, table_idx, table, points, n_sims: int, key: Tuple[int, int],
                            target_masks, in_play=None, reweight: bool = True, log_weights=None, chunk_sims: int = 0,
                            pair_init=None, head_to_head: bool = False) -> dict:
        """`match_leverage` with matches in progress and weighted draws (csrc/dc_live_queries.hip.h,
        bplhip_match_leverage_live): simulate_season_live's simulations under the same arguments.  home_idx / away_idx
        are the F fixtures still to kick off; in_play, reweight and log_weights are simulate_season_live's.  Returns
        match_leverage's raw counts over the F + L fixtures of the concatenated list, the matches in play last
        ("outcome" u64 [F + L, 3], "joint" u64 [F + L, 3, n, K]), plus "ess" and "log_evidence" (floats)."""
        return self.match_leverage(home_idx, away_idx, table_idx, table, points, n_sims, key, target_masks,
                                   chunk_sims=chunk_sims, pair_init=pair_init, head_to_head=head_to_head,
                                   live=self._live_request(in_play, reweight, log_weights))

    def season_points_live(self, home_idx, away_idx, table_idx, table, points, n_sims: int, key: Tuple[int, int],
                           target_masks, points_min: int, n_bins: int, in_play=None, reweight: bool = True,
                           log_weights=None, chunk_sims: int = 0, pair_init=None, head_to_head: bool = False) -> dict:
        """`season_points` with matches in progress and weighted draws (csrc/dc_live_queries.hip.h,
        bplhip_season_points_live): simulate_season_live's simulations under the same arguments.  in_play, reweight
        and log_weights are simulate_season_live's; the points axis must hold the matches in play as remaining
        matches.  Returns season_points' raw counts plus "ess" and "log_evidence" (floats)."""
        return self.season_points(home_idx, away_idx, table_idx, table, points, n_sims, key, target_masks, points_min,
                                  n_bins, chunk_sims=chunk_sims, pair_init=pair_init, head_to_head=head_to_head,
                                  live=self._live_request(in_play, reweight, log_weights))

    def season_scenarios_live(self, home_idx, away_idx, table_idx, table, points, n_sims: int, key: Tuple[int, int],
                              target_masks, key_fixture, key_cap, in_play=None, reweight: bool = True,
                              log_weights=None, chunk_sims: int = 0, pair_init=None,
                              head_to_head: bool = False) -> dict:
        """`season_scenarios` with matches in progress and weighted draws (csrc/dc_live_queries.hip.h,
        bplhip_season_scenarios_live): simulate_season_live's simulations under the same arguments.  in_play, reweight
        and log_weights are simulate_season_live's; key_fixture holds positions in the concatenated list, F + m being
        match m in play.  Returns season_scenarios' raw counts plus "ess" and "log_evidence" (floats)."""
        return self.season_scenarios(home_idx, away_idx, table_idx, table, points, n_sims, key, target_masks, key_fixture,
                                     key_cap, chunk_sims=chunk_sims, pair_init=pair_init, head_to_head=head_to_head,
                                     live=self._live_request(in_play, reweight, log_weights))

    def season_trajectory(self, home_idx, away_idx, table_idx, table, points, n_sims: int, key: Tuple[int, int],
                          target_masks, points_min: int, n_bins: int, fix_id, round_end, chunk_sims: int = 0,
                          pair_init=None, head_to_head: bool = False) -> dict:
        """simulate_season's simulations ranked after every matchday, the paths counted on the device
        (csrc/dc_trajectory.hip.h, bplhip_season_trajectory): the arguments up to `n_bins` and chunk_sims, pair_init
        and head_to_head are season_points' (the axis must hold every total a slot passes through); fix_id: the
        fixtures' indices sorted by matchday, round_end [R]: one past each matchday's last entry of fix_id.  The
        fixtures themselves stay in the caller's order: fixture f keeps the random block of simulate_season.
        Returns the raw counts, u64: "position" [R, n, n], "target" and "target_final" [R, n, K], "points_sum" and
        "points_sq_sum" [R, n] (of points - points_min), "rounds_inside" and "secured" [n, K, R + 1],
        "lead_changes" [R]."""
        n, nf, head, _keep = self._season_head(home_idx, away_idx, table_idx, table, points, n_sims, key)
        masks = self._target_masks(target_masks)
        ids = np.ascontiguousarray(fix_id, dtype=np.int32)
        ends = np.ascontiguousarray(round_end, dtype=np.int32)
        if ids.size != nf:
            raise ValueError("fix_id must have one entry per fixture")
        k, r = masks.size, ends.size
        out = {"position": np.zeros((r, n, n), dtype=np.uint64), "target": np.zeros((r, n, k), dtype=np.uint64),
               "target_final": np.zeros((r, n, k), dtype=np.uint64), "points_sum": np.zeros((r, n), dtype=np.uint64),
               "points_sq_sum": np.zeros((r, n), dtype=np.uint64),
               "rounds_inside": np.zeros((n, k, r + 1), dtype=np.uint64),
               "secured": np.zeros((n, k, r + 1), dtype=np.uint64), "lead_changes": np.zeros(r, dtype=np.uint64)}
        # (the entry point reads a non-null pair_init as the head-to-head order)
        pair = self._pair_init(pair_init, n, zeros=True) if head_to_head else None
        with self._torch.cuda.device(self.device):
            self._check(self._lib.bplhip_season_trajectory(
                *head, k, _np_ptr(masks), int(chunk_sims), int(points_min), int(n_bins), r, _np_ptr(ends),
                _np_ptr(ids),
                *(_np_ptr(out[name]) for name in ("position", "target", "target_final", "points_sum", "points_sq_sum",
                                                  "rounds_inside", "secured", "lead_changes")),
                self._stream(), _np_ptr(pair)))
        return out

    def _tournament_head(self, team_idx, bracket, n_sims, key, team_conf, team_host, team_group, table, fix_p, fix_q,
                         advance, best_of_rest, points, pair_init, head_to_head):
        """What every entry point of the tournament family takes first.  Returns (n, rounds, n_groups, keep, head):
        the slots, the knockout rounds R of a bracket of 2^R, the groups, the converted arrays by name ("team_idx",
        "bracket", "team_conf", "team_host", "team_group", "init", "fix_p", "fix_q", "pair"; None where the caller
        gave none), which the caller holds until its call has returned, and the arguments from the context to key_lo
        that point into them."""
        ti = np.ascontiguousarray(team_idx, dtype=np.uint16)
        n = ti.size
        br = np.ascontiguousarray(bracket, dtype=np.uint16)
        rounds = max(int(br.size).bit_length() - 1, 0)
        conf = None if team_conf is None else np.ascontiguousarray(team_conf, dtype=np.uint16)
        host = None if team_host is None else np.ascontiguousarray(team_host, dtype=np.uint8)
        n_groups, grp, init = 0, None, [None, None, None]
        if team_group is not None:
            grp = np.ascontiguousarray(team_group, dtype=np.uint8)
            n_groups = int(grp.max()) + 1 if grp.size else 0
            tab = np.zeros((n, 3), dtype=np.int64) if table is None else np.asarray(table, dtype=np.int64).reshape(n, 3)
            init = [np.ascontiguousarray(tab[:, i], dtype=np.int32) for i in range(3)]
        fp = np.ascontiguousarray(fix_p, dtype=np.uint8)
        fq = np.ascontiguousarray(fix_q, dtype=np.uint8)
        if fp.size != fq.size:
            raise ValueError("fix_p and fix_q must have equal length")
        win, draw, loss = (int(p) for p in points)
        keep = dict(team_idx=ti, bracket=br, team_conf=conf, team_host=host, team_group=grp, init=init, fix_p=fp, fix_q=fq,
                    pair=self._pair_init(pair_init, n) if head_to_head else None)
        head = (self._h, n, _np_ptr(ti), _np_ptr(conf), _np_ptr(host), n_groups, _np_ptr(grp),
                *(_np_ptr(x) for x in init), fp.size, _np_ptr(fp), _np_ptr(fq), int(advance), int(best_of_rest),
                br.size, _np_ptr(br), win, draw, loss, int(n_sims), int(key[0]), int(key[1]))
        return n, rounds, n_groups, keep, head

    @contextlib.contextmanager
    def _allocation(self, allocation, n_groups: int):
        """The best-of-rest allocation in force for the one tournament call inside the block
        (bplhip_tournament_set_allocation): `allocation` is None (nothing is set, nothing cleared) or a dict with
        "row_of_mask" u16 [1 << n_groups], "slots" u8 [rows, n_groups] and "best" (bpl.allocation.device_tables).
        Cleared when the block is left, also by an exception."""
        if allocation is None:
            yield
            return
        rows = np.ascontiguousarray(allocation["row_of_mask"], dtype=np.uint16)
        slots = np.ascontiguousarray(allocation["slots"], dtype=np.uint8)
        if rows.shape != (1 << n_groups,) or slots.ndim != 2 or slots.shape[1] != n_groups:
            raise ValueError("allocation: row_of_mask must be [1 << n_groups] and slots [rows, n_groups]")
        self._check(self._lib.bplhip_tournament_set_allocation(self._h, n_groups, int(allocation["best"]), slots.shape[0],
                                                               _np_ptr(rows), _np_ptr(slots)))
        try:
            yield
        finally:
            self._lib.bplhip_tournament_set_allocation(self._h, 0, 0, 0, None, None)

    @staticmethod
    def _knockout_rule(knockout, n: int, rounds: int, out: dict, decided_shape=None):
        """The knockout rule as the entry points take it after their own flags: (legs_mask, scale, away_goals,
        strength, decided_counts) and the converted strengths, which the caller holds until its call has returned.
        knockout None: the redraw rule's placeholders.  Otherwise out["decided_counts"] u64 [R, 4] is allocated, and
        with decided_shape out["decided"], zeroed u8 of that shape."""
        if knockout is None:
            return (0, 1.0, 0, None, None), None
        strength = knockout.get("strength")
        if strength is not None:
            strength = np.ascontiguousarray(strength, dtype=np.float64)
            if strength.shape != (n,):
                raise ValueError("strength must have one entry per slot")
        out["decided_counts"] = np.zeros((rounds, 4), dtype=np.uint64)
        if decided_shape is not None:
            out["decided"] = np.zeros(decided_shape, dtype=np.uint8)
        return (int(knockout["legs_mask"]), float(knockout["scale"]), int(knockout["away_goals"]), _np_ptr(strength),
                _np_ptr(out["decided_counts"])), strength

    def simulate_tournament(self, team_idx, bracket, n_sims: int, key: Tuple[int, int], team_conf=None,
                            team_host=None, team_group=None, table=None, fix_p=(), fix_q=(), advance: int = 2,
                            best_of_rest: int = 0, points=(3, 1, 0), return_stages: bool = False, pair_init=None,
                            head_to_head: bool = False, knockout=None, allocation=None) -> dict:
        """A group-and-knockout tournament, n_sims times, jointly over the posterior
        (csrc/dc_tournament.hip.h; needs a predict_set_posterior_venue posterior).  team_idx: the
        slots' model indices; team_conf / team_host: per slot (or None); team_group: per slot (None:
        knockout only); table: [n, 3] current (points, goals for, goals against) of the groups;
        fix_p / fix_q: the group fixtures' slots (listed order); bracket: the first round's entries,
        group << 8 | place, 0xFF00 | k (the k-th best of the rest) or, without groups, a slot; key:
        the threefry key (hi, lo).  Returns the raw integer results: "stage_counts" u64 [n, R + 2],
        with groups "position_counts" u64 [n, 8], and when asked "stage" u8 [n_sims, n].  pair_init /
        head_to_head: the groups are ordered by the head-to-head rule (bplhip_simulate_tournament_h2h), as
        for simulate_season.  knockout: None (a level knockout match is redrawn), or the extra-time rule
        (bplhip_simulate_tournament_knockout, csrc/dc_knockout.hip.h) as a dict with "legs_mask" (bit r: round r
        has two legs), "scale" (extra time's share of the rates), "away_goals" and "strength" (f64 per slot, or
        None); it adds "decided_counts" u64 [R, 4] and, with return_stages, "decided" u8 [n_sims, 2^R - 1].
        allocation: None, or the best-of-rest allocation table (`_allocation`), under which the bracket code
        0xFF00 | k is allocation slot k (bplhip_simulate_tournament_alloc); it adds "slot_counts" u64 [n_groups, best]."""
        n, rounds, n_groups, keep, head = self._tournament_head(
            team_idx, bracket, n_sims, key, team_conf, team_host, team_group, table, fix_p, fix_q, advance, best_of_rest,
            points, pair_init, head_to_head)
        n_sims, nm = int(n_sims), max(keep["bracket"].size - 1, 0)
        out = {"stage_counts": np.zeros((n, rounds + 2), dtype=np.uint64)}
        if n_groups:
            out["position_counts"] = np.zeros((n, 8), dtype=np.uint64)
        if return_stages:
            out["stage"] = np.empty((n_sims, n), dtype=np.uint8)
        fn = self._lib.bplhip_simulate_tournament_h2h if head_to_head else self._lib.bplhip_simulate_tournament
        tail = (_np_ptr(keep["pair"]),) if head_to_head else ()
        if knockout is not None:
            rule, strength = self._knockout_rule(knockout, n, rounds, out)
            if return_stages:
                out["decided"] = np.empty((n_sims, nm), dtype=np.uint8)
            fn = self._lib.bplhip_simulate_tournament_knockout
            tail = (_np_ptr(keep["pair"]), int(bool(head_to_head)), *rule, _np_ptr(out.get("decided")))
        if allocation is not None:
            # one entry point for every form under a table: the rule's placeholders when a level match is redrawn
            rule = tail[2:-1] if knockout is not None else self._knockout_rule(None, n, rounds, out)[0]
            out["slot_counts"] = np.zeros((n_groups, int(allocation["best"])), dtype=np.uint64)
            fn = self._lib.bplhip_simulate_tournament_alloc
            tail = (_np_ptr(keep["pair"]), int(bool(head_to_head)), int(knockout is not None), *rule,
                    _np_ptr(out.get("decided")), _np_ptr(out["slot_counts"]))
        with self._torch.cuda.device(self.device), self._allocation(allocation, n_groups):
            self._check(fn(*head, _np_ptr(out["stage_counts"]), _np_ptr(out.get("position_counts")),
                           _np_ptr(out.get("stage")), self._stream(), *tail))
        return out

    def simulate_tournament_live(self, team_idx, bracket, n_sims: int, key: Tuple[int, int], team_conf=None,
                                 team_host=None, team_group=None, table=None, fix_p=(), fix_q=(), advance: int = 2,
                                 best_of_rest: int = 0, points=(3, 1, 0), return_stages: bool = False, pair_init=None,
                                 head_to_head: bool = False, knockout=None, allocation=None, in_play=None,
                                 reweight: bool = True, log_weights=None, return_weights: bool = False) -> dict:
        """`simulate_tournament` with group matches in progress and weighted draws (csrc/dc_tournament_live.hip.h,
        bplhip_simulate_tournament_live).  The arguments up to `allocation` are simulate_tournament's, fix_p / fix_q
        the group fixtures still to kick off.  in_play: None, or (slot p, slot q, goals of p, goals of q, elapsed) of
        the L group matches in progress, in the listed order; log_weights: None or f64 [draws].  Returns
        simulate_tournament's raw results plus "ess" and "log_evidence" (floats), with return_stages "draw" i32
        [n_sims] and "in_play_home_goals" / "in_play_away_goals" u8 [n_sims, L] (final scores, listed order), and with
        return_weights "L" and "L0" f64 [draws]: the draws' log weights and the states' log likelihood per draw."""
        n, rounds, n_groups, keep, head = self._tournament_head(
            team_idx, bracket, n_sims, key, team_conf, team_host, team_group, table, fix_p, fix_q, advance, best_of_rest,
            points, pair_init, head_to_head)
        live = self._live_request(in_play, reweight, log_weights, sides=np.uint8)
        n_live, n_sims, nm = live[0], int(n_sims), max(keep["bracket"].size - 1, 0)
        out = {"stage_counts": np.zeros((n, rounds + 2), dtype=np.uint64)}
        if n_groups:
            out["position_counts"] = np.zeros((n, 8), dtype=np.uint64)
        if return_stages:
            out["stage"] = np.empty((n_sims, n), dtype=np.uint8)
            out["draw"] = np.empty(n_sims, dtype=np.int32)
            out["in_play_home_goals"] = np.empty((n_sims, n_live), dtype=np.uint8)
            out["in_play_away_goals"] = np.empty((n_sims, n_live), dtype=np.uint8)
        self._draw_weight_outputs(out, return_weights)
        rule, _strength = self._knockout_rule(knockout, n, rounds, out, (n_sims, nm) if return_stages else None)
        if allocation is not None:
            out["slot_counts"] = np.zeros((n_groups, int(allocation["best"])), dtype=np.uint64)
        with self._torch.cuda.device(self.device), self._allocation(allocation, n_groups):
            self._check(self._lib.bplhip_simulate_tournament_live(
                *head, _np_ptr(out["stage_counts"]), _np_ptr(out.get("position_counts")), _np_ptr(out.get("stage")),
                self._stream(), _np_ptr(keep["pair"]), int(bool(head_to_head)), int(knockout is not None), *rule,
                _np_ptr(out.get("decided")), _np_ptr(out.get("slot_counts")), *live[1], _np_ptr(out.get("draw")),
                _np_ptr(out.get("L")), _np_ptr(out.get("L0")), _np_ptr(out.get("in_play_home_goals")),
                _np_ptr(out.get("in_play_away_goals"))))
        return self._live_figures(out, live)

    def tournament_paths(self, team_idx, bracket, n_sims: int, key: Tuple[int, int], team_conf=None, team_host=None,
                         team_group=None, table=None, fix_p=(), fix_q=(), advance: int = 2, best_of_rest: int = 0,
                         points=(3, 1, 0), return_records: bool = False, pair_init=None, head_to_head: bool = False,
                         knockout=None, chunk_sims: int = 0, allocation=None, live=None) -> dict:
        """simulate_tournament's simulations cross-tabulated on the device (csrc/dc_paths.hip.h,
        bplhip_tournament_paths): the arguments up to `knockout` are simulate_tournament's, return_records standing
        for return_stages; chunk_sims: simulations per pass through the device workspace (0 = the library's choice;
        the results do not depend on it).  Returns simulate_tournament's raw integer results ("stage_counts", with
        groups "position_counts", under the extra-time rule "decided_counts") and, u64: "advance" [R, n, n] (t went
        through against u in round r); with groups "position_stage" [n, 8, 8]; with group fixtures "outcome"
        [nf, 3] (0 = the first-listed side wins, 1 draw, 2), "target" [n, R + 1] and "joint" [nf, 3, n, R + 1].
        With return_records also, u8: "stage" [n_sims, n], "position" [n_sims, n] (with groups), "group_outcome"
        [n_sims, nf], "pair" [n_sims, 2^R - 1, 2], "winner" [n_sims, 2^R - 1] and under the extra-time rule
        "decided" [n_sims, 2^R - 1].  allocation: as in simulate_tournament, without the slot counts.  live: None
        (this entry), or `_live_request`'s result (tournament_paths_live: the group-fixture axis is then the
        concatenated list)."""
        n, rounds, n_groups, keep, head = self._tournament_head(
            team_idx, bracket, n_sims, key, team_conf, team_host, team_group, table, fix_p, fix_q, advance, best_of_rest,
            points, pair_init, head_to_head)
        n_sims, nm = int(n_sims), max(keep["bracket"].size - 1, 0)
        n_live = 0 if live is None else live[0]
        nf, k = keep["fix_p"].size + n_live, rounds + 1
        rows = max(n_sims, 0)
        out = {"stage_counts": np.zeros((n, rounds + 2), dtype=np.uint64),
               "advance": np.zeros((rounds, n, n), dtype=np.uint64)}
        if n_groups:
            out["position_counts"] = np.zeros((n, 8), dtype=np.uint64)
            out["position_stage"] = np.zeros((n, 8, 8), dtype=np.uint64)
        if nf:
            out.update(outcome=np.zeros((nf, 3), dtype=np.uint64), target=np.zeros((n, k), dtype=np.uint64),
                       joint=np.zeros((nf, 3, n, k), dtype=np.uint64))
        if return_records:
            out["stage"] = np.zeros((rows, n), dtype=np.uint8)
            if n_groups:
                out["position"] = np.zeros((rows, n), dtype=np.uint8)
            out["group_outcome"] = np.zeros((rows, nf), dtype=np.uint8)
            out["pair"] = np.zeros((rows, nm, 2), dtype=np.uint8)
            out["winner"] = np.zeros((rows, nm), dtype=np.uint8)
            if live is not None:
                out["draw"] = np.zeros(rows, dtype=np.int32)
                out["in_play_home_goals"] = np.zeros((rows, n_live), dtype=np.uint8)
                out["in_play_away_goals"] = np.zeros((rows, n_live), dtype=np.uint8)
        rule, strength = self._knockout_rule(knockout, n, rounds, out, (rows, nm) if return_records else None)
        fn, tail = self._lib.bplhip_tournament_paths, ()
        if live is not None:
            fn = self._lib.bplhip_tournament_paths_live
            tail = (*live[1], *(_np_ptr(out.get(name)) for name in ("draw", "in_play_home_goals", "in_play_away_goals")))
        with self._torch.cuda.device(self.device), self._allocation(allocation, n_groups):
            self._check(fn(
                *head, _np_ptr(out["stage_counts"]), _np_ptr(out.get("position_counts")), _np_ptr(out.get("stage")),
                self._stream(), _np_ptr(keep["pair"]), int(bool(head_to_head)), int(knockout is not None), *rule,
                _np_ptr(out.get("decided")), int(chunk_sims),
                *(_np_ptr(out.get(name)) for name in ("advance", "position_stage", "outcome", "target", "joint",
                                                      "position", "group_outcome", "pair", "winner")), *tail))
        return self._live_figures(out, live)

    def tournament_paths_live(self, *args, in_play=None, reweight: bool = True, log_weights=None, **kwargs) -> dict:
        """`tournament_paths` with group matches in progress and weighted draws
        (csrc/dc_tournament_live_queries.hip.h, bplhip_tournament_paths_live): tournament_paths' arguments, fix_p /
        fix_q the group fixtures still to kick off, and simulate_tournament_live's in_play, reweight and log_weights.
        The group-fixture axis of "outcome", "joint" and "group_outcome" is the concatenated list, the fixtures and then
        the L matches in play.  Adds "ess" and "log_evidence" (floats) and with return_records "draw" i32 [n_sims] and
        "in_play_home_goals" / "in_play_away_goals" u8 [n_sims, L] (final scores, listed order)."""
        return self.tournament_paths(*args, live=self._live_request(in_play, reweight, log_weights, sides=np.uint8),
                                     **kwargs)

    def tournament_scenarios(self, team_idx, bracket, n_sims: int, key: Tuple[int, int], team_conf=None,
                             team_host=None, team_group=None, table=None, fix_p=(), fix_q=(), advance: int = 2,
                             best_of_rest: int = 0, points=(3, 1, 0), return_records: bool = False, pair_init=None,
                             head_to_head: bool = False, knockout=None, chunk_sims: int = 0, key_fixture=(),
                             key_cap=(), allocation=None, live=None) -> dict:
        """simulate_tournament's simulations, the joint class of the key group fixtures cross-tabulated against the
        K = R + 2 targets (plays knockout round k < R; wins; first in its group) on the device
        (csrc/dc_tscen.hip.h, bplhip_tournament_scenarios): the arguments are tournament_paths'; key_fixture [k]:
        the key fixtures' positions in the group-fixture list; key_cap [k]: their margin caps c, 2 c + 1 classes
        each (class = c - clipped margin in the LISTED order of the fixture).  A scenario is one class per key,
        row-major in the order given, M = the product of the class counts (the library refuses more than
        SCENARIO_MAX_CELLS, and a call without groups or group fixtures).  Returns the raw counts: "scenario" u64
        [M], "joint" u64 [M, n, K], under the extra-time rule "decided_counts" u64 [R, 4], and with return_records
        "sim_scenario" u32 [n_sims] and "sim_tset" u8 [n_sims, n] (bit k: inside target k).  allocation, live: as in
        tournament_paths (live: the keys index the concatenated list)."""
        n, rounds, n_groups, keep, head = self._tournament_head(
            team_idx, bracket, n_sims, key, team_conf, team_host, team_group, table, fix_p, fix_q, advance, best_of_rest,
            points, pair_init, head_to_head)
        n_sims = int(n_sims)
        kf, kc, cells = self._scenario_keys(key_fixture, key_cap)
        k, rows = rounds + 2, max(n_sims, 0)
        out = {"scenario": np.zeros(cells, dtype=np.uint64), "joint": np.zeros((cells, n, k), dtype=np.uint64)}
        if return_records:
            out["sim_scenario"] = np.zeros(rows, dtype=np.uint32)
            out["sim_tset"] = np.zeros((rows, n), dtype=np.uint8)
            if live is not None:
                out["draw"] = np.zeros(rows, dtype=np.int32)
                out["in_play_home_goals"] = np.zeros((rows, live[0]), dtype=np.uint8)
                out["in_play_away_goals"] = np.zeros((rows, live[0]), dtype=np.uint8)
        rule, strength = self._knockout_rule(knockout, n, rounds, out)
        fn, tail = self._lib.bplhip_tournament_scenarios, ()
        if live is not None:
            fn = self._lib.bplhip_tournament_scenarios_live
            tail = (*live[1], *(_np_ptr(out.get(name)) for name in ("draw", "in_play_home_goals", "in_play_away_goals")))
        with self._torch.cuda.device(self.device), self._allocation(allocation, n_groups):
            self._check(fn(
                *head, self._stream(), _np_ptr(keep["pair"]), int(bool(head_to_head)), int(knockout is not None), *rule,
                int(chunk_sims), kf.size, _np_ptr(kf), _np_ptr(kc), _np_ptr(out["scenario"]), _np_ptr(out["joint"]),
                _np_ptr(out.get("sim_scenario")), _np_ptr(out.get("sim_tset")), *tail))
        return self._live_figures(out, live)

    def tournament_scenarios_live(self, *args, in_play=None, reweight: bool = True, log_weights=None, **kwargs) -> dict:
        """`tournament_scenarios` with group matches in progress and weighted draws
        (csrc/dc_tournament_live_queries.hip.h, bplhip_tournament_scenarios_live): tournament_scenarios' arguments,
        fix_p / fix_q the group fixtures still to kick off, key_fixture positions in the concatenated list (F + m:
        match m in play), and simulate_tournament_live's in_play, reweight and log_weights.  Adds what
        tournament_paths_live adds."""
        return self.tournament_scenarios(*args, live=self._live_request(in_play, reweight, log_weights, sides=np.uint8),
                                         **kwargs)

    def tournament_points(self, team_idx, bracket, n_sims: int, key: Tuple[int, int], team_conf=None, team_host=None,
                          team_group=None, table=None, fix_p=(), fix_q=(), advance: int = 2, best_of_rest: int = 0,
                          points=(3, 1, 0), pair_init=None, head_to_head: bool = False, knockout=None,
                          chunk_sims: int = 0, points_min: int = 0, n_bins: int = 1, gd_cap: int = 3,
                          allocation=None, live=None) -> dict:
        """simulate_tournament's simulations, every slot's group points cross-tabulated on the device against its
        K = R + 2 targets and its group place, the points of every group place and the points and clipped goal
        difference of the slots placed advance + 1 against their rank across the groups
        (csrc/dc_group_points.hip.h, bplhip_tournament_points): the arguments up to chunk_sims are
        tournament_scenarios'; points_min / n_bins: the points axis (bin b = points_min + b points, at most
        GROUP_POINTS_MAX_BINS); gd_cap: the goal-difference axis, D = 2 gd_cap + 1 bins.  With Z the largest group and
        B the groups with a place advance + 1, returns the raw counts, u64: "team_points" [n, P], "team_target"
        [n, P, K], "team_place" [n, P, Z], "place_points" [Gn, Z, P], "place_gap" [Gn, Z - 1, P]; with best_of_rest
        > 0 "rest_count" and "rest_through" [P, D] and "rest_rank" [B, P, D]; under the extra-time rule
        "decided_counts" u64 [R, 4].  allocation, live: as in tournament_paths (live: the matches in play are matches
        to come on the points axis)."""
        n, rounds, n_groups, keep, head = self._tournament_head(
            team_idx, bracket, n_sims, key, team_conf, team_host, team_group, table, fix_p, fix_q, advance, best_of_rest,
            points, pair_init, head_to_head)
        size, rest_groups = 1, 0
        if n_groups:
            sizes = np.bincount(keep["team_group"], minlength=n_groups)
            size, rest_groups = max(int(sizes.max(initial=1)), 1), int((sizes > int(advance)).sum())
        # (outside its ranges the library refuses the call before it writes an output)
        p = int(n_bins) if 1 <= int(n_bins) <= GROUP_POINTS_MAX_BINS else 1
        d = 2 * int(gd_cap) + 1 if 0 <= int(gd_cap) <= GROUP_POINTS_MAX_GD_CAP else 1
        k = rounds + 2
        out = {"team_points": np.zeros((n, p), dtype=np.uint64), "team_target": np.zeros((n, p, k), dtype=np.uint64),
               "team_place": np.zeros((n, p, size), dtype=np.uint64),
               "place_points": np.zeros((n_groups, size, p), dtype=np.uint64),
               "place_gap": np.zeros((n_groups, size - 1, p), dtype=np.uint64)}
        if int(best_of_rest) > 0:
            out.update(rest_count=np.zeros((p, d), dtype=np.uint64), rest_through=np.zeros((p, d), dtype=np.uint64),
                       rest_rank=np.zeros((rest_groups, p, d), dtype=np.uint64))
        rule, strength = self._knockout_rule(knockout, n, rounds, out)
        fn, tail = self._lib.bplhip_tournament_points, ()
        if live is not None:
            fn, tail = self._lib.bplhip_tournament_points_live, live[1]
        with self._torch.cuda.device(self.device), self._allocation(allocation, n_groups):
            self._check(fn(
                *head, self._stream(), _np_ptr(keep["pair"]), int(bool(head_to_head)), int(knockout is not None), *rule,
                int(chunk_sims), int(points_min), int(n_bins), int(gd_cap),
                *(_np_ptr(out.get(name)) for name in ("team_points", "team_target", "team_place", "place_points",
                                                      "place_gap", "rest_count", "rest_through", "rest_rank")), *tail))
        return self._live_figures(out, live)

    def tournament_points_live(self, *args, in_play=None, reweight: bool = True, log_weights=None, **kwargs) -> dict:
        """`tournament_points` with group matches in progress and weighted draws
        (csrc/dc_tournament_live_queries.hip.h, bplhip_tournament_points_live): tournament_points' arguments, fix_p /
        fix_q the group fixtures still to kick off, points_min / n_bins an axis that holds the matches in play as
        matches to come, and simulate_tournament_live's in_play, reweight and log_weights.  Adds "ess" and
        "log_evidence" (floats)."""
        return self.tournament_points(*args, live=self._live_request(in_play, reweight, log_weights, sides=np.uint8),
                                      **kwargs)

    def loglik_matrix(self, home_idx, away_idx, home_goals, away_goals, neutral=None, conf=None) -> np.ndarray:
        """ll[draw, fixture] = log p(goals | draw) of the uploaded posterior, float64 [draws, m]
        (csrc/dc_loglik.hip.h).  `neutral` / `conf` as in predict_score_proba."""
        q = fixtures(home_idx, away_idx, home_goals, away_goals, neutral, conf)
        out = np.empty((getattr(self, "pred_draws", 0), q.m), dtype=np.float64)
        with self._torch.cuda.device(self.device):
            self._check(self._lib.bplhip_loglik_matrix(self._h, C.byref(q), _np_ptr(out), self._stream()))
        return out

    def loglik_summary(self, home_idx, away_idx, home_goals, away_goals, neutral=None, conf=None,
                       r_eff: float = 1.0, psis: bool = True) -> dict:
        """Per-fixture summaries of the log-likelihood over the draws, without the matrix
        (csrc/dc_loglik.hip.h): "lppd", "mean", "var" float64 [m]; with psis also "elpd_loo",
        "pareto_k" float64 [m] and "tail_len" int32 [m] (PSIS-LOO)."""
        q = fixtures(home_idx, away_idx, home_goals, away_goals, neutral, conf)
        keys = ("lppd", "mean", "var") + (("elpd_loo", "pareto_k") if psis else ())
        out = {k: np.empty(q.m, dtype=np.float64) for k in keys}
        if psis:
            out["tail_len"] = np.empty(q.m, dtype=np.int32)
        outs = [_np_ptr(out.get(k)) for k in ("lppd", "mean", "var", "elpd_loo", "pareto_k", "tail_len")]
        with self._torch.cuda.device(self.device):
            self._check(self._lib.bplhip_loglik_summary(
                self._h, C.byref(q), float(r_eff), int(bool(psis)), *outs, self._stream()))
        return out

    def outcome_scores(self, home_idx, away_idx, home_goals, away_goals, max_goals: int, neutral=None,
                       conf=None) -> dict:
        """Outcome probabilities of the m fixtures on the grid 0..max_goals and the scoring rules of every
        draw's own probabilities against the actual goals (csrc/dc_score.hip.h): "proba" float64 [m, 3]
        (home win, draw, away win; the mean over the draws) and "draw_sums" float64 [draws, 3] (per draw
        the sums over the fixtures of the log score, the Brier score and the ranked probability score).
        `neutral` / `conf` as in predict_score_proba."""
        q = fixtures(home_idx, away_idx, home_goals, away_goals, neutral, conf)
        out = {"proba": np.empty((q.m, 3), dtype=np.float64),
               "draw_sums": np.empty((getattr(self, "pred_draws", 0), 3), dtype=np.float64)}
        with self._torch.cuda.device(self.device):
            self._check(self._lib.bplhip_outcome_scores(
                self._h, C.byref(q), int(max_goals), _np_ptr(out["proba"]), _np_ptr(out["draw_sums"]), self._stream()))
        return out

    def loo_scores(self, home_idx, away_idx, home_goals, away_goals, max_goals: int, r_eff: float = 1.0,
                   neutral=None, conf=None) -> dict:
        """Leave-one-out forecasts of the m fixtures, each under its own PSIS-LOO weights (csrc/dc_loo.hip.h,
        DESIGN.md section 32): "elpd_loo", "pareto_k", "ess" float64 [m] and "tail_len" int32 [m] (the first,
        second and last as loglik_summary); "proba" float64 [m, 3], the weighted sum over the draws of the outcome
        probabilities of outcome_scores, and "proba_in_sample" [m, 3], their plain mean; "pit" float64 [m, 4]: the
        weighted home goal distribution below and up to the actual home goals, then the away pair, on the grid
        0..max_goals.  `neutral` / `conf` as in predict_score_proba."""
        q = fixtures(home_idx, away_idx, home_goals, away_goals, neutral, conf)
        out = {k: np.empty(q.m, dtype=np.float64) for k in ("elpd_loo", "pareto_k", "ess")}
        out["tail_len"] = np.empty(q.m, dtype=np.int32)
        out.update(proba=np.empty((q.m, 3), dtype=np.float64), proba_in_sample=np.empty((q.m, 3), dtype=np.float64),
                   pit=np.empty((q.m, 4), dtype=np.float64))
        outs = [_np_ptr(out[k]) for k in ("elpd_loo", "pareto_k", "tail_len", "ess", "proba", "proba_in_sample", "pit")]
        with self._torch.cuda.device(self.device):
            self._check(self._lib.bplhip_loo_scores(
                self._h, C.byref(q), float(r_eff), int(max_goals), *outs, self._stream()))
        return out

    def _block_queries(self, m, block_idx, n_blocks):
        b = np.ascontiguousarray(block_idx, dtype=np.int32)
        if b.shape != (m,):
            raise ValueError("block_idx must have one value per fixture")
        return b, int(n_blocks)

    def block_loglik(self, home_idx, away_idx, home_goals, away_goals, block_idx, n_blocks: int, neutral=None,
                     conf=None) -> np.ndarray:
        """A[b, draw] = the sum of the log-likelihood over the fixtures with block_idx = b, float64
        [n_blocks, draws] (csrc/dc_sequential.hip.h); 0 for a block without fixtures.  `neutral` / `conf` as
        in predict_score_proba."""
        q = fixtures(home_idx, away_idx, home_goals, away_goals, neutral, conf)
        b, B = self._block_queries(q.m, block_idx, n_blocks)
        out = np.empty((max(B, 0), getattr(self, "pred_draws", 0)), dtype=np.float64)
        with self._torch.cuda.device(self.device):
            self._check(self._lib.bplhip_block_loglik(self._h, C.byref(q), _np_ptr(b), B, _np_ptr(out), self._stream()))
        return out

    def psis_weights(self, log_ratios, r_eff: float = 1.0) -> dict:
        """Pareto-smoothed, normalised log weights of the rows of `log_ratios` float64 [blocks, draws]
        (csrc/dc_sequential.hip.h; needs no posterior): "log_weights" [blocks, draws],
        "pareto_k", "ess" float64 [blocks], "tail_len" int32 [blocks]."""
        r = np.ascontiguousarray(log_ratios, dtype=np.float64)
        if r.ndim != 2:
            raise ValueError("log_ratios must have shape [blocks, draws]")
        B, S = r.shape
        out = {"log_weights": np.empty((B, S), dtype=np.float64), "pareto_k": np.empty(B, dtype=np.float64),
               "ess": np.empty(B, dtype=np.float64), "tail_len": np.empty(B, dtype=np.int32)}
        with self._torch.cuda.device(self.device):
            self._check(self._lib.bplhip_psis_weights(
                self._h, B, S, _np_ptr(r), float(r_eff), _np_ptr(out["log_weights"]), _np_ptr(out["pareto_k"]),
                _np_ptr(out["ess"]), _np_ptr(out["tail_len"]), self._stream()))
        return out

    def weighted_scores(self, home_idx, away_idx, home_goals, away_goals, block_idx, log_weights, max_goals: int,
                        neutral=None, conf=None) -> dict:
        """Importance-weighted forecasts of the m fixtures, each under the row of `log_weights` float64
        [blocks, draws] that block_idx names (csrc/dc_sequential.hip.h): "elpd" float64 [m] =
        lse_s(log weight + log-likelihood) and "proba" float64 [m, 3], the weighted sum over the draws of the
        outcome probabilities of outcome_scores.  `neutral` / `conf` as in predict_score_proba."""
        q = fixtures(home_idx, away_idx, home_goals, away_goals, neutral, conf)
        lw = np.ascontiguousarray(log_weights, dtype=np.float64)
        S = getattr(self, "pred_draws", 0)   # (0: no posterior; the library says so)
        if lw.ndim != 2 or (S and lw.shape[1] != S):
            raise ValueError("log_weights must have shape [blocks, draws]")
        b, B = self._block_queries(q.m, block_idx, lw.shape[0])
        out = {"elpd": np.empty(q.m, dtype=np.float64), "proba": np.empty((q.m, 3), dtype=np.float64)}
        with self._torch.cuda.device(self.device):
            self._check(self._lib.bplhip_weighted_scores(
                self._h, C.byref(q), _np_ptr(b), B, _np_ptr(lw), int(max_goals), _np_ptr(out["elpd"]),
                _np_ptr(out["proba"]), self._stream()))
        return out

    # ---- what the summary queries share (market, period, in-play, slate, ratings)
    @staticmethod
    def _market_weights(weights, max_goals: int, power: int, top: int, shape: str):
        """float64 weights [K, (max_goals+1)^power] and K; the size is compared for a max_goals the library takes."""
        w = np.ascontiguousarray(weights, dtype=np.float64)
        K = w.shape[0] if w.ndim else 0
        if 0 <= int(max_goals) <= top and w.size != K * (int(max_goals) + 1) ** power:
            raise ValueError(f"weights must have shape [K, {shape}]")
        return w, K

    def _summary_outputs(self, quantiles, K: int, n: int, rows, return_draws: bool):
        """The quantile levels, the summary's outputs over K statistics of n items, and with return_draws the buffer
        [*rows, draws] the library fills with the per-draw values."""
        qs = np.ascontiguousarray(quantiles, dtype=np.float64).reshape(-1)
        out = {"mean": np.empty((K, n), dtype=np.float64), "sd": np.empty((K, n), dtype=np.float64),
               "quantile": np.empty((K, qs.size, n), dtype=np.float64)}
        S = getattr(self, "pred_draws", 0)
        return qs, out, np.empty((*rows, S), dtype=np.float64) if return_draws else None

    def market_summary(self, home_idx, away_idx, max_goals: int, weights, quantiles=(), neutral=None, conf=None,
                       return_draws: bool = False, workspace_bytes: int = 0) -> dict:
        """Match markets of the m fixtures on the grid 0..max_goals (csrc/dc_market.hip.h): market k of draw s
        is sum_xy weights[k, x, y] q_s(x, y), formed per draw and summarised over the draws.  `weights`
        float64 [K, max_goals+1, max_goals+1] (axis 1 the home goals), `quantiles` [Q] in [0, 1].  Returns
        "mean", "sd" float64 [K, m], "quantile" [K, Q, m] (linear interpolation between exact order
        statistics) and, with return_draws, "draws" [draws, K, m].  `workspace_bytes` caps the device
        memory for the per-draw values (0: the library's default); the fixtures go in chunks that fit.
        `neutral` / `conf` as in predict_score_proba."""
        q = fixtures(home_idx, away_idx, neutral=neutral, conf=conf)
        m = q.m
        w, K = self._market_weights(weights, max_goals, 2, 63, "max_goals+1, max_goals+1")
        qs, out, draws = self._summary_outputs(quantiles, K, m, (m, K), return_draws)
        with self._torch.cuda.device(self.device):
            self._check(self._lib.bplhip_market_summary(
                self._h, C.byref(q), int(max_goals), K, _np_ptr(w), qs.size, _np_ptr(qs), _np_ptr(out["mean"]),
                _np_ptr(out["sd"]), _np_ptr(out["quantile"]), _np_ptr(draws), int(workspace_bytes), self._stream()))
        if return_draws:
            out["draws"] = np.ascontiguousarray(draws.transpose(2, 1, 0))
        return out

    def slate_summary(self, home_idx, away_idx, max_goals: int, tables, leg_table, start, quantiles=(), neutral=None,
                      conf=None, return_draws: bool = False, workspace_bytes: int = 0) -> dict:
        """Totals over slates of the m fixtures (csrc/dc_slate.hip.h): fixture i scores tables[leg_table[i], x, y]
        (uint8 [L, max_goals+1, max_goals+1], values 0..7; axis 1 the home goals) at the final score (x, y), and
        slate j is the fixtures start[j] .. start[j+1]-1 (int32 [J+1]) in the order given.  Per draw the law of a
        slate's total is the convolution of its fixtures' value laws; with P the largest total any slate can reach
        the K = 2 (P+1) + 2 statistics pmf[0..P], at_least[0..P], expected, mass are summarised over the draws as
        market_summary does.  Returns "mean", "sd" float64 [K, J], "quantile" [K, Q, J], "leg_proba" [m, 8] (the
        fixtures' value laws, averaged over the draws) and, with return_draws, "draws" [draws, J, P+1] (the pmf).
        `workspace_bytes` caps the device memory for the per-draw values of a chunk of slates (0: the library's
        default).  `neutral` / `conf` as in predict_score_proba."""
        q = fixtures(home_idx, away_idx, neutral=neutral, conf=conf)
        m = q.m
        t = np.ascontiguousarray(tables, dtype=np.uint8)
        L = t.shape[0] if t.ndim else 0
        if 0 <= int(max_goals) <= 63 and (L == 0 or t.size != L * (int(max_goals) + 1) ** 2):
            raise ValueError("tables must have shape [L, max_goals+1, max_goals+1], L >= 1")
        lt = np.ascontiguousarray(leg_table, dtype=np.int32).reshape(-1)
        st = np.ascontiguousarray(start, dtype=np.int32).reshape(-1)
        if lt.size != m or st.size < 2:
            raise ValueError("leg_table must have one index per fixture and start at least two entries")
        J = st.size - 1
        # the size of the outputs: P as the library derives it (it repeats every check)
        tops = t.reshape(L, -1).max(axis=1, initial=0).astype(np.int64)
        inside = lt[(lt >= 0) & (lt < L)]
        csum = np.concatenate([[0], np.cumsum(tops[inside])]) if inside.size == m else np.zeros(m + 1, dtype=np.int64)
        ends = np.clip(st, 0, m)
        P = int(min(max((csum[ends[1:]] - csum[ends[:-1]]).max(), 0), 127))
        K = 2 * (P + 1) + 2
        qs, out, draws = self._summary_outputs(quantiles, K, J, (J, P + 1), return_draws)
        leg = np.empty((8, m), dtype=np.float64)
        with self._torch.cuda.device(self.device):
            self._check(self._lib.bplhip_slate_summary(
                self._h, C.byref(q), int(max_goals), J, _np_ptr(st), L, _np_ptr(t), _np_ptr(lt), qs.size, _np_ptr(qs),
                _np_ptr(out["mean"]), _np_ptr(out["sd"]), _np_ptr(out["quantile"]), _np_ptr(leg), _np_ptr(draws),
                int(workspace_bytes), self._stream()))
        out["leg_proba"] = np.ascontiguousarray(leg.T)
        if return_draws:
            out["draws"] = np.ascontiguousarray(draws.transpose(2, 0, 1))
        return out

    def team_ratings(self, teams, opponents, venue: int, max_goals: int, points, rank_by: int = 0, quantiles=(),
                     team_conf=None, opponent_conf=None, return_draws: bool = False, workspace_bytes: int = 0) -> dict:
        """Ratings of the R `teams` against the field `opponents` (model indices; csrc/dc_ratings.hip.h): per draw
        the five statistics points, win, goals_for, goals_against, goal_difference averaged over a team's matches
        under `venue` (0 both, 1 home, 2 away, 3 neutral), summarised over the draws, and the per-draw ranks by
        statistic `rank_by`.  `points` = (win, draw, loss); `team_conf` / `opponent_conf` the confederation
        indices when the posterior has them.  Returns "mean", "sd" float64 [5, R], "quantile" [5, Q, R],
        "rank_count", "better_count" int32 [R, R], "matches" int32 [R] and, with return_draws, "draws"
        [draws, 5, R].  `workspace_bytes` caps the device memory for the per-draw values of a chunk of teams
        (0: the library's default)."""
        def u16(a):
            return None if a is None else np.ascontiguousarray(a, dtype=np.uint16).reshape(-1)

        t, o, tc, oc = u16(teams), u16(opponents), u16(team_conf), u16(opponent_conf)
        if (tc is not None and tc.size != t.size) or (oc is not None and oc.size != o.size):
            raise ValueError("one confederation per team and per opponent")
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1)
        if pts.size != 3:
            raise ValueError("points must be (win, draw, loss)")
        R, K = t.size, 5
        qs, out, draws = self._summary_outputs(quantiles, K, R, (R, K), return_draws)
        out.update(rank_count=np.empty((R, R), dtype=np.int32), better_count=np.empty((R, R), dtype=np.int32),
                   matches=np.empty(R, dtype=np.int32))
        with self._torch.cuda.device(self.device):
            self._check(self._lib.bplhip_team_ratings(
                self._h, R, _np_ptr(t), _np_ptr(tc), o.size, _np_ptr(o), _np_ptr(oc), int(venue), int(max_goals),
                _np_ptr(pts), int(rank_by), qs.size, _np_ptr(qs), _np_ptr(out["mean"]), _np_ptr(out["sd"]),
                _np_ptr(out["quantile"]), _np_ptr(out["rank_count"]), _np_ptr(out["better_count"]),
                _np_ptr(out["matches"]), _np_ptr(draws), int(workspace_bytes), self._stream()))
        if return_draws:
            out["draws"] = np.ascontiguousarray(draws.transpose(2, 1, 0))
        return out

    def inplay_summary(self, home_idx, away_idx, home_goals, away_goals, elapsed, max_goals: int, weights,
                       quantiles=(), reweight: bool = True, log_weights=None, neutral=None, conf=None,
                       return_draws: bool = False, workspace_bytes: int = 0) -> dict:
        """Markets of the m matches in progress (csrc/dc_inplay.hip.h): `home_goals` / `away_goals` the current
        score, `elapsed` float64 [m] in [0, 1) the fraction played.  Market k of draw s is the conditional law
        of the FINAL score given the state, contracted with weights[k, x, y] (float64 [K, max_goals+1,
        max_goals+1], indexed by the final score); the draws are re-weighted per fixture by the likelihood of the
        state (`reweight`) and by `log_weights` float64 [draws] if given.  Returns "mean", "sd" float64 [K, m],
        "quantile" [K, Q, m] (weighted inverted CDF, no interpolation), "ess", "log_evidence" [m] and, with
        return_draws, "draws" [draws, K, m] and "draw_log_evidence" [draws, m].  `workspace_bytes` as in
        market_summary.  `neutral` / `conf` as in predict_score_proba."""
        q = fixtures(home_idx, away_idx, home_goals, away_goals, neutral, conf)
        m = q.m
        t = np.ascontiguousarray(elapsed, dtype=np.float64)
        if t.shape != (m,):
            raise ValueError("elapsed must have one value per fixture")
        w, K = self._market_weights(weights, max_goals, 2, 63, "max_goals+1, max_goals+1")
        qs, out, draws = self._summary_outputs(quantiles, K, m, (m, K), return_draws)
        S = getattr(self, "pred_draws", 0)
        lw = None if log_weights is None else np.ascontiguousarray(log_weights, dtype=np.float64)
        if lw is not None and (lw.ndim != 1 or (S and lw.shape[0] != S)):
            raise ValueError("log_weights must have shape [draws]")
        out.update(ess=np.empty(m, dtype=np.float64), log_evidence=np.empty(m, dtype=np.float64))
        lev = np.empty((m, S), dtype=np.float64) if return_draws else None
        with self._torch.cuda.device(self.device):
            self._check(self._lib.bplhip_inplay_summary(
                self._h, C.byref(q), _np_ptr(t), int(max_goals), K, _np_ptr(w), qs.size, _np_ptr(qs),
                int(bool(reweight)), _np_ptr(lw), _np_ptr(out["mean"]), _np_ptr(out["sd"]), _np_ptr(out["quantile"]),
                _np_ptr(out["ess"]), _np_ptr(out["log_evidence"]), _np_ptr(draws), _np_ptr(lev),
                int(workspace_bytes), self._stream()))
        if return_draws:
            out["draws"] = np.ascontiguousarray(draws.transpose(2, 1, 0))
            out["draw_log_evidence"] = np.ascontiguousarray(lev.T)
        return out

    def period_summary(self, home_idx, away_idx, split, max_goals: int, weights, quantiles=(), neutral=None,
                       conf=None, return_draws: bool = False, workspace_bytes: int = 0) -> dict:
        """Period markets of the m fixtures (csrc/dc_period.hip.h): `split` float64 [m] in [0, 1] the share of the
        match's scoring before the split; market k of draw s is sum weights[k, a, b, x, y] p_s(a, b, x, y) over
        the score (a, b) at the split and the final score (x, y), 0 <= a <= x <= max_goals, 0 <= b <= y <=
        max_goals (0..31; the other cells of `weights` float64 [K, (max_goals+1)^4] are never read), formed
        per draw and summarised over the draws as market_summary does.  Returns "mean", "sd" float64 [K, m],
        "quantile" [K, Q, m] and, with return_draws, "draws" [draws, K, m].  `workspace_bytes` as in
        market_summary.  `neutral` / `conf` as in predict_score_proba."""
        q = fixtures(home_idx, away_idx, neutral=neutral, conf=conf)
        m = q.m
        t = np.ascontiguousarray(split, dtype=np.float64)
        if t.shape != (m,):
            raise ValueError("split must have one value per fixture")
        w, K = self._market_weights(weights, max_goals, 4, 31, "max_goals+1, max_goals+1, max_goals+1, max_goals+1")
        qs, out, draws = self._summary_outputs(quantiles, K, m, (m, K), return_draws)
        with self._torch.cuda.device(self.device):
            self._check(self._lib.bplhip_period_summary(
                self._h, C.byref(q), _np_ptr(t), int(max_goals), K, _np_ptr(w), qs.size, _np_ptr(qs),
                _np_ptr(out["mean"]), _np_ptr(out["sd"]), _np_ptr(out["quantile"]), _np_ptr(draws),
                int(workspace_bytes), self._stream()))
        if return_draws:
            out["draws"] = np.ascontiguousarray(draws.transpose(2, 1, 0))
        return out

    def mcmc_diagnostics(self, values, num_chains: int, quantiles=(0.05, 0.95), workspace_bytes: int = 0) -> dict:
        """Convergence diagnostics of float64 `values` [num_chains * N, Q], chain-major rows, one quantity per
        column (csrc/dc_diagnostics.hip.h; definitions: DESIGN.md section 20).  Returns float64 [Q] arrays
        "mean", "sd", "rhat", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean".  `workspace_bytes` caps the
        device memory beyond the draws (0: the library's default); the quantities go in chunks that fit."""
        v = np.ascontiguousarray(values, dtype=np.float64)
        if v.ndim != 2 or int(num_chains) < 1 or v.shape[0] % int(num_chains):
            raise ValueError("values must be [num_chains * N, Q]")
        qs = np.ascontiguousarray(quantiles, dtype=np.float64).reshape(-1)
        names = ("mean", "sd", "rhat", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean")
        out = {nm: np.empty(v.shape[1], dtype=np.float64) for nm in names}
        with self._torch.cuda.device(self.device):
            self._check(self._lib.bplhip_mcmc_diagnostics(
                self._h, int(num_chains), v.shape[0] // int(num_chains), v.shape[1], _np_ptr(v), qs.size, _np_ptr(qs),
                int(workspace_bytes), *(_np_ptr(out[nm]) for nm in names), self._stream()))
        return out

    def weighted_shift(self, values, log_ratios, r_eff: float = 1.0, workspace_bytes: int = 0) -> dict:
        """The shift of every column of float64 `values` [draws, Q] under the Pareto-smoothed weights of the rows
        of `log_ratios` float64 [rows, draws] (csrc/dc_sensitivity.hip.h; definitions: DESIGN.md section 33; needs
        no posterior).  Returns "cjs_sq", "mean", "sd" float64 [rows, Q] and psis_weights' "log_weights",
        "pareto_k", "ess", "tail_len" for the rows.  `workspace_bytes` caps the device memory of the sort beyond
        12 288 draws (0: the library's default); the quantities go in chunks that fit."""
        v = np.ascontiguousarray(values, dtype=np.float64)
        r = np.ascontiguousarray(log_ratios, dtype=np.float64)
        if v.ndim != 2 or r.ndim != 2 or r.shape[1] != v.shape[0]:
            raise ValueError("values must be [draws, Q] and log_ratios [rows, draws]")
        (S, Q), R = v.shape, r.shape[0]
        out = {"log_weights": np.empty((R, S), dtype=np.float64), "pareto_k": np.empty(R, dtype=np.float64),
               "ess": np.empty(R, dtype=np.float64), "tail_len": np.empty(R, dtype=np.int32)}
        out.update({nm: np.empty((R, Q), dtype=np.float64) for nm in ("cjs_sq", "mean", "sd")})
        names = ("log_weights", "pareto_k", "ess", "tail_len", "cjs_sq", "mean", "sd")
        with self._torch.cuda.device(self.device):
            self._check(self._lib.bplhip_weighted_shift(
                self._h, S, Q, _np_ptr(v), R, _np_ptr(r), float(r_eff), int(workspace_bytes),
                *(_np_ptr(out[nm]) for nm in names), self._stream()))
        return out

    def ppc(self, home_idx, away_idx, home_slot, away_slot, n_slots: int, max_goals: int, n_reps: int,
            key: Tuple[int, int], fixture_id=None, neutral=None, conf=None, return_scores: bool = False) -> dict:
        """Posterior predictive replications of m fixtures, reduced per replication on the device
        (csrc/dc_ppc.hip.h).  home_slot / away_slot: the teams' slots (< n_slots) in the caller's numbering;
        fixture_id: the RNG counter of each fixture (None: 0..m-1); `neutral` / `conf` as in
        predict_score_proba; key: the threefry key (hi, lo).  Returns the raw integer results per
        replication: "score" u32 [n_reps, max_goals+1, max_goals+1], "outcome" u32 [n_reps, 3] (home win,
        draw, away win), "sums" i64 [n_reps, 5] (sum x, y, x^2, y^2, x y), "team" u32 [n_reps, n_slots, 4]
        (goals for, goals against, wins, draws), and when asked "home_goals" / "away_goals" u8 [n_reps, m]."""
        q = fixtures(home_idx, away_idx, neutral=neutral, conf=conf)
        hs = np.ascontiguousarray(home_slot, dtype=np.uint16)
        as_ = np.ascontiguousarray(away_slot, dtype=np.uint16)
        m, R, k, g1 = q.m, int(n_reps), int(n_slots), int(max_goals) + 1
        if not (hs.size == as_.size == m):
            raise ValueError("query arrays must have equal length")
        fid = None if fixture_id is None else np.ascontiguousarray(fixture_id, dtype=np.uint32)
        if fid is not None and fid.size != m:
            raise ValueError("fixture_id must have one entry per fixture")
        out = {"score": np.empty((R, g1, g1), dtype=np.uint32), "outcome": np.empty((R, 3), dtype=np.uint32),
               "sums": np.empty((R, 5), dtype=np.int64), "team": np.empty((R, k, 4), dtype=np.uint32)}
        if return_scores:
            out["home_goals"] = np.empty((R, m), dtype=np.uint8)
            out["away_goals"] = np.empty((R, m), dtype=np.uint8)
        outs = [_np_ptr(out.get(nm)) for nm in ("score", "outcome", "sums", "team", "home_goals", "away_goals")]
        with self._torch.cuda.device(self.device):
            self._check(self._lib.bplhip_ppc(
                self._h, C.byref(q), _np_ptr(hs), _np_ptr(as_), _np_ptr(fid), k, int(max_goals), R, int(key[0]),
                int(key[1]), *outs, self._stream()))
        return out

    def selftest_math(self, which: int, x) -> np.ndarray:
        """The library's short float64 device math on x: 0 exp, 1 log, 2 log1p (x >= 0), 3 1/x."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.empty_like(x)
        with self._torch.cuda.device(self.device):
            self._check(self._lib.bplhip_selftest_math(self._h, int(which), x.size, _np_ptr(x), _np_ptr(out)))
        return out

    def selftest_lanes(self, which: int, f64, f32, i32):
        """One probe of the cross-lane layer (include/bplhip.h: bplhip_selftest_lanes) on arrays of shape
        [n_waves, SELFTEST_CHANNELS, 64]: what every lane holds after the call, as (f64, f32, i32)."""
        f64 = np.ascontiguousarray(f64, dtype=np.float64)
        f32 = np.ascontiguousarray(f32, dtype=np.float32)
        i32 = np.ascontiguousarray(i32, dtype=np.int32)
        if not (f64.shape == f32.shape == i32.shape and f64.ndim == 3 and f64.shape[1:] == (SELFTEST_CHANNELS, 64)):
            raise ValueError("selftest_lanes: arrays of shape [n_waves, %d, 64]" % SELFTEST_CHANNELS)
        if not 0 <= int(which) < SELFTEST_COUNTED_ROWS:
            raise ValueError("selftest_lanes: no such probe")
        out = (np.empty_like(f64), np.empty_like(f32), np.empty_like(i32))
        with self._torch.cuda.device(self.device):
            self._check(self._lib.bplhip_selftest_lanes(self._h, int(which), f64.shape[0], _np_ptr(f64), _np_ptr(f32),
                                                        _np_ptr(i32), *[_np_ptr(o) for o in out]))
        return out

    def selftest_counted_rows(self, values):
        """The counted-row probe of bplhip_selftest_lanes: values[contribution, row] in units of 2^-30 ->
        (words int64 [rows, SELFTEST_GA_WORDS], flags int32 [rows, 4])."""
        v = np.ascontiguousarray(values, dtype=np.float64)
        if v.ndim != 2 or not 1 <= v.shape[0] <= 255 or v.shape[1] < 1:
            raise ValueError("selftest_counted_rows: values[1..255 contributions, rows]")
        words = np.empty((v.shape[1], SELFTEST_GA_WORDS), dtype=np.int64)
        flags = np.empty((v.shape[1], 4), dtype=np.int32)
        n = np.array([v.shape[0]], dtype=np.int32)
        with self._torch.cuda.device(self.device):
            self._check(self._lib.bplhip_selftest_lanes(self._h, SELFTEST_COUNTED_ROWS, v.shape[1], _np_ptr(v), None,
                                                        _np_ptr(n), _np_ptr(words), None, _np_ptr(flags)))
        return words, flags

    # -- sampler
    @staticmethod
    def _stats_buffers(kept: int, d: int):
        out = {
            "potential_energy": np.empty(kept),
            "accept_prob": np.empty(kept),
            "step_size": np.empty(kept),
            "num_steps": np.empty(kept, dtype=np.int32),
            "diverging": np.empty(kept, dtype=np.int32),
            "corr_coef": np.empty(kept),
            "inverse_mass_matrix": np.empty(d),
        }
        st = NutsStats()
        dp = C.POINTER(C.c_double)
        ip = C.POINTER(C.c_int32)
        st.potential_energy = out["potential_energy"].ctypes.data_as(dp)
        st.accept_prob = out["accept_prob"].ctypes.data_as(dp)
        st.step_size = out["step_size"].ctypes.data_as(dp)
        st.num_steps = out["num_steps"].ctypes.data_as(ip)
        st.diverging = out["diverging"].ctypes.data_as(ip)
        st.corr_coef = out["corr_coef"].ctypes.data_as(dp)
        st.inverse_mass_matrix = out["inverse_mass_matrix"].ctypes.data_as(dp)
        return out, st

    @staticmethod
    def _stats_scalars(out, st):
        out.update(
            final_step_size=st.final_step_size,
            mean_accept_prob=st.mean_accept_prob,
            total_leapfrogs=int(st.total_leapfrogs),
            total_divergences=int(st.total_divergences),
            wall_seconds=st.wall_seconds,
        )

    def nuts_run(self, cfg: NutsCfg, key: Tuple[int, int], z0: Optional[np.ndarray] = None):
        kept = cfg.num_samples // cfg.thinning
        d = self.dim
        draws = np.empty((kept, d), dtype=np.float64)
        out, st = self._stats_buffers(kept, d)
        z0c = None if z0 is None else np.ascontiguousarray(z0, dtype=np.float64)
        if z0c is not None and z0c.shape != (d,):
            raise ValueError(f"init_params must have shape ({d},)")
        with self._torch.cuda.device(self.device):
            self._check(
                self._lib.bplhip_nuts_run(
                    self._h, C.byref(cfg), _np_ptr(z0c), key[0], key[1],
                    draws.ctypes.data_as(C.c_void_p), C.byref(st), self._stream(),
                )
            )
        self._stats_scalars(out, st)
        return draws, out

    def nuts_run_chains(self, cfg: NutsCfg, keys, z0: Optional[np.ndarray] = None):
        """Lock-step chains on this GPU (numpyro chain_method="vectorized").  Returns a list
        of (draws, stats) per chain, same content as nuts_run.  Raises BplHipError with
        code EUNSUPPORTED when the bound model cannot run in lock step."""
        n = len(keys)
        kept = cfg.num_samples // cfg.thinning
        d = self.dim
        draws = np.empty((n, kept, d), dtype=np.float64)
        bufs = [self._stats_buffers(kept, d) for _ in range(n)]
        st_arr = (NutsStats * n)()
        for i, (_, st) in enumerate(bufs):
            st_arr[i] = st
        seeds = np.ascontiguousarray(np.asarray(keys, dtype=np.uint32).reshape(n, 2))
        z0c = None if z0 is None else np.ascontiguousarray(z0, dtype=np.float64)
        if z0c is not None:
            if z0c.shape == (d,):
                z0c = np.ascontiguousarray(np.tile(z0c, (n, 1)))
            if z0c.shape != (n, d):
                raise ValueError(f"init_params must have shape ({n}, {d})")
        with self._torch.cuda.device(self.device):
            self._check(
                self._lib.bplhip_nuts_run_chains(
                    self._h, C.byref(cfg), n, _np_ptr(z0c), _np_ptr(seeds),
                    draws.ctypes.data_as(C.c_void_p), st_arr, self._stream(),
                )
            )
        res = []
        for i, (out, _) in enumerate(bufs):
            self._stats_scalars(out, st_arr[i])
            res.append((draws[i], out))
        return res

    def constrain(self, z_draws: np.ndarray):
        z = np.ascontiguousarray(z_draws, dtype=np.float64)
        s, t = z.shape[0], self.n_teams
        attack = np.empty((s, t))
        defence = np.empty((s, t))
        ha = np.empty(s) if self.model == MODEL_BASIC else np.empty((s, t))
        corr = np.empty(s)
        self._check(
            self._lib.bplhip_constrain(
                self._h, _np_ptr(z), s, _np_ptr(attack), _np_ptr(defence), _np_ptr(ha),
                _np_ptr(corr),
            )
        )
        return {"attack": attack, "defence": defence, "home_advantage": ha, "corr_coef": corr}
