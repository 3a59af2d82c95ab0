"""The samplers on the edges of the forms the host picks from the latent size, the covariate count, the weights and
the chain count (tests/sampler_cases.py; tests/test_sampler_cases_host.py keeps every case on its edge):

  a. every engine against the independent NUTS restatement on the float64 C potential (tests/golden/nuts_edge_*.npz,
     oracle/make_nuts_golden.py), at the gates of tests/test_gpu_nuts_golden.py;
  b. the host tree against every device engine on the same fixed-step run, at the gates of
     tests/test_gpu_fit.py::test_device_tree_matches_host_tree (leaf in dc_eval's tail) and
     tests/test_gpu_parity.py::test_nuts_with_many_teams (kp_leaf / kw_leaf);
  c. the persistent kernel against one launch per leapfrog, and persist_spec 1 against 0, bit for bit through an adapted
     chain (tests/test_gpu_soak.py) -- the register leaf of dc_eval_loop<.., 2> against the LDS-staged leaf;
  d. several chains against single chains at the gates of test_lockstep_chains_match_single_chains, and chain 0
     bit for bit when only its neighbours change.

Every run is followed by an assertion on bplhip_last_nuts_engine: a case that stops reaching its form fails here.
The fixed-step runs are made once per (case, engine, step) and shared by a. and b.
"""
import os

import numpy as np
import pytest

import dc_oracle as O
import sampler_cases as SC

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BINDABLE = [c.name for c in SC.ALL if c.bindable]
_RUNS = {}     # (case, setting, step) -> (draws, stats, engine name)


def _bind(ctx, case):
    fx = SC.fixtures(case)
    cov = O.standardise_covariates(fx.covariates) if case.K else None
    w32 = fx.weights.astype(np.float32) if case.weighted else None
    ctx.set_fixtures(case.model, fx.home_idx.astype(np.uint16), fx.away_idx.astype(np.uint16),
                     fx.home_goals.astype(np.uint8), fx.away_goals.astype(np.uint8), fx.n_teams,
                     weights=w32, covariates_std=cov)
    assert ctx.dim == case.D and _engine(ctx) == "NONE"


def _engine(ctx):
    from bpl import _ffi

    return _ffi.ENGINE_NAMES[ctx.last_nuts_engine()]


class _options:
    """Options set for the block, their defaults (1) restored after it."""

    def __init__(self, ctx, opts):
        self.ctx, self.opts = ctx, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.ctx.set_option(k, 1)


def _settings(case):
    """The settings that reach different engines for the case (past dc_eval's tail persistent_nuts = 0 and
    persistent_kernel = 0 change nothing: the library has no device tree there)."""
    return ("persistent", "kernel0", "device", "host") if case.tail else ("persistent", "host")


def _fixed(ctx, case, setting, step=SC.STEP):
    """The golden's fixed-step run under `setting` (bound by the caller), made once."""
    from bpl._ffi import default_nuts_cfg

    k = (case.name, setting, step)
    if k not in _RUNS:
        cfg = default_nuts_cfg()
        cfg.num_warmup, cfg.num_samples, cfg.step_size = 0, SC.TRANSITIONS, step
        with _options(ctx, SC.OPTIONS[setting]):
            d, st = ctx.nuts_run(cfg, SC.KEY, SC.start(case))
            _RUNS[k] = (d, st, _engine(ctx))
    return _RUNS[k]


def _golds(case):
    out = [(SC.STEP, np.load(os.path.join(GOLD, f"nuts_edge_{case.name}.npz")))]
    if case.name in SC.FINE:
        out.append((SC.FINE_STEP, np.load(os.path.join(GOLD, f"nuts_edge_{case.name}_fine.npz"))))
    return out


# ---------------------------------------------------------------------------------------------- a. the oracle
@pytest.mark.parametrize("name", BINDABLE)
def test_fixed_step_chain_follows_the_oracle(hip_ctx, name):
    case = SC.CASES[name]
    _bind(hip_ctx, case)
    for step, g in _golds(case):
        assert float(g["step_size0"]) == step and np.array_equal(g["z0"], SC.start(case))
        for setting in _settings(case):
            d, st, engine = _fixed(hip_ctx, case, setting, step)
            print(name, setting, engine, "step", step, "tree sizes", st["num_steps"].tolist(), "oracle",
                  g["num_steps"].tolist(), "max |d draw| per transition", np.abs(d - g["draws"]).max(axis=1))
            assert engine == case.engine(setting)
            assert st["num_steps"][:5].tolist() == g["num_steps"][:5].tolist()
            assert np.abs(d[:3] - g["draws"][:3]).max() < 1e-5
            assert np.abs(st["accept_prob"][:3] - g["accept_prob"][:3]).max() < 1e-5
            assert np.abs(st["potential_energy"][:3] - g["potential_energy"][:3]).max() < 1e-3
            assert np.allclose(st["step_size"], step)


@pytest.mark.parametrize("name", [n for n in SC.ADAPTED if SC.CASES[n].bindable])
def test_adapted_chain_follows_the_oracle(hip_ctx, name):
    """The weighted persistent-loop instantiations through a warm-up of trees of at most 3 leapfrogs
    (tests/test_gpu_nuts_golden.py::test_adapted_chain_follows_the_oracle, its gates)."""
    from bpl._ffi import default_nuts_cfg

    case = SC.CASES[name]
    g = np.load(os.path.join(GOLD, f"nuts_edge_{name}_adapt_shallow.npz"))
    _bind(hip_ctx, case)
    cfg = default_nuts_cfg()
    w = int(g["num_warmup"])
    cfg.num_warmup, cfg.num_samples, cfg.step_size = w, int(g["num_samples"]), 1.0
    cfg.max_tree_depth = int(g["max_tree_depth"])
    for setting in _settings(case):
        with _options(hip_ctx, SC.OPTIONS[setting]):
            d, st = hip_ctx.nuts_run(cfg, tuple(int(k) for k in g["key"]), g["z0"])
            assert _engine(hip_ctx) == case.engine(setting)
        print(name, setting, st["num_steps"].tolist(), g["num_steps"][w:].tolist(), st["final_step_size"],
              float(g["final_step_size"]), st["total_leapfrogs"], int(g["num_steps"].sum()), np.abs(d - g["draws"]).max())
        assert st["total_leapfrogs"] == int(g["num_steps"].sum())
        assert st["num_steps"].tolist() == g["num_steps"][w:].tolist()
        assert abs(st["final_step_size"] / float(g["final_step_size"]) - 1) < 1e-4
        assert np.abs(st["inverse_mass_matrix"] / g["inverse_mass_matrix"] - 1).max() < 1e-4
        assert np.abs(d - g["draws"]).max() < 1e-4


def test_weighted_basic_model_is_refused(hip_ctx):
    """b65w (basic model, weights) exists in the oracle only: bplhip_set_fixtures refuses weights for the basic model,
    as the reference's basic model has none, so dc_eval_loop<true, false, *> is never launched.  Should the library
    ever take such fixtures this fails, and b65w joins the other cases."""
    from bpl._ffi import BPLHIP_EINVAL, BplHipError

    case = SC.CASES["b65w"]
    assert not case.bindable
    with pytest.raises(BplHipError) as e:
        _bind(hip_ctx, case)
    assert e.value.code == BPLHIP_EINVAL and "weights" in str(e.value)
    assert _engine(hip_ctx) == "NONE"


# ---------------------------------------------------------------------------------------------- b. engine against engine
@pytest.mark.parametrize("name", BINDABLE)
def test_device_engines_match_the_host_tree(hip_ctx, name):
    case = SC.CASES[name]
    _bind(hip_ctx, case)
    for step, _ in _golds(case):
        d0, s0, e0 = _fixed(hip_ctx, case, "host", step)
        assert e0 == "HOST_TREE"
        for setting in _settings(case)[:-1]:
            d1, s1, e1 = _fixed(hip_ctx, case, setting, step)
            assert e1 == case.engine(setting) != "HOST_TREE"
            print(name, setting, e1, "step", step, s1["num_steps"].tolist(), "max |d draw| per transition",
                  np.abs(d1 - d0).max(axis=1), "max |d accept|", np.abs(s1["accept_prob"] - s0["accept_prob"]).max())
            assert s1["num_steps"].tolist() == s0["num_steps"].tolist()
            if case.tail:
                assert s1["total_leapfrogs"] == s0["total_leapfrogs"]
                assert np.abs(d1[:4] - d0[:4]).max() < 1e-10
                assert np.abs(s1["potential_energy"][:4] - s0["potential_energy"][:4]).max() < 1e-8
                assert np.abs(s1["accept_prob"][:4] - s0["accept_prob"][:4]).max() < 1e-9
            else:
                assert np.abs(d1[:3] - d0[:3]).max() < 1e-9
                assert np.abs(s1["accept_prob"][:3] - s0["accept_prob"][:3]).max() < 1e-8


# ---------------------------------------------------------------------------------------------- c. bit for bit
def _adapted_pair(ctx, case, option):
    from bpl._ffi import default_nuts_cfg

    _bind(ctx, case)
    cfg = default_nuts_cfg()
    cfg.num_warmup, cfg.num_samples = 60, 40
    runs = {}
    for v in (1, 0):
        with _options(ctx, {option: v}):
            runs[v] = ctx.nuts_run(cfg, (0, 11)) + (_engine(ctx),)
    return runs


def _assert_same_chain(a, b):
    (d1, s1), (d0, s0) = a, b
    print("leapfrogs", s1["total_leapfrogs"], s0["total_leapfrogs"], "first differing draw",
          int(np.argmax((d1 != d0).any(axis=1))) if (d1 != d0).any() else None, "max |d draw|", np.abs(d1 - d0).max())
    assert s1["total_leapfrogs"] == s0["total_leapfrogs"] > 100
    assert np.array_equal(s1["num_steps"], s0["num_steps"])
    assert np.array_equal(s1["potential_energy"], s0["potential_energy"])
    assert np.array_equal(d1, d0)


@pytest.mark.parametrize("name", [n for n in SC.BITWISE if SC.CASES[n].bindable])
def test_persistent_kernel_walks_the_per_launch_chain(hip_ctx, name):
    """persistent_kernel 1 against 0 through warm-up and sampling: nuts_dev.hip.h's claim that the staged leaf and
    the register leaf walk the same trajectory bit for bit, at one and at two elements per lane."""
    case = SC.CASES[name]
    runs = _adapted_pair(hip_ctx, case, "persistent_kernel")
    assert runs[1][2] == case.engine("persistent") and runs[0][2] == case.engine("kernel0") == "PERSIST_TAIL"
    _assert_same_chain(runs[1][:2], runs[0][:2])


@pytest.mark.parametrize("name", SC.SPEC)
def test_leaf_one_step_behind_is_bitwise_neutral(hip_ctx, name):
    case = SC.CASES[name]
    runs = _adapted_pair(hip_ctx, case, "persist_spec")
    assert runs[1][2] == runs[0][2] == case.engine("persistent") == "LOOP_LNE2"
    _assert_same_chain(runs[1][:2], runs[0][:2])


# ---------------------------------------------------------------------------------------------- d. several chains
_SINGLES = {}
N_MAX = max(SC.MULTI_CHAINS)


def _chain_inputs(case):
    z0 = np.random.RandomState(2).uniform(-0.2, 0.2, (N_MAX, case.D))
    return [(0, 11 + c) for c in range(N_MAX)], z0


def _cfg():
    from bpl._ffi import default_nuts_cfg

    cfg = default_nuts_cfg()
    cfg.num_warmup, cfg.num_samples, cfg.step_size = 0, SC.TRANSITIONS, SC.STEP
    return cfg


def _single(ctx, case, c):
    """Chain c of the case on its own (bound by the caller), made once."""
    if (case.name, c) not in _SINGLES:
        keys, z0 = _chain_inputs(case)
        _SINGLES[case.name, c] = ctx.nuts_run(_cfg(), keys[c], z0[c])
        assert _engine(ctx) == case.engine("persistent")
    return _SINGLES[case.name, c]


def _assert_chains_match_singles(ctx, case, multi):
    for c, (dm, sm) in enumerate(multi):
        d1, s1 = _single(ctx, case, c)
        assert sm["num_steps"][:3].tolist() == s1["num_steps"][:3].tolist(), c
        assert np.abs(dm[:3] - d1[:3]).max() < 1e-5, c
        assert np.abs(sm["potential_energy"][:3] - s1["potential_energy"][:3]).max() < 1e-4, c


@pytest.mark.parametrize("nch", SC.MULTI_CHAINS)
@pytest.mark.parametrize("name", SC.MULTI)
def test_chains_match_single_chains(hip_ctx, name, nch):
    case = SC.CASES[name]
    _bind(hip_ctx, case)
    keys, z0 = _chain_inputs(case)
    multi = hip_ctx.nuts_run_chains(_cfg(), keys[:nch], z0[:nch])
    assert _engine(hip_ctx) == SC.chains_engine(case.T, case.D, nch) == \
        ("PERSIST_GRIDY" if nch <= SC.GRIDY_MAX_CHAINS else "PERSIST_VEC")
    _assert_chains_match_singles(hip_ctx, case, multi)
    if nch >= SC.GRIDY_MAX_CHAINS:
        # chain 0 does not depend on its neighbours: other keys and starts for them, the same chain bit for bit
        keys2 = keys[:1] + [(3, 100 + c) for c in range(1, nch)]
        z2 = z0[:nch].copy()
        z2[1:] = np.random.RandomState(9).uniform(-0.2, 0.2, (nch - 1, case.D))
        other = hip_ctx.nuts_run_chains(_cfg(), keys2, z2)
        assert _engine(hip_ctx) == SC.chains_engine(case.T, case.D, nch)
        assert np.abs(other[1][0] - multi[1][0]).max() > 1e-3
        assert np.array_equal(other[0][0], multi[0][0])
        assert np.array_equal(other[0][1]["potential_energy"], multi[0][1]["potential_energy"])
        assert np.array_equal(other[0][1]["num_steps"], multi[0][1]["num_steps"])


@pytest.mark.parametrize("option,engine", [("persistent_nuts", "LOCKSTEP_VEC"), ("chunk_graph", "PERSIST_VEC")])
def test_lockstep_and_ungraphed_chains_match_single_chains(hip_ctx, option, engine):
    case = SC.CASES["e128w"]
    _bind(hip_ctx, case)
    keys, z0 = _chain_inputs(case)
    with _options(hip_ctx, {option: 0}):
        multi = hip_ctx.nuts_run_chains(_cfg(), keys, z0)
        assert _engine(hip_ctx) == engine == SC.chains_engine(case.T, case.D, N_MAX, int(option != "persistent_nuts"))
    _assert_chains_match_singles(hip_ctx, case, multi)
