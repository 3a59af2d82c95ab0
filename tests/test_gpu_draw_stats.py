"""The per-draw sampler statistics against the float64 oracle evaluated at the draws the device returned
(tests/draw_stats_cases.py): on every engine, `potential_energy[i]` is U(draws[i]) and `corr_coef[i]` is
rho(draws[i]) at the gates of the family's parity test, `num_steps`, `step_size`, `diverging` and the run totals
are consistent, a thinned run keeps the rows nuts.hpp says it keeps, and every chain of a several-chain run carries
its OWN statistics.  The posterior `corr_coef` of the neutral, World-Cup and dynamic classes is this statistic
(bpl/neutral_dixon_coles.py, bpl/dynamic_dixon_coles.py): nothing recomputes it from the draw.

Before each comparison the test asserts from the oracle alone that the comparison could fail: consecutive kept
draws (and the chains of one run) differ by more than 100 gates in U and in rho, so a column shifted by a row, taken
from another leaf of the tree or from another chain cannot pass.

Every run is followed by an assertion on bplhip_last_nuts_engine; options are restored in a `finally`."""
import numpy as np
import pytest

import cases
import dc_oracle as O
import draw_stats_cases as DS
import sampler_cases as SC

pytestmark = pytest.mark.gpu
STATS = ("potential_energy", "accept_prob", "step_size", "num_steps", "diverging", "corr_coef")


def _engine(ctx):
    from bpl import _ffi

    return _ffi.ENGINE_NAMES[ctx.last_nuts_engine()]


def _cfg(shape):
    from bpl._ffi import default_nuts_cfg

    cfg = default_nuts_cfg()
    cfg.num_warmup, cfg.num_samples, cfg.thinning = shape["num_warmup"], shape["num_samples"], shape["thinning"]
    cfg.max_tree_depth = shape["max_tree_depth"]
    if shape["step_size"] is not None:
        cfg.step_size = shape["step_size"]
    return cfg


def _run(ctx, cfg, opts, engine, keys, z0):
    """[(draws, stats)] per chain under `opts` (restored after the run), the engine asserted."""
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        out = [ctx.nuts_run(cfg, keys[0], z0[0])] if len(keys) == 1 else ctx.nuts_run_chains(cfg, keys, z0)
        assert _engine(ctx) == engine
    finally:
        for k in opts:
            ctx.set_option(k, 1)
    return out


def _bind_league(ctx, case):
    fx = SC.fixtures(case)
    cov = O.standardise_covariates(fx.covariates) if case.K else None
    ctx.set_fixtures(case.model, fx.home_idx.astype(np.uint16), fx.away_idx.astype(np.uint16),
                     fx.home_goals.astype(np.uint8), fx.away_goals.astype(np.uint8), fx.n_teams,
                     weights=fx.weights.astype(np.float32) if case.weighted else None, covariates_std=cov)
    assert ctx.dim == case.D


def _bind_venue(ctx, family, fx, random_walk):
    import dc_dynamic_oracle as DO
    import dc_neutral_oracle as NO

    if family == "neutral":
        cov = None if fx.covariates is None else NO.standardise_covariates(fx.covariates)
        ctx.set_fixtures_neutral(fx.home_idx, fx.away_idx, fx.home_goals, fx.away_goals, fx.neutral, fx.n_teams,
                                 weights=fx.weights.astype(np.float32), covariates_std=cov, home_conf=fx.home_conf,
                                 away_conf=fx.away_conf, n_conf=fx.n_conf)
    else:
        cov = None if fx.covariates is None else DO.standardise_covariates(fx.covariates)
        ctx.set_fixtures_dynamic(fx.home_idx, fx.away_idx, fx.home_goals, fx.away_goals, fx.gameweek, fx.neutral,
                                 fx.n_teams, fx.n_gameweeks, covariates_std=cov, random_walk=random_walk)
    assert ctx.dim == DS.venue_dim(family, fx)


def _check_chain(tag, family, at, n_fixtures, cfg, draws, st, sensitive=True):
    """One chain's per-draw statistics against the oracle at its own draws.  Returns the oracle's U column."""
    kept = cfg.num_samples // cfg.thinning
    assert draws.shape[0] == kept and all(st[nm].shape == (kept,) for nm in STATS)
    U, rho = DS.oracle_columns(at, draws)
    if sensitive:
        fu, fr = DS.sensitivity(family, n_fixtures, U, rho)
        print(f"{tag}: consecutive kept pairs apart by > {DS.SENSITIVITY:g} gates: U {fu:.2f}, rho {fr:.2f}")
        assert fu >= DS.MIN_FRACTION and fr >= DS.MIN_FRACTION, (tag, fu, fr)
    gate = np.array([DS.u_gate(family, n_fixtures, u) for u in U])
    du, dr = np.abs(st["potential_energy"] - U), np.abs(st["corr_coef"] - rho)
    print(f"{tag}: max |dU| / gate {np.max(du / gate):.3g}, max |drho| {dr.max():.3g} (gate {DS.RHO_GATE[family]:g}), "
          f"tree sizes {st['num_steps'].tolist()}, diverging {int(st['diverging'].sum())}")
    assert (du <= gate).all(), (tag, np.argmax(du / gate), (du / gate).max())
    assert (dr <= DS.RHO_GATE[family]).all(), (tag, int(np.argmax(dr)), dr.max())
    assert st["num_steps"].min() >= 1 and st["num_steps"].max() <= 2 ** cfg.max_tree_depth - 1
    assert set(np.unique(st["diverging"]).tolist()) <= {0, 1}
    assert ((st["accept_prob"] >= 0) & (st["accept_prob"] <= 1)).all()
    if cfg.num_warmup == 0:
        assert np.array_equal(st["step_size"], np.full(kept, cfg.step_size))
        if cfg.thinning == 1:
            assert int(st["num_steps"].sum()) == st["total_leapfrogs"]
            assert int(st["diverging"].sum()) == st["total_divergences"]
            assert abs(st["mean_accept_prob"] - st["accept_prob"].mean()) <= 1e-13   # (a running mean of <= 14 terms)
    else:
        assert np.array_equal(st["step_size"], np.full(kept, st["final_step_size"]))
        assert st["total_leapfrogs"] >= int(st["num_steps"].sum()) and st["total_divergences"] >= int(st["diverging"].sum())
    return U


def _check_run(tag, family, at, n_fixtures, cfg, chains):
    cols = [_check_chain(f"{tag} chain {c}", family, at, n_fixtures, cfg, d, st) for c, (d, st) in enumerate(chains)]
    for a in range(len(cols)):   # the chains differ: a statistic taken from a neighbour cannot pass
        for b in range(a + 1, len(cols)):
            gate = max(DS.u_gate(family, n_fixtures, u) for u in np.concatenate([cols[a], cols[b]]))
            apart = float((np.abs(cols[a] - cols[b]) > DS.SENSITIVITY * gate).mean())
            assert apart >= DS.MIN_FRACTION, (tag, a, b, apart)


# ------------------------------------------------------------------------------------------------- the league
@pytest.mark.parametrize("engine,name,setting", DS.league_single_runs())
def test_league_chain_statistics_belong_to_their_draws(hip_ctx, engine, name, setting):
    case = SC.CASES[name]
    _bind_league(hip_ctx, case)
    at, n = DS.league_oracle(case)
    for label, shape in (("fixed", DS.league_fixed(case)), ("adapted", DS.ADAPTED)):
        cfg = _cfg(shape)
        chains = _run(hip_ctx, cfg, SC.OPTIONS[setting], engine, [DS.KEY], [SC.start(case)])
        _check_run(f"{engine} {name} {label}", "league", at, n, cfg, chains)


@pytest.mark.parametrize("engine,name,nch,opts", DS.league_chain_runs())
def test_league_chains_carry_their_own_statistics(hip_ctx, engine, name, nch, opts):
    case = SC.CASES[name]
    _bind_league(hip_ctx, case)
    at, n = DS.league_oracle(case)
    keys, z0 = DS.chain_inputs(case.D, nch)
    for label, shape in (("fixed", DS.FIXED), ("adapted", DS.ADAPTED)):
        cfg = _cfg(shape)
        _check_run(f"{engine} {name} x{nch} {label}", "league", at, n, cfg, _run(hip_ctx, cfg, opts, engine, keys, z0))


# ------------------------------------------------------------------------------------------- neutral and dynamic
@pytest.mark.parametrize("family,fixture,random_walk,opts,engine,nch", DS.VENUE_RUNS)
def test_venue_chain_statistics_belong_to_their_draws(hip_ctx, family, fixture, random_walk, opts, engine, nch):
    fx = DS.neutral_fixture(fixture) if family == "neutral" else DS.dynamic_fixture(fixture)
    _bind_venue(hip_ctx, family, fx, random_walk)
    at, n = DS.venue_oracle(family, fx, random_walk)
    keys, z0 = DS.chain_inputs(hip_ctx.dim, nch)
    for label, shape in (("fixed", dict(DS.FIXED, step_size=DS.VENUE_STEP[family])), ("adapted", DS.ADAPTED)):
        cfg = _cfg(shape)
        chains = _run(hip_ctx, cfg, opts, engine, keys, z0)
        _check_run(f"{engine} {family} {fixture} rw={random_walk} x{nch} {label}", family, at, n, cfg, chains)


# ------------------------------------------------------------------------------------------- thinning alignment
def _assert_thinned_rows(tag, one, thin, rows, bitwise):
    (d1, s1), (d3, s3) = one, thin
    print(f"{tag}: rows {rows}, max |d draw| {np.abs(d3 - d1[rows]).max():.3g}")
    if bitwise:
        assert np.array_equal(d3, d1[rows])
        for nm in STATS:
            assert np.array_equal(s3[nm], s1[nm][rows]), nm
    else:   # the gates tests/test_gpu_dynamic.py puts between chains run together and alone
        assert np.abs(d3[:3] - d1[rows][:3]).max() < 1e-8 and np.abs(d3 - d1[rows]).max() < 1e-3
        assert s3["num_steps"][:3].tolist() == s1["num_steps"][rows][:3].tolist()
        assert np.abs(s3["potential_energy"][:3] - s1["potential_energy"][rows][:3]).max() < 1e-6
        assert np.abs(s3["corr_coef"][:3] - s1["corr_coef"][rows][:3]).max() < 1e-8


@pytest.mark.parametrize("engine,name,setting", [r for r in DS.league_single_runs() if SC.CASES[r[1]].tail])
def test_thinned_league_run_keeps_the_rows_of_the_full_run(hip_ctx, engine, name, setting):
    """nuts.hpp ChainDriver::end: start_idx = num_warmup + num_samples % thinning; iteration `it` is kept when
    it >= start_idx and (it - start_idx) % thinning == thinning - 1, as row (it - start_idx) / thinning.  A
    thinning = 3 run of 14 samples therefore holds iterations 14 % 3 + 3 j + 2 = 4, 7, 10, 13 of the thinning = 1 run
    with the same key and start: the draws and all six per-draw statistics, bit for bit (these engines repeat a run
    bit for bit, which is asserted first)."""
    case = SC.CASES[name]
    _bind_league(hip_ctx, case)
    rows = DS.kept_rows(DS.THIN["num_samples"], DS.THIN["thinning"])
    assert rows == [14 % 3 + 3 * j + 2 for j in range(4)] == [4, 7, 10, 13]
    args = (SC.OPTIONS[setting], engine, [DS.KEY], [SC.start(case)])
    one = _run(hip_ctx, _cfg(dict(DS.THIN, thinning=1)), *args)[0]
    again = _run(hip_ctx, _cfg(dict(DS.THIN, thinning=1)), *args)[0]
    assert np.array_equal(one[0], again[0]) and all(np.array_equal(one[1][nm], again[1][nm]) for nm in STATS)
    assert len({one[1]["potential_energy"][r] for r in range(14)}) >= 12   # the rows can be told apart
    thin = _run(hip_ctx, _cfg(DS.THIN), *args)[0]
    _assert_thinned_rows(f"{engine} {name}", one, thin, rows, bitwise=True)


@pytest.mark.parametrize("family,fixture,random_walk,opts,engine,nch", [r for r in DS.VENUE_RUNS if r[-1] == 1])
def test_thinned_venue_run_keeps_the_rows_of_the_full_run(hip_ctx, family, fixture, random_walk, opts, engine, nch):
    """The same rows for the neutral and the dynamic model, whose evaluations add with float64 atomics in arbitrary
    order: at the gates tests/test_gpu_dynamic.py puts between chains run together and alone."""
    fx = DS.neutral_fixture(fixture) if family == "neutral" else DS.dynamic_fixture(fixture)
    _bind_venue(hip_ctx, family, fx, random_walk)
    keys, z0 = DS.chain_inputs(hip_ctx.dim, 1)
    shape = dict(DS.THIN, step_size=DS.VENUE_STEP[family])
    one = _run(hip_ctx, _cfg(dict(shape, thinning=1)), opts, engine, keys, z0)[0]
    thin = _run(hip_ctx, _cfg(shape), opts, engine, keys, z0)[0]
    assert len({one[1]["potential_energy"][r] for r in range(14)}) >= 12
    _assert_thinned_rows(f"{engine} {family} {fixture}", one, thin, DS.kept_rows(14, 3), bitwise=False)


# ------------------------------------------------------------------------------------------ divergent transitions
@pytest.mark.parametrize("engine,opts,nch", DS.DIVERGENT_ENGINES)
def test_divergent_transitions_keep_the_statistics_of_the_kept_point(hip_ctx, engine, opts, nch):
    """Divergences that a large fixed step brings about on the basic dummy league (draw_stats_cases.py: why no
    candidate step gives both kinds in one run).  Step 0.5: every transition diverges at its first leaf, the draw
    equals its predecessor and the statistics are those of that point.  Step 0.0625 from a typical point: the trees
    are cut short by a divergence after a few leapfrogs and some accept an inner leaf."""
    from bpl._ffi import default_nuts_cfg

    fx = cases.fixtures("dummy")
    hip_ctx.set_fixtures(O.MODEL_BASIC, fx.home_idx.astype(np.uint16), fx.away_idx.astype(np.uint16),
                         fx.home_goals.astype(np.uint8), fx.away_goals.astype(np.uint8), fx.n_teams)
    assert hip_ctx.dim == DS.DIVERGENT_START.size == 45

    def at(z):
        U, _, aux = O.potential_and_grad(O.MODEL_BASIC, fx, z)
        return U, aux["rho"]

    keys = [(DS.KEY[0], DS.KEY[1] + c) for c in range(nch)]
    for step, z0 in ((DS.DIVERGENT_FIRST_LEAF, DS.chain_inputs(45, nch)[1]),
                     (DS.DIVERGENT_LATER, np.stack([DS.DIVERGENT_START + 0.01 * c for c in range(nch)]))):
        cfg = default_nuts_cfg()
        cfg.num_warmup, cfg.num_samples, cfg.max_tree_depth, cfg.step_size = 0, DS.DIVERGENT_TRANSITIONS, 5, step
        for c, (d, st) in enumerate(_run(hip_ctx, cfg, opts, engine, keys, z0)):
            tag = f"{engine} x{nch} step {step} chain {c}"
            _check_chain(tag, "league", at, fx.n, cfg, d, st, sensitive=False)
            prev = np.vstack([z0[c][None], d[:-1]])
            moved = (d != prev).any(axis=1)
            print(f"{tag}: diverging {st['diverging'].tolist()} moved {moved.astype(int).tolist()}")
            first_leaf = (st["diverging"] == 1) & (st["num_steps"] == 1)
            assert not moved[first_leaf].any()
            assert st["diverging"].sum() >= 2
            if step == DS.DIVERGENT_FIRST_LEAF:
                assert first_leaf.all() and st["num_steps"].tolist() == DS.DIVERGENT_TREE_SIZES[step]
                assert np.array_equal(d, np.tile(z0[c], (cfg.num_samples, 1)))
            elif c == 0:   # the chain the restatement walked
                assert st["diverging"].tolist() == DS.DIVERGENT_LATER_FLAGS
                assert st["num_steps"].tolist() == DS.DIVERGENT_LATER_TREE_SIZES
                assert moved.astype(int).tolist() == DS.DIVERGENT_LATER_MOVED
