"""GPU: every form of the neutral-venue and dynamic evaluation kernels against the float64 oracles, on inputs
built to reach that form (tests/eval_path_cases.py; tests/test_eval_path_cases_host.py keeps them there), with
the form that actually ran asserted through bplhip_last_eval_path.

Tolerances are those of tests/test_gpu_neutral.py (|dU| <= 1e-11 |U|, |dg|_inf <= 1e-10 |g|_inf, aux 1e-12) and
tests/test_gpu_dynamic.py (1e-9, 1e-9, aux 1e-12).  Each case prints one line per evaluation: the form, dU, dg.
"""
import numpy as np
import pytest

import dc_dynamic_oracle as DO
import dc_neutral_oracle as NO
import eval_path_cases as E

pytestmark = pytest.mark.gpu

DEFAULTS = {"fused_small": 1, "dyn_big_wgs": 0, "neu_runs": 1, "dyn_gather": 1}
NEUTRAL = E.neutral_cases()
DYNAMIC = E.dynamic_cases()


def _restore(ctx):
    for name, value in DEFAULTS.items():
        ctx.set_option(name, value)


def _path_name(ctx):
    from bpl import _ffi

    return _ffi.PATH_NAMES[ctx.last_eval_path()]


def _eval(ctx, z):
    import torch

    U, g, aux = ctx.logp_grad(torch.tensor(z, dtype=torch.float64, device=ctx.device))
    path = _path_name(ctx)   # (host bookkeeping of the launch just enqueued)
    return float(U.cpu()[0]), g.cpu().numpy(), aux.cpu().numpy()[0], path


@pytest.mark.parametrize("case", NEUTRAL, ids=[c.name for c in NEUTRAL])
def test_neutral_form_matches_oracle(hip_ctx, case):
    fx = case.fx
    fx.weights = fx.weights.astype(np.float32).astype(np.float64)  # what the device holds
    refs = [(seed, z) + NO.potential_and_grad(fx, z) for seed, _, z in E.neutral_points(case)]
    sl = NO.site_slices(fx.n_teams, fx.k, fx.n_conf)
    # the other form on the same binding and back: each must find the scratch and the tickets left clean
    rounds = [(1, case.path)]
    if case.path == "NEU_BIG_RUNS":
        rounds += [(0, "NEU_BIG_FIXTURE"), (1, "NEU_BIG_RUNS")]
    try:
        cov = None if fx.covariates is None else NO.standardise_covariates(fx.covariates)
        hip_ctx.set_fixtures_neutral(fx.home_idx, fx.away_idx, fx.home_goals, fx.away_goals, fx.neutral,
                                     fx.n_teams, weights=fx.weights.astype(np.float32), covariates_std=cov,
                                     home_conf=fx.home_conf, away_conf=fx.away_conf, n_conf=fx.n_conf)
        assert hip_ctx.dim == NO.latent_dim(fx.n_teams, fx.k, fx.n_conf)
        assert _path_name(hip_ctx) == "NONE"
        hip_ctx.set_option("dyn_big_wgs", case.wgs)
        for neu_runs, want in rounds:
            hip_ctx.set_option("neu_runs", neu_runs)
            for seed, z, Uo, go, auxo in refs:
                U, g, aux, path = _eval(hip_ctx, z)
                print(f"{case.name:26s} neu_runs={neu_runs} seed={seed} path={path:16s} N={fx.n:6d} U={Uo:.6f} "
                      f"dU={U - Uo:+.2e} dg={np.abs(g - go).max():.2e} |g|={np.abs(go).max():.2e}")
                assert path == want
                assert abs(U - Uo) <= 1e-11 * abs(Uo)
                assert np.abs(g - go).max() <= 1e-10 * np.abs(go).max()
                assert abs(aux[0] - auxo["rho"]) <= 1e-12
                assert abs(aux[1] - auxo["LB"]) <= 1e-12 and abs(aux[2] - auxo["UB"]) <= 1e-12
                if case.name == "far_records":   # |g|_inf is a prior gradient of ~8000 there: each per-team block by its own
                    for nm, s in sl.items():
                        if s.stop - s.start == fx.n_teams:
                            err, top = np.abs(g[s] - go[s]).max(), np.abs(go[s]).max()
                            print(f"    {nm:26s} dg={err:.2e} |g|={top:.2e}")
                            assert err <= 1e-10 * top, nm
    finally:
        _restore(hip_ctx)


@pytest.mark.parametrize("random_walk", [True, False])
@pytest.mark.parametrize("case", DYNAMIC, ids=[c.name for c in DYNAMIC])
def test_dynamic_form_matches_oracle(hip_ctx, case, random_walk):
    fx = case.fx
    refs = [(seed, z) + DO.potential_and_grad(fx, z, random_walk) for seed, z in E.dynamic_points(case)]
    # gather -> atomics -> gather on the same binding (a list too long for the gather stays with the atomics)
    rounds = [(1, case.path), (0, "DYN_FUSED_ATOMICS"), (1, case.path)]
    try:
        hip_ctx.set_fixtures_dynamic(fx.home_idx, fx.away_idx, fx.home_goals, fx.away_goals, fx.gameweek,
                                     fx.neutral, fx.n_teams, fx.n_gameweeks, random_walk=random_walk)
        assert hip_ctx.dim == DO.latent_dim(fx.n_gameweeks, fx.n_teams, fx.k)
        assert _path_name(hip_ctx) == "NONE"
        for gather, want in rounds:
            hip_ctx.set_option("dyn_gather", gather)
            for seed, z, Uo, go, auxo in refs:
                U, g, aux, path = _eval(hip_ctx, z)
                print(f"{case.name:14s} rw={int(random_walk)} dyn_gather={gather} seed={seed} path={path:18s} U={Uo:.6f} "
                      f"dU={U - Uo:+.2e} dg={np.abs(g - go).max():.2e} |g|={np.abs(go).max():.2e}")
                assert path == want
                assert abs(U - Uo) <= 1e-9 * abs(Uo)
                assert np.abs(g - go).max() <= 1e-9 * np.abs(go).max()
                assert abs(aux[0] - auxo["rho"]) <= 1e-12
                assert abs(aux[1] - auxo["LB"]) <= 1e-12 and abs(aux[2] - auxo["UB"]) <= 1e-12
    finally:
        _restore(hip_ctx)


def test_remaining_forms_report_themselves(hip_ctx):
    """The forms the other files already compare with the oracles, named: the neutral single workgroup, both
    models' four launches, the dynamic sliced launch, and the last chain's form of a batched call."""
    import torch

    try:
        fx = NO.fixtures_from_data(NO.neutral_dummy_recipe())
        hip_ctx.set_fixtures_neutral(fx.home_idx, fx.away_idx, fx.home_goals, fx.away_goals, fx.neutral,
                                     fx.n_teams, weights=fx.weights.astype(np.float32))
        z = np.random.RandomState(1).uniform(-0.2, 0.2, hip_ctx.dim)
        assert _eval(hip_ctx, z)[3] == "NEU_FUSED"
        hip_ctx.set_option("fused_small", 0)
        assert _eval(hip_ctx, z)[3] == "NEU_MULTI"
        hip_ctx.set_option("fused_small", 1)
        c = DYNAMIC[0]
        d = c.fx
        hip_ctx.set_fixtures_dynamic(d.home_idx, d.away_idx, d.home_goals, d.away_goals, d.gameweek, d.neutral,
                                     d.n_teams, d.n_gameweeks)
        _, z = next(E.dynamic_points(c))
        Uo, go, _ = DO.potential_and_grad(d, z)
        hip_ctx.set_option("fused_small", 0)
        assert _eval(hip_ctx, z)[3] == "DYN_MULTI"
        hip_ctx.set_option("fused_small", 1)
        hip_ctx.set_option("dyn_big_wgs", 5)
        assert _eval(hip_ctx, z)[3] == "DYN_SLICED"
        hip_ctx.set_option("dyn_big_wgs", 0)
        zb = torch.tensor(np.stack([z, z, z]), dtype=torch.float64, device=hip_ctx.device)
        Ub, gb, _ = hip_ctx.logp_grad(zb)
        assert _path_name(hip_ctx) == c.path
        assert np.abs(Ub.cpu().numpy() - Uo).max() <= 1e-9 * abs(Uo)
        assert np.abs(gb.cpu().numpy() - go).max() <= 1e-9 * np.abs(go).max()
    finally:
        _restore(hip_ctx)
