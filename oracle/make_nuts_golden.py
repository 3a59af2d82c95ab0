"""TEST INFRASTRUCTURE: writes tests/golden/nuts_*.npz from the independent NUTS restatement
(oracle/nuts_oracle.py) on (i) a diagonal Gaussian and (ii) the reference's dummy_data recipe
(tests/conftest.py:7-29) with the float64 C restatement of the Dixon-Coles potential.  Each file
holds the inputs (key, z0, step size, counts) and the oracle's trajectory: draws, tree sizes,
acceptance statistics, energies, step sizes.  (iii) nuts_edge_<case>.npz for every case of tests/sampler_cases.py,
each saved only after a conditioning check of its inputs (edge_check).  Run: python oracle/make_nuts_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "tests")]
import cases  # noqa: E402
import dc_oracle as O  # noqa: E402
import dc_oracle_c as OC  # noqa: E402
import nuts_oracle as NO  # noqa: E402
import sampler_cases as SC  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")
GAUSS_SD = np.array([1.0, 2.0, 0.5, 3.0, 1.5, 0.25, 4.0])


def gauss_pot(z):
    return 0.5 * float(np.sum(z * z / GAUSS_SD ** 2)), z / GAUSS_SD ** 2


def dc_pot(model, name):
    fx = cases.fixtures(name)
    cf = OC.CFixtures(model, fx)

    def pot(z):
        U, g, _ = OC.potential_and_grad(cf, z, 1)
        return U, g

    return pot, cf


def save(name, pot, key, warm, samp, z0=None, step=1.0, sites=None, max_depth=10, **extra):
    o = NO.run_chain(pot, key, warm, samp, z0=z0, site_shapes=sites, step_size=step, max_depth=max_depth)
    np.savez_compressed(
        os.path.join(OUT, name + ".npz"), key=np.array(key, dtype=np.uint32), num_warmup=warm,
        num_samples=samp, step_size0=step, max_tree_depth=max_depth, z0=o["z0"], z0_given=z0 is not None, draws=o["draws"],
        num_steps=o["num_steps"], accept_prob=o["accept_prob"], diverging=o["diverging"],
        step_size=o["step_size"], potential_energy=o["potential_energy"], depth=o["depth"],
        final_step_size=o["final_step_size"], inverse_mass_matrix=o["inverse_mass_matrix"], **extra)
    print(f"{name}: {o['num_steps'].sum()} leapfrogs, tree sizes {o['num_steps'][:12].tolist()} ...")
    return o


def edge_check(case, pot, o, z0, step, tag=""):
    """The condition a sampler-edge golden must meet before it is saved: the same chain on a potential scaled by
    (1 + 1e-9) with every gradient entry scaled by (1 + 1e-7 u), u seeded uniform in [-1, 1] -- an order of magnitude
    coarser than the float32-table error of the GPU potential -- builds the same trees in all transitions and agrees on
    the first 3 draws and acceptance probabilities to 1e-6 and potential energies to 1e-4: every gate the GPU test
    applies to them (1e-5, 1e-5, 1e-3), ten times inside.  A case that fails gets the next league seed
    (sampler_cases.Case.seed: the first that passes), never a wider gate.  (e128w, e128k32: with seed 0 the
    acceptance probabilities moved by 1.5e-6 and 1.8e-6 -- the start's gradient of several hundred turns draw
    differences of 1e-7 into energy differences of 1e-5.)"""
    u = np.random.RandomState(17).uniform(-1.0, 1.0, case.D)

    def pot2(z):
        U, g = pot(z)
        return U * (1.0 + 1e-9), g * (1.0 + 1e-7 * u)

    p = NO.run_chain(pot2, SC.KEY, 0, SC.TRANSITIONS, z0=z0, step_size=step)
    same = p["num_steps"].tolist() == o["num_steps"].tolist()
    dd = float(np.abs(p["draws"][:3] - o["draws"][:3]).max())
    da = float(np.abs(p["accept_prob"][:3] - o["accept_prob"][:3]).max())
    de = float(np.abs(p["potential_energy"][:3] - o["potential_energy"][:3]).max())
    ok = same and dd < 1e-6 and da < 1e-6 and de < 1e-4
    print(f"  cpu check {case.name}{tag}: league seed {case.seed}, start RandomState(2), step {step}, trees "
          f"{'equal' if same else 'DIFFER ' + str(p['num_steps'].tolist())}, max |d draw[:3]| = {dd:.2e}, "
          f"|d accept[:3]| = {da:.2e}, |d energy[:3]| = {de:.2e} ({'pass' if ok else 'FAIL'})")
    assert ok, case.name


def edge_goldens():
    """tests/golden/nuts_edge_*.npz: adaptation off, 6 transitions at step 0.02 from RandomState(2).uniform(-0.2, 0.2, D)
    under key (0, 11), as nuts_dummy_*_fixed; and for the two weighted loop instantiations the shallow adapted run of
    nuts_dummy_basic_adapt_shallow (22 warm-up, 6 samples, max_depth 2).
    Unweighted leagues with many covariates are too stiff for step 0.02 whatever the seed (the curvature along the
    coefficients grows with K): every transition diverges within three leapfrogs and the chain stays at its start.
    Those goldens are kept -- they pin the divergence decision -- and the same cases (sampler_cases.FINE) get a second
    golden, nuts_edge_<case>_fine.npz, at half the step, where the chain moves through trees of hundreds of leapfrogs;
    it has to meet the same check."""
    for case in SC.ALL:
        cf = OC.CFixtures(case.model, SC.fixtures(case))
        assert cf.D == case.D, case.name

        def pot(z, cf=cf):
            U, g, _ = OC.potential_and_grad(cf, z, 1)
            return U, g

        z0 = SC.start(case)
        o = save("nuts_edge_" + case.name, pot, SC.KEY, 0, SC.TRANSITIONS, z0=z0, step=SC.STEP)
        edge_check(case, pot, o, z0, SC.STEP)
        stuck = bool(np.array_equal(o["draws"][2], z0))        # three transitions that compare nothing but the start
        assert stuck == (case.name in SC.FINE), (case.name, o["accept_prob"].tolist())
        if stuck:
            o = save("nuts_edge_" + case.name + "_fine", pot, SC.KEY, 0, SC.TRANSITIONS, z0=z0, step=SC.FINE_STEP)
            edge_check(case, pot, o, z0, SC.FINE_STEP, "_fine")
            assert (o["accept_prob"][:3] > 1e-2).all() and not o["diverging"].any(), case.name
        if case.name in SC.ADAPTED:
            save("nuts_edge_" + case.name + "_adapt_shallow", pot, (0, 5), 22, 6, z0=z0, step=1.0, max_depth=2)


def main():
    os.makedirs(OUT, exist_ok=True)
    zg = np.array([0.3, -0.2, 0.1, 0.5, -0.4, 0.05, 1.0])
    # Gaussian: fixed step (pure tree builder), then the windowed adaptation
    save("nuts_gauss_fixed", gauss_pot, (0, 11), 0, 12, z0=zg, step=0.4, sd=GAUSS_SD)
    save("nuts_gauss_adapt", gauss_pot, (0, 7), 40, 10, z0=zg, step=1.0, sd=GAUSS_SD)
    # the reference's dummy_data, both in-scope models, fixed small step (deep trees)
    zb = np.random.RandomState(2).uniform(-0.2, 0.2, 45)
    pot, _ = dc_pot(O.MODEL_BASIC, "dummy")
    save("nuts_dummy_basic_fixed", pot, (0, 11), 0, 10, z0=zb, step=0.02)
    save("nuts_dummy_basic_adapt", pot, (0, 5), 30, 10, z0=zb, step=1.0)
    # the same with trees of at most 3 leapfrogs: rounding differences are amplified far less per
    # transition, so a float32-table potential (the GPU's) still tracks the whole warm-up --
    # one slow window (mass matrix update + dual-averaging restart at t = 19) and the final
    # averaging of the step size
    save("nuts_dummy_basic_adapt_shallow", pot, (0, 5), 22, 6, z0=zb, step=1.0, max_depth=2)
    # initial point: init_to_uniform(radius=2) + retry, then a short adapted run
    save("nuts_dummy_basic_init", pot, NO.prng_key(42), 20, 5, z0=None,
         sites=NO.site_shapes(0, 20))
    pot, cf = dc_pot(O.MODEL_EXTENDED, "dummy_cov")
    ze = np.random.RandomState(2).uniform(-0.2, 0.2, cf.D)
    save("nuts_dummy_ext_fixed", pot, (0, 11), 0, 8, z0=ze, step=0.02)
    save("nuts_dummy_ext_init", pot, NO.prng_key(7), 20, 5, z0=None,
         sites=NO.site_shapes(1, 20, 5))
    edge_goldens()


if __name__ == "__main__":
    main()
