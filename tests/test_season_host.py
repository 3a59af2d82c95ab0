"""simulate_season without a GPU: the numpy restatement's threefry against the library's, the exact
sampler's inverse-CDF intervals against max(tau, 0) Pois Pois / Z, and every argument check (all
made on the host before the device is touched)."""
import numpy as np
import pytest
from scipy.stats import poisson

import season_ref as R
from bpl import DixonColesMatchPredictor, ExtendedDixonColesMatchPredictor, _ffi


@pytest.mark.parametrize("key", [(0, 0), (0, 42), (0xDEADBEEF, 0x12345678), (0xFFFFFFFF, 0xFFFFFFFF)])
def test_numpy_block_matches_library_threefry(key):
    # bplhip_threefry_bits(key, 2m): word i is o0 of block (i, m + i), word m + i its o1
    for m in (1, 37, 1000):
        bits = _ffi.threefry_bits(key, 2 * m)
        o0, o1 = R.threefry_block(key, np.arange(m), m + np.arange(m))
        np.testing.assert_array_equal(bits[:m], o0)
        np.testing.assert_array_equal(bits[m:], o1)


def _rho_bounds(lh, la):
    # tau >= 0 on all four low scorelines
    return max(-1.0 / lh, -1.0 / la), min(1.0 / (lh * la), 1.0)


def _cases():
    out = [(1.4, 1.1, -0.05), (0.3, 2.5, 0.1), (3.2, 0.4, 0.0), (0.05, 0.08, 0.3)]
    for lh, la in ((1.4, 1.1), (2.7, 0.6)):
        lo, hi = _rho_bounds(lh, la)
        out += [(lh, la, lo + 1e-6), (lh, la, hi - 1e-6)]
    out.append((1.5, 1.2, 0.9))      # 1 - lh la rho < 0: t00 clips
    out.append((0.9, 1.3, -1.5))     # 1 + lh rho and 1 + la rho clip
    return out


@pytest.mark.parametrize("lh,la,rho", _cases())
def test_sampler_intervals_are_the_clipped_dixon_coles_pmf(lh, la, rho):
    G, depth = 14, 80
    x, y = np.meshgrid(np.arange(depth), np.arange(depth), indexing="ij")
    tau = np.ones((depth, depth))
    tau[0, 0], tau[0, 1], tau[1, 0], tau[1, 1] = 1 - lh * la * rho, 1 + lh * rho, 1 + la * rho, 1 - rho
    w = np.maximum(tau, 0.0) * poisson.pmf(x, lh) * poisson.pmf(y, la)
    target = (w / w.sum())[: G + 1, : G + 1]
    home, away = R.scoreline_edges(lh, la, rho, G)
    lengths = np.diff(home)[:, None] * np.diff(away, axis=1)
    np.testing.assert_allclose(lengths, target, rtol=0, atol=1e-12)
    # the vectorised sampler draws (x, y) at the middle of each interval of non-negligible length
    xs, ys = np.nonzero((np.diff(home)[:, None] > 1e-9) & (np.diff(away, axis=1) > 1e-9))
    u1 = (home[xs] + home[xs + 1]) / 2
    u2 = (away[xs, ys] + away[xs, ys + 1]) / 2
    gx, gy, _ = R.sample_scorelines(np.full(xs.size, lh), np.full(xs.size, la), np.full(xs.size, rho), u1, u2)
    np.testing.assert_array_equal(gx, xs)
    np.testing.assert_array_equal(gy, ys)


def _hand_posterior(cls=DixonColesMatchPredictor, T=6, S=8):
    rs = np.random.RandomState(1)
    m = cls()
    m.teams = np.array([f"t{i:02d}" for i in range(T)])
    m._teams_dict = {t: i for i, t in enumerate(m.teams)}
    m.attack = rs.normal(0, 0.2, (S, T))
    m.defence = rs.normal(0, 0.2, (S, T))
    m.home_advantage = rs.normal(0.2, 0.05, S if cls is DixonColesMatchPredictor else (S, T))
    m.corr_coef = rs.uniform(-0.05, 0.05, S)
    return m


def _raises(m, exc, *args, **kwargs):
    with pytest.raises(exc):
        m.simulate_season(*args, **kwargs)
    assert m._predict_ctx is None   # no device context was ever made


@pytest.mark.parametrize("cls", [DixonColesMatchPredictor, ExtendedDixonColesMatchPredictor])
def test_argument_checks_run_on_the_host(cls):
    m = _hand_posterior(cls)
    H, A = ["t00", "t01"], ["t01", "t02"]
    _raises(m, KeyError, ["t00", "nope"], ["t01", "t02"], num_simulations=10)
    _raises(m, KeyError, H, A, num_simulations=10, current_table={"nope": (1, 1, 1)})
    _raises(m, KeyError, H, A, num_simulations=10, teams=["t00", "nope"])
    _raises(m, ValueError, [], [], num_simulations=10)                                   # n == 0
    _raises(m, ValueError, [], [], num_simulations=10, teams=[])
    _raises(m, ValueError, H, A, num_simulations=10, teams=["t00", "t01"])               # t02 not in the table
    _raises(m, ValueError, ["t00", "t01"], ["t00", "t02"], num_simulations=10)          # t00 plays itself
    _raises(m, ValueError, H, A, num_simulations=0)
    _raises(m, ValueError, H, A, num_simulations=2 ** 31)
    _raises(m, ValueError, H, A, num_simulations=10.0)
    _raises(m, ValueError, H, A, num_simulations=10, current_table={"t00": (-1, 0, 0)})
    _raises(m, ValueError, H, A, num_simulations=10, current_table={"t00": (3, -2, 0)})
    _raises(m, ValueError, H, A, num_simulations=10, current_table={"t00": (3, 0)})
    _raises(m, ValueError, H, A, num_simulations=10, current_table={"t05": (3, 0, 0)}, teams=["t00", "t01", "t02"])
    for pts in [(3, 1), (3, -1, 0), (3.5, 1, 0), (3, 1, 0, 0), ("3", 1, 0)]:
        _raises(m, ValueError, H, A, num_simulations=10, points=pts)
    _raises(m, ValueError, [0, 1], [1, 9], num_simulations=10)                            # index beyond the model


def test_more_than_64_teams_is_refused_on_the_host():
    m = _hand_posterior(T=70)
    _raises(m, ValueError, ["t00"], ["t01"], num_simulations=10, teams=list(m.teams))
    h = [f"t{i:02d}" for i in range(0, 66, 2)]
    a = [f"t{i:02d}" for i in range(1, 66, 2)]
    _raises(m, ValueError, h, a, num_simulations=10)


def test_table_inputs_resolve_in_model_order():
    m = _hand_posterior()
    h, a, table_idx, table, points, n = m._season_inputs(
        ["t03", "t01"], ["t01", "t04"], 5, {"t05": (10, 4, 2)}, None, (2, 1, 0))
    assert list(table_idx) == [1, 3, 4, 5]
    assert table.tolist() == [[0, 0, 0], [0, 0, 0], [0, 0, 0], [10, 4, 2]]
    assert points == (2, 1, 0) and n == 5
    _, _, table_idx, _, _, _ = m._season_inputs(["t03"], ["t01"], 5, None, ["t05", "t01", "t03", "t01"], (3, 1, 0))
    assert list(table_idx) == [1, 3, 5]
