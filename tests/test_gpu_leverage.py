"""match_leverage on the device (csrc/dc_leverage.hip.h) against simulate_season: under one random_state
simulation j here is simulation j there, so the three count tables must equal, integer for integer, the
numpy cross-tabulation (tests/leverage_ref.py) of simulate_season's per-simulation positions and
scorelines.  Every comparison is of integers."""
import numpy as np
import pytest

import leverage_ref as L
from bpl import DixonColesMatchPredictor, ExtendedDixonColesMatchPredictor
from bpl._ffi import BPLHIP_EINVAL, BPLHIP_ESTATE, BplHipError, HipContext, prng_key
from bpl.base import LEVERAGE_TARGETS, leverage_targets

pytestmark = pytest.mark.gpu

EIGHT = {"title": (0,), "top_two": (0, 1), "top_half": range(0, 32), "odd": range(1, 64, 2), "last": (-1,),
         "bottom_three": (-3, -2, -1), "all": range(64), "second": (1,)}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _model(cls, attack, defence, home_advantage, corr_coef):
    m = cls()
    T = attack.shape[1]
    m.teams = np.array([f"t{i:02d}" for i in range(T)])
    m._teams_dict = {t: i for i, t in enumerate(m.teams)}
    m.attack, m.defence = np.asarray(attack, float), np.asarray(defence, float)
    m.home_advantage, m.corr_coef = np.asarray(home_advantage, float), np.asarray(corr_coef, float)
    return m


def _round_robin(T):
    h, a = np.nonzero(~np.eye(T, dtype=bool))
    return h.astype(np.uint16), a.astype(np.uint16)


def _pairings(T, F, seed):
    rs = np.random.RandomState(seed)
    h = rs.randint(0, T, F)
    a = (h + rs.randint(1, T, F)) % T
    return h.astype(np.uint16), a.astype(np.uint16)


def _posterior(kind, T=20, S=64, seed=0):
    rs = np.random.RandomState(seed)
    att, dfn = rs.normal(0, 0.3, (S, T)), rs.normal(0, 0.3, (S, T))
    if kind == "extended":
        return _model(ExtendedDixonColesMatchPredictor, att, dfn, rs.normal(0.25, 0.1, (S, T)), rs.uniform(-0.1, 0.1, S))
    m = _model(DixonColesMatchPredictor, att, dfn, rs.normal(0.25, 0.05, S), rs.uniform(-0.1, 0.1, S))
    if kind == "clipped":   # tau clips for some pairs: rho beyond the bounds in both directions
        m.corr_coef = np.where(np.arange(S) % 2 == 0, 0.9, -1.1)
    return m


def _table(m, seed=3):
    rs = np.random.RandomState(seed)
    return {t: (int(rs.randint(0, 60)), int(rs.randint(0, 70)), int(rs.randint(0, 70))) for t in m.teams[::2]}


def _season_counts(m, h, a, N, seed, targets=None, **kw):
    """The reference: simulate_season's per-simulation outputs, cross-tabulated in numpy."""
    season = m.simulate_season(h, a, num_simulations=N, random_state=seed, return_tables=True, return_scores=True, **kw)
    inside = L.target_masks(LEVERAGE_TARGETS if targets is None else targets, len(season["teams"]))
    return season, L.counts(season["position"], season["home_goals"], season["away_goals"], inside)


def _assert_identity(m, h, a, N, seed=1234, targets=None, **kw):
    season, (outcome, target, joint) = _season_counts(m, h, a, N, seed, targets, **kw)
    res = m.match_leverage(h, a, num_simulations=N, random_state=seed, targets=targets, **kw)
    assert list(res["teams"]) == list(season["teams"])
    for key, want in (("outcome_count", outcome), ("target_count", target), ("joint_count", joint)):
        assert res[key].dtype == np.int64 and res[key].shape == want.shape, key
        np.testing.assert_array_equal(res[key], want, err_msg=key)
    return res


# ---------------------------------------------------------------- 1. identity with the season kernel
@pytest.mark.parametrize("kind", ["basic", "extended", "clipped"])
def test_counts_are_the_season_kernels(kind):
    m = _posterior(kind)
    h, a = _round_robin(20)
    res = _assert_identity(m, h, a, 3000, current_table=_table(m))
    assert res["joint_count"].shape == (380, 3, 20, 3) and list(res["targets"]) == ["title", "top_four", "relegation"]
    assert (res["outcome_count"] > 0).all() and res["leverage"].max() > 0


# ---------------------------------------------------------------- 2. shape edges
@pytest.mark.parametrize("F", [1, 63, 64, 65, 129])
def test_fixture_counts_around_the_block_of_64(F):
    m = _posterior("basic", T=12, S=16, seed=F)
    h, a = _pairings(12, F, seed=F)
    _assert_identity(m, h, a, 300, seed=F, teams=list(m.teams))


@pytest.mark.parametrize("n,F", [(2, 3), (3, 6), (64, 130)])
def test_table_sizes(n, F):
    m = _posterior("extended", T=n, S=8, seed=n)
    h, a = _pairings(n, F, seed=n)
    _assert_identity(m, h, a, 400, seed=n, teams=list(m.teams))


@pytest.mark.parametrize("n", [7, 64])
def test_one_and_eight_overlapping_targets(n):
    m = _posterior("basic", T=n, S=8, seed=n)
    h, a = _pairings(n, 70, seed=n + 1)
    _assert_identity(m, h, a, 300, targets={"top_three": (0, 1, 2)}, teams=list(m.teams))
    res = _assert_identity(m, h, a, 300, targets=EIGHT, teams=list(m.teams))
    assert res["joint_count"].shape == (70, 3, n, 8)
    np.testing.assert_array_equal(res["target_count"][:, 6], 300)     # "all": every team, every simulation


@pytest.mark.parametrize("N,S", [(1, 64), (7, 64), (257, 64), (4097, 64), (257, 1)])
def test_simulation_counts(N, S):
    m = _posterior("basic", T=8, S=S, seed=N)
    h, a = _pairings(8, 40, seed=N)
    _assert_identity(m, h, a, N, seed=N)


def test_other_points_and_a_table_larger_than_the_fixtures():
    m = _posterior("extended", T=20, S=16, seed=5)
    h, a = _pairings(10, 45, seed=5)                                     # teams 0..9 play
    res = _assert_identity(m, h, a, 500, points=(2, 1, 0), current_table=_table(m), teams=list(m.teams))
    assert res["joint_count"].shape == (45, 3, 20, 3)
    _assert_identity(m, h, a, 500, points=(2, 1, 0))


# ---------------------------------------------------------------- 3. chunking
def test_chunking_changes_nothing():
    m = _posterior("basic", T=14, S=32, seed=8)
    h, a = _pairings(14, 65, seed=8)
    N, seed = 4097, 77
    hh, aa, table_idx, table, points, n_sims = m._season_inputs(h, a, N, _table(m), None, (3, 1, 0))
    _, masks = leverage_targets(None, table_idx.size)
    _, want = _season_counts(m, h, a, N, seed, current_table=_table(m))
    ctx = m._device()
    for chunk in (1, 64, 1000, 0):
        raw = ctx.match_leverage(hh, aa, table_idx, table, points, n_sims, prng_key(seed), masks, chunk_sims=chunk)
        for key, ref in zip(("outcome", "target", "joint"), want):
            np.testing.assert_array_equal(raw[key].astype(np.int64), ref, err_msg=f"{key} at chunk_sims={chunk}")


# ---------------------------------------------------------------- 4. closed identities
def test_closed_identities():
    m = _posterior("extended", seed=2)
    h, a = _round_robin(20)
    N, seed, table = 2000, 42, _table(m, 4)
    res = m.match_leverage(h, a, num_simulations=N, random_state=seed, current_table=table)
    np.testing.assert_array_equal(res["outcome_count"].sum(axis=1), N)
    np.testing.assert_array_equal(res["joint_count"].sum(axis=1), np.broadcast_to(res["target_count"], (380, 20, 3)))
    np.testing.assert_array_equal(res["target_count"].sum(axis=0), [N * 1, N * 4, N * 3])
    season = m.simulate_season(h, a, num_simulations=N, random_state=seed, current_table=table)
    counts = np.rint(season["position_proba"] * N).astype(np.int64)
    np.testing.assert_array_equal(counts / N, season["position_proba"])
    inside = L.target_masks(LEVERAGE_TARGETS, 20)
    np.testing.assert_array_equal(res["target_count"], counts @ inside.T.astype(np.int64))
    assert (res["joint_count"] >= 0).all() and (res["joint_count"] <= res["outcome_count"][:, :, None, None]).all()


# ---------------------------------------------------------------- 5. meaning
def test_a_title_already_won_has_no_leverage():
    m = _posterior("basic", T=6, S=16, seed=1)
    h, a = _round_robin(6)
    table = {"t02": (1000, 10, 0)}
    res = m.match_leverage(h, a, num_simulations=1000, random_state=3, current_table=table)
    np.testing.assert_array_equal(res["target_count"][:, 0], [0, 0, 1000, 0, 0, 0])
    np.testing.assert_array_equal(res["leverage"][:, :, 0], 0.0)
    assert res["leverage"][:, :, 2].max() > 0           # relegation is still open


def test_level_teams_with_one_fixture_between_them():
    S = 8
    m = _model(DixonColesMatchPredictor, np.zeros((S, 2)), np.zeros((S, 2)), np.zeros(S), np.zeros(S))
    res = m.match_leverage(["t00"], ["t01"], num_simulations=2000, random_state=11, targets={"title": (0,)})
    assert (res["outcome_count"] > 0).all()
    title = res["conditional_proba"][0, :, :, 0]        # [outcome, team]
    np.testing.assert_array_equal(title[0], [1.0, 0.0])
    np.testing.assert_array_equal(title[2], [0.0, 1.0])
    draws, top = res["outcome_count"][0, 1], res["joint_count"][0, 1, :, 0]
    assert 0 < top[0] < draws and top[0] + top[1] == draws and 0.0 < title[1, 0] < 1.0   # left to the tie-break


def test_an_outcome_that_never_occurs():
    """lambda_home = e^3 ~ 20, lambda_away = e^-4.6 ~ 0.01 at N = 500: no away win (P ~ 1e-9 per simulation).
    At those rates a draw is as rare (it needs 0-0 or a home side held to the away side's goals), so its
    count is 0 too: the conditional is NaN exactly on the outcomes with count 0 of that fixture, and nowhere
    on the balanced fixture next to it."""
    S = 4
    att = np.tile([1.5, -2.3, 0.0, 0.0], (S, 1))
    dfn = np.tile([2.3, -1.5, 0.0, 0.0], (S, 1))
    m = _model(DixonColesMatchPredictor, att, dfn, np.zeros(S), np.zeros(S))
    res = m.match_leverage(["t00", "t02"], ["t01", "t03"], num_simulations=500, random_state=2)
    assert res["outcome_count"][0, 2] == 0 and res["outcome_count"][0, 0] > 0 and (res["outcome_count"][1] > 0).all()
    nan = np.isnan(res["conditional_proba"])
    np.testing.assert_array_equal(nan, np.broadcast_to((res["outcome_count"] == 0)[:, :, None, None], nan.shape))
    assert nan[0, 2].all() and not nan[0, 0].any() and not nan[1].any()
    np.testing.assert_array_equal(np.isnan(res["conditional_se"]), nan)
    assert np.isfinite(res["leverage"]).all()


# ---------------------------------------------------------------- 6. errors
def test_context_state_and_argument_errors():
    ctx = HipContext(0)
    try:
        args = ([0], [1], [0, 1], np.zeros((2, 3)), (3, 1, 0), 10, (0, 1))
        with pytest.raises(BplHipError) as e:
            ctx.match_leverage(*args, [1])
        assert e.value.code == BPLHIP_ESTATE
        S, T = 4, 3
        ctx.predict_set_posterior_venue(*[np.zeros((S, T)) for _ in range(6)], np.zeros(S))
        with pytest.raises(BplHipError) as e:
            ctx.match_leverage(*args, [1])
        assert e.value.code == BPLHIP_ESTATE
        ctx.predict_set_posterior(np.zeros((S, T)), np.zeros((S, T)), np.zeros(S), np.zeros(S))
        for masks in ([], [1] * 9, [1, 0], [0b100]):          # K = 0, K = 9, a zero mask, a position outside the table
            with pytest.raises(BplHipError) as e:
                ctx.match_leverage(*args, masks)
            assert e.value.code == BPLHIP_EINVAL, masks
        h = np.tile([0, 1, 2], 1366)[:4097]
        with pytest.raises(BplHipError) as e:
            ctx.match_leverage(h, (h + 1) % 3, [0, 1, 2], np.zeros((3, 3)), (3, 1, 0), 10, (0, 1), [1])
        assert e.value.code == BPLHIP_EINVAL
        with pytest.raises(BplHipError) as e:
            ctx.match_leverage(*args, [1], chunk_sims=-1)
        assert e.value.code == BPLHIP_EINVAL
        with pytest.raises(BplHipError) as e:                  # simulate_season's own rules: a team playing itself
            ctx.match_leverage([0], [0], [0, 1], np.zeros((2, 3)), (3, 1, 0), 10, (0, 1), [1])
        assert e.value.code == BPLHIP_EINVAL
        out = ctx.match_leverage(h[:4096], (h[:4096] + 1) % 3, [0, 1, 2], np.zeros((3, 3)), (3, 1, 0), 10, (0, 1), [1])
        assert out["outcome"].sum() == 4096 * 10 and out["target"].sum() == 10
    finally:
        ctx.close()


# ---------------------------------------------------------------- 7. reproducibility
def test_reproducible_and_the_context_stays_usable():
    m = _posterior("extended", T=10, S=16, seed=6)
    h, a = _round_robin(10)
    kw = dict(num_simulations=1500, current_table=_table(m, 9))
    before = m.simulate_season(h, a, random_state=21, return_tables=True, return_scores=True, **kw)
    r1 = m.match_leverage(h, a, random_state=21, **kw)
    r2 = m.match_leverage(h, a, random_state=21, **kw)
    r3 = m.match_leverage(h, a, random_state=22, **kw)
    for key in r1:
        np.testing.assert_array_equal(r1[key], r2[key], err_msg=key)
    assert not np.array_equal(r1["joint_count"], r3["joint_count"])
    after = m.simulate_season(h, a, random_state=21, return_tables=True, return_scores=True, **kw)
    for key in before:
        np.testing.assert_array_equal(before[key], after[key], err_msg=key)
