"""match_scenarios on the device (csrc/dc_scenario.hip.h) against simulate_season: under one random_state simulation
j here is simulation j there, so the two count tables must equal, integer for integer, the numpy cross-tabulation
(tests/scenarios_ref.py) of simulate_season's per-simulation positions and scorelines.  Every comparison is of
integers, and every derived float is one operation on the same integers on both sides: compared exactly."""
import numpy as np
import pytest

import leverage_ref as L
import scenarios_ref as R
from bpl import DixonColesMatchPredictor, ExtendedDixonColesMatchPredictor
from bpl._ffi import BPLHIP_EINVAL, BPLHIP_ESTATE, HipContext, _np_ptr, prng_key
from bpl.base import LEVERAGE_TARGETS, leverage_targets
from bpl.scenarios import coarsen, marginal

pytestmark = pytest.mark.gpu

EIGHT = {"title": (0,), "top_two": (0, 1), "top_half": range(0, 32), "odd": range(1, 64, 2), "last": (-1,),
         "bottom_three": (-3, -2, -1), "all": range(64), "second": (1,)}
ONE = {"top_half": range(0, 10)}
TABLES = ("scenario_count", "joint_count")
DERIVED = ("scenario_proba", "target_count", "target_proba", "conditional_proba", "conditional_se", "settled", "leverage")


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
    return _model(DixonColesMatchPredictor, att, dfn, rs.normal(0.25, 0.05, S), rs.uniform(-0.1, 0.1, S))


def _table(m, seed=3):
    rs = np.random.RandomState(seed)
    return {t: (int(rs.randint(0, 12)), int(rs.randint(0, 30)), int(rs.randint(0, 30))) for t in m.teams[::2]}


def _half_season(m, seed):
    """A single round robin already played: simulate_season's `played`."""
    T = len(m.teams)
    rs = np.random.RandomState(seed)
    h, a = np.nonzero(np.triu(np.ones((T, T), dtype=bool), 1))
    swap = rs.rand(h.size) < 0.5
    h, a = np.where(swap, a, h), np.where(swap, h, a)
    return {"home_team": list(m.teams[h]), "away_team": list(m.teams[a]),
            "home_goals": [int(v) for v in rs.poisson(1.4, h.size)], "away_goals": [int(v) for v in rs.poisson(1.1, h.size)]}


def _season_tables(m, h, a, keys, caps, N, seed, targets=None, **kw):
    """The yardstick: simulate_season's per-simulation positions and scorelines, cross-tabulated in numpy."""
    season = m.simulate_season(h, a, num_simulations=N, random_state=seed, return_tables=True, return_scores=True, **kw)
    inside = L.target_masks(LEVERAGE_TARGETS if targets is None else targets, len(season["teams"]))
    return season, R.counts(season["position"], season["home_goals"], season["away_goals"], inside, keys, caps)


def _assert_identity(m, h, a, keys, caps, N, seed=1234, targets=None, **kw):
    key_cap = [caps] * len(keys) if isinstance(caps, int) else list(caps)
    season, want = _season_tables(m, h, a, keys, key_cap, N, seed, targets, **kw)
    res = m.match_scenarios(h, a, keys, num_simulations=N, random_state=seed, targets=targets, margin_cap=caps, **kw)
    assert list(res["teams"]) == list(season["teams"])
    assert res["shape"] == R.shape_of(key_cap) and res["fixtures"].tolist() == list(keys)
    np.testing.assert_array_equal(res["margins"], R.margins(key_cap))
    for key, ref in zip(TABLES, want):
        assert res[key].dtype == np.int64 and res[key].shape == ref.shape, (key, res[key].shape, ref.shape)
        np.testing.assert_array_equal(res[key], ref, err_msg=key)
    assert res["scenario_count"].sum() == N
    for key, ref in R.derived(want[0], want[1], N).items():
        assert res[key].shape == ref.shape and res[key].dtype == ref.dtype, key
        np.testing.assert_array_equal(res[key], ref, err_msg=key)         # (NaN == NaN in assert_array_equal)
    return res


# ---------------------------------------------------------------- 1. identity with the season kernel
# (id, posterior, table rows, fixtures, key fixtures, caps, targets, simulations, draws)
IDENTITY = [
    ("one_fixture_two_teams", "basic", 2, 1, [0], 1, {"title": (0,)}, 63, 64),                  # S larger than N
    ("lanes_0_and_63", "extended", 20, 64, [63, 0], (2, 1), None, 3000, 64),
    ("lanes_0_63_64_mixed_caps", "basic", 20, 65, [64, 0, 63], (3, 1, 2), EIGHT, 3000, 64),
    ("last_partial_block_64_teams", "extended", 64, 130, [129, 64, 0, 63, 128], (1, 1, 2, 1, 1), EIGHT, 65, 1),
    ("eight_keys_many_tiles", "basic", 20, 130, [0, 63, 64, 127, 128, 129, 5, 70], 1, EIGHT, 3000, 64),   # M = 6561
    ("one_simulation", "basic", 20, 65, [64], 3, ONE, 1, 64),
    ("one_key_one_target", "extended", 64, 130, [129], 1, ONE, 3000, 16),
]


@pytest.mark.parametrize("tiebreak", ["overall", "head_to_head"])
@pytest.mark.parametrize("case", IDENTITY, ids=[c[0] for c in IDENTITY])
def test_tables_are_the_season_kernels(case, tiebreak):
    _, kind, n, F, keys, caps, targets, N, S = case
    m = _posterior(kind, T=n, S=S, seed=n + F)
    h, a = _pairings(n, F, seed=F) if n > 2 else (np.array([0], dtype=np.uint16), np.array([1], dtype=np.uint16))
    kw = dict(tiebreak="head_to_head", played=_half_season(m, seed=F + 1)) if tiebreak == "head_to_head" else \
        dict(current_table=_table(m), teams=list(m.teams))
    res = _assert_identity(m, h, a, keys, caps, N, seed=F, targets=targets, **kw)
    assert res["joint_count"].shape[1:] == (n, len(LEVERAGE_TARGETS if targets is None else targets))
    if case[0] == "eight_keys_many_tiles":
        assert res["shape"] == (3,) * 8 and res["scenario_count"].size == 6561
        assert (res["scenario_count"] == 0).any() and np.count_nonzero(res["scenario_count"]) > 500
        np.testing.assert_array_equal(res["joint_count"][:, :, 6], np.broadcast_to(res["scenario_count"][:, None], (6561, 20)))


def test_a_team_without_a_fixture():
    m = _posterior("extended", T=20, S=16, seed=5)
    h, a = _pairings(10, 70, seed=5)                                # teams 0..9 play, 10..19 keep their table rows
    res = _assert_identity(m, h, a, [69, 3], (1, 2), 1500, current_table=_table(m), teams=list(m.teams))
    assert len(res["teams"]) == 20 and res["scenario_count"].sum() == 1500


# ---------------------------------------------------------------- 2. identity with match_leverage
def test_one_key_with_cap_one_is_match_leverage():
    m = _posterior("basic", seed=2)
    h, a = _pairings(20, 130, seed=2)
    N, kw = 2000, dict(num_simulations=2000, random_state=9, current_table=_table(m))
    lev = m.match_leverage(h, a, **kw)
    for f in (0, 63, 64, 129):
        res = m.match_scenarios(h, a, [f], **kw)
        np.testing.assert_array_equal(res["scenario_count"], lev["outcome_count"][f])
        np.testing.assert_array_equal(res["joint_count"], lev["joint_count"][f])
        np.testing.assert_array_equal(res["target_count"], lev["target_count"])
        np.testing.assert_array_equal(res["conditional_proba"], lev["conditional_proba"][f])
    for keys, caps in (([5, 64], 1), ([129, 0, 77], (3, 1, 2)), (list(range(60, 68)), 1)):
        res = m.match_scenarios(h, a, keys, margin_cap=caps, **kw)
        np.testing.assert_array_equal(res["target_count"], lev["target_count"])
        assert res["scenario_count"].sum() == N
    played = _half_season(m, seed=3)
    lev = m.match_leverage(h, a, num_simulations=N, random_state=9, tiebreak="head_to_head", played=played)
    res = m.match_scenarios(h, a, [64], num_simulations=N, random_state=9, tiebreak="head_to_head", played=played)
    np.testing.assert_array_equal(res["scenario_count"], lev["outcome_count"][64])
    np.testing.assert_array_equal(res["joint_count"], lev["joint_count"][64])


# ---------------------------------------------------------------- 3. marginalisation
def _assert_same_tables(got, want):
    assert got["shape"] == want["shape"] and got["fixtures"].tolist() == want["fixtures"].tolist()
    for key in TABLES + DERIVED + ("margins", "margin_cap", "home", "away"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)


def test_marginal_of_three_keys_is_the_two_key_call():
    m = _posterior("extended", seed=4)
    h, a = _pairings(20, 100, seed=4)
    kw = dict(num_simulations=2500, random_state=31, current_table=_table(m))
    three = m.match_scenarios(h, a, [70, 2, 64], margin_cap=(2, 1, 3), **kw)
    _assert_same_tables(marginal(three, (0, 2)), m.match_scenarios(h, a, [70, 64], margin_cap=(2, 3), **kw))
    _assert_same_tables(marginal(three, (2, 0)), m.match_scenarios(h, a, [64, 70], margin_cap=(3, 2), **kw))
    _assert_same_tables(marginal(three, (1,)), m.match_scenarios(h, a, [2], margin_cap=1, **kw))
    # the permuted call is the transposed table
    turned = m.match_scenarios(h, a, [64, 70, 2], margin_cap=(3, 2, 1), **kw)
    np.testing.assert_array_equal(turned["scenario_count"].reshape(7, 5, 3),
                                  three["scenario_count"].reshape(5, 3, 7).transpose(2, 0, 1))
    np.testing.assert_array_equal(turned["joint_count"].reshape(7, 5, 3, 20, 3),
                                  three["joint_count"].reshape(5, 3, 7, 20, 3).transpose(2, 0, 1, 3, 4))
    _assert_same_tables(marginal(three, (2, 0, 1)), turned)


# ---------------------------------------------------------------- 4. coarsening
def _favourites(S=32, seed=11):
    """Six teams: 0..2 strong, 3..5 long shots.  A strong side at home to a long shot scores at about 2.0 to 0.8, so
    every clipped margin from home by 3+ (about 0.20) to away by 3+ (about 0.009) has a real chance."""
    rs = np.random.RandomState(seed)
    att = np.array([0.3, 0.3, 0.3, -0.1, -0.1, -0.1]) + rs.normal(0, 0.03, (S, 6))
    dfn = np.array([0.123, 0.123, 0.123, -0.193, -0.193, -0.193]) + rs.normal(0, 0.03, (S, 6))
    return _model(DixonColesMatchPredictor, att, dfn, np.full(S, 0.2), rs.uniform(-0.05, 0.05, S))


def test_coarsened_cap_three_is_the_cap_one_call():
    m = _favourites()
    h = np.array([0, 1, 2, 3, 4, 5, 0, 3], dtype=np.uint16)
    a = np.array([3, 4, 5, 0, 1, 2, 1, 4], dtype=np.uint16)
    keys, N = [0, 1, 2], 3000
    kw = dict(num_simulations=N, random_state=17, targets={"title": (0,), "last": (-1,)})
    # the reference's own cross-tabulation: every margin class of every key fixture occurs, and some scenario never does
    _, (sc, _) = _season_tables(m, h, a, keys, [3, 3, 3], N, 17, targets=kw["targets"])
    cube = sc.reshape(7, 7, 7)
    for q in range(3):
        assert (cube.sum(axis=tuple(r for r in range(3) if r != q)) > 0).all(), q
    assert (sc == 0).any()
    fine = _assert_identity(m, h, a, keys, 3, N, seed=17, targets=kw["targets"])
    assert np.isnan(fine["conditional_proba"]).any() and not np.isnan(fine["conditional_proba"]).all()
    coarse = m.match_scenarios(h, a, keys, margin_cap=1, **kw)
    _assert_same_tables(coarsen(fine, 1), coarse)
    _assert_same_tables(coarsen(fine, (2, 1, 3)), m.match_scenarios(h, a, keys, margin_cap=(2, 1, 3), **kw))
    np.testing.assert_array_equal(coarse["target_count"], fine["target_count"])


# ---------------------------------------------------------------- 5. chunking and repeatability
def test_chunking_changes_nothing():
    m = _posterior("basic", T=14, S=32, seed=8)
    h, a = _pairings(14, 65, seed=8)
    N, seed, keys, caps = 1000, 77, [64, 3, 20], [2, 1, 3]
    hh, aa, table_idx, table, points, n_sims = m._season_inputs(h, a, N, _table(m), None, (3, 1, 0))
    _, masks = leverage_targets(None, table_idx.size)
    _, want = _season_tables(m, h, a, keys, caps, N, seed, current_table=_table(m))
    ctx = m._device()
    whole = ctx.season_scenarios(hh, aa, table_idx, table, points, n_sims, prng_key(seed), masks, keys, caps, chunk_sims=0)
    for key, ref in zip(("scenario", "joint"), want):
        np.testing.assert_array_equal(whole[key].astype(np.int64), ref, err_msg=key)
    for chunk in (1, 64, 100, 4096):
        raw = ctx.season_scenarios(hh, aa, table_idx, table, points, n_sims, prng_key(seed), masks, keys, caps,
                                   chunk_sims=chunk)
        for key in whole:
            np.testing.assert_array_equal(raw[key], whole[key], err_msg=f"{key} at chunk_sims={chunk}")


def test_reproducible_and_the_context_stays_as_it_was():
    m = _posterior("extended", T=10, S=16, seed=6)
    h, a = _pairings(10, 90, seed=6)
    kw = dict(num_simulations=1500, current_table=_table(m, 9))
    before = m.simulate_season(h, a, random_state=21, return_tables=True, **kw)
    r1 = m.match_scenarios(h, a, [0, 89, 64], random_state=21, margin_cap=2, **kw)
    r2 = m.match_scenarios(h, a, [0, 89, 64], random_state=21, margin_cap=2, **kw)
    r3 = m.match_scenarios(h, a, [0, 89, 64], random_state=22, margin_cap=2, **kw)
    for key in r1:
        np.testing.assert_array_equal(r1[key], r2[key], err_msg=key)
    assert not np.array_equal(r1["scenario_count"], r3["scenario_count"])
    after = m.simulate_season(h, a, random_state=21, return_tables=True, **kw)
    for key in before:
        np.testing.assert_array_equal(before[key], after[key], err_msg=key)


# ---------------------------------------------------------------- 6. the raw entry's error codes, in the order of its checks
S_, T_, N_, NF_, SIMS_ = 4, 6, 4, 2, 10       # draws, model teams, table rows, fixtures, simulations
OVER = np.zeros((N_, N_), dtype=np.uint32)
OVER[0, 1] = 0xFFFF << 16                     # slot 0 has 65535 head-to-head points against slot 1, and meets it again


def _raw_call(ctx, **over):
    """bplhip_season_scenarios through the loaded library, all arguments valid (slots 0..3 are model teams 0..3, 0
    plays 1 and 2 plays 3; both fixtures are keys with cap 1) but for `over`: (code, message, scenario, joint)."""
    u16, i32 = (lambda v: np.ascontiguousarray(v, dtype=np.uint16)), (lambda v: np.ascontiguousarray(v, dtype=np.int32))
    keep = dict(h=u16([0, 2]), a=u16([1, 3]), ti=u16([0, 1, 2, 3]), init=[np.zeros(N_, dtype=np.int32) for _ in range(3)],
                masks=np.array([0b0011], dtype=np.uint64), kf=i32(over.pop("keys", [0, 1])),
                kc=i32(over.pop("caps", [1, 1])), scenario=np.zeros(6561, dtype=np.uint64),
                joint=np.zeros(6561 * N_, dtype=np.uint64), pair=over.pop("pair", None))
    args = dict(ctx=ctx._h, n_fixtures=NF_, home_idx=_np_ptr(keep["h"]), away_idx=_np_ptr(keep["a"]), n_table=N_,
                table_idx=_np_ptr(keep["ti"]), init_points=_np_ptr(keep["init"][0]), init_gf=_np_ptr(keep["init"][1]),
                init_ga=_np_ptr(keep["init"][2]), win=3, draw=1, loss=0, n_sims=SIMS_, key_hi=0, key_lo=1, n_targets=1,
                target_mask=_np_ptr(keep["masks"]), chunk_sims=0, n_key=keep["kf"].size, key_fixture=_np_ptr(keep["kf"]),
                key_cap=_np_ptr(keep["kc"]), scenario=_np_ptr(keep["scenario"]), joint=_np_ptr(keep["joint"]),
                stream=None, pair_init=None if keep["pair"] is None else _np_ptr(keep["pair"]))
    assert set(over) <= set(args), set(over) - set(args)
    args.update(over)
    rc = ctx._lib.bplhip_season_scenarios(*args.values())
    return rc, ctx._lib.bplhip_last_error(ctx._h).decode(), keep["scenario"], keep["joint"]


def test_raw_entry_error_codes_in_the_order_of_the_checks():
    bare, ctx = HipContext(0), HipContext(0)
    try:
        # no posterior comes first, whatever else is wrong; so does a venue-form posterior
        assert _raw_call(bare, keys=[0, 2])[:2] == (BPLHIP_ESTATE, "season_scenarios: no posterior set")
        bare.predict_set_posterior_venue(*[np.zeros((S_, T_)) for _ in range(6)], np.zeros(S_))
        assert _raw_call(bare, caps=[0, 1])[0] == BPLHIP_ESTATE
        ctx.predict_set_posterior(np.zeros((S_, T_)), np.zeros((S_, T_)), np.zeros(S_), np.zeros(S_))
        cases = [
            # season_setup and the targets before the keys
            (dict(n_sims=0, keys=[0, 2]), "season_scenarios: n_sims=0 out of range [1,2^31)"),
            (dict(n_targets=0, keys=[0, 2]), "season_scenarios: n_targets=0 out of range [1,8] or null masks"),
            (dict(chunk_sims=-1, keys=[0, 2]), "season_scenarios: chunk_sims=-1 is negative"),
            # the keys: their number and pointers, then the positions, before the caps
            (dict(keys=[], caps=[]), "season_scenarios: n_key=0 out of range [1,8] or null keys"),
            (dict(n_key=9), "season_scenarios: n_key=9 out of range [1,8] or null keys"),
            (dict(key_cap=None, keys=[0, 2]), "season_scenarios: n_key=2 out of range [1,8] or null keys"),
            (dict(keys=[0, 2], caps=[4, 1]), "season_scenarios: key fixture 1 is 2, outside [0,2)"),
            (dict(keys=[-1, 0], caps=[1, 0]), "season_scenarios: key fixture 0 is -1, outside [0,2)"),
            (dict(keys=[1, 1], caps=[1, 0]), "season_scenarios: key fixtures 0 and 1 are both fixture 1"),
            # a bad cap before the number of scenarios, the outputs and the pair records
            (dict(caps=[1, 4], scenario=None), "season_scenarios: the cap of key fixture 1 is 4, outside [1,3]"),
            (dict(caps=[0, 1], pair=OVER), "season_scenarios: the cap of key fixture 0 is 0, outside [1,3]"),
            (dict(caps=[1, 1], joint=None, pair=OVER), "season_scenarios: null required output"),
            # the pair records last
            (dict(pair=OVER), "season_scenarios: the pair record of slots 0 and 1 can pass 16 bits"),
        ]
        for over, message in cases:
            rc, text = _raw_call(ctx, **dict(over))[:2]
            assert (rc, text) == (BPLHIP_EINVAL, message), (over, rc, text)
        # M too large needs more keys than two: five fixtures between the four slots, all keys with cap 3 (7^5 = 16807)
        u16 = lambda v: np.ascontiguousarray(v, dtype=np.uint16)
        five = dict(n_fixtures=5, home_idx=u16([0, 2, 0, 1, 3]), away_idx=u16([1, 3, 2, 3, 0]))
        ptrs = {k: (_np_ptr(v) if isinstance(v, np.ndarray) else v) for k, v in five.items()}
        rc, text = _raw_call(ctx, keys=[0, 1, 2, 3, 4], caps=[3] * 5, pair=OVER, scenario=None, **ptrs)[:2]
        assert (rc, text) == (BPLHIP_EINVAL, "season_scenarios: 16807 scenarios, at most 6561")
        rc, text, _, _ = _raw_call(ctx, keys=[0, 1, 2, 3], caps=[3] * 4, pair=OVER, **ptrs)   # 2401 scenarios: the pairs are next
        assert (rc, text) == (BPLHIP_EINVAL, "season_scenarios: the pair record of slots 0 and 1 can pass 16 bits")
        # and the context stays usable: both orders, every simulation in exactly one scenario
        for pair in (None, np.zeros((N_, N_), dtype=np.uint32)):
            rc, _, scenario, joint = _raw_call(ctx, pair=pair)
            assert rc == 0 and scenario[:9].sum() == SIMS_ and scenario[9:].sum() == 0
            assert joint[:9 * N_].sum() == 2 * SIMS_ and joint[9 * N_:].sum() == 0       # two of the four slots are in the top two
    finally:
        bare.close()
        ctx.close()
