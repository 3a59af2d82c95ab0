"""float64 numpy restatement of team_ratings (bpl/ratings.py, csrc/dc_ratings.hip.h), operation for operation
where the definition fixes an order: the log rates in the product forms of tests/fake_ctx.py::_log_rates (the
forms of tests/loglik_ref.py), the matches of a rated team in the kernel's order (opponents as given; under
"both" the home match of a pairing before its away match), the running sums taken match by match, left to
right.  The outcome probabilities come by the route of tests/scores_ref.py, NOT the kernel's walk: the full
scoreline grid of every (draw, match) from closed-form pmfs and its three triangles.  Summaries with numpy's
own mean / std / quantile; the rank rule as a double loop over the teams."""
import numpy as np

import scores_ref as SR
from fake_ctx import FakePredictCtx

STATISTICS = ("points", "win", "goals_for", "goals_against", "goal_difference")
VENUES = ("both", "home", "away", "neutral")


def fixtures_of(teams, opponents, venue, team_conf=None, opp_conf=None):
    """The matches in the kernel's order: (home, away, neutral, home conf, away conf, rated team listed first,
    position of the rated team) per match, as columns, and the matches per rated team."""
    rows, n = [], []
    for i, t in enumerate(teams):
        n.append(0)
        for j, o in enumerate(opponents):
            if o == t:
                continue
            tc = None if team_conf is None else team_conf[i]
            oc = None if opp_conf is None else opp_conf[j]
            if venue in ("both", "home", "neutral"):
                rows.append((t, o, int(venue == "neutral"), tc, oc, True, i))
                n[-1] += 1
            if venue in ("both", "away"):
                rows.append((o, t, 0, oc, tc, False, i))
                n[-1] += 1
    return rows, np.array(n, dtype=np.int64)


def values_from(log_rates, rho, teams, opponents, venue, G, points, team_conf=None, opp_conf=None):
    """(v [S, 5, R], matches [R], the largest rate): `log_rates(h, a, neutral, conf)` as FakePredictCtx._log_rates."""
    rows, n = fixtures_of(list(teams), list(opponents), venue, team_conf, opp_conf)
    h = np.array([r[0] for r in rows], dtype=int)
    a = np.array([r[1] for r in rows], dtype=int)
    plain = venue != "neutral" and getattr(log_rates, "plain", False)
    neutral = None if plain else np.array([r[2] for r in rows])
    conf = None if team_conf is None else (np.array([r[3] for r in rows], dtype=int),
                                           np.array([r[4] for r in rows], dtype=int))
    eh, ea = log_rates(h, a, neutral, conf)
    lh, la = np.exp(eh), np.exp(ea)
    rho = np.asarray(rho, dtype=np.float64)
    p = SR.draw_probs(lh, la, rho, G)   # [S, n, 3]: home win, draw, away win
    S, W, D, L = rho.size, float(points[0]), float(points[1]), float(points[2])
    sums = np.zeros((4, S, len(teams)))   # points, win, goals_for, goals_against
    for m, (_, _, _, _, _, first, i) in enumerate(rows):
        p_win, p_draw, p_loss = (p[:, m, 0], p[:, m, 1], p[:, m, 2]) if first else (p[:, m, 2], p[:, m, 1], p[:, m, 0])
        sums[0, :, i] = sums[0, :, i] + (W * p_win + D * p_draw + L * p_loss)
        sums[1, :, i] = sums[1, :, i] + p_win
        sums[2, :, i] = sums[2, :, i] + (lh[:, m] if first else la[:, m])
        sums[3, :, i] = sums[3, :, i] + (la[:, m] if first else lh[:, m])
    nd = n.astype(np.float64)
    v = np.empty((S, 5, len(teams)))
    for k in range(4):
        v[:, k, :] = sums[k] / nd
    v[:, 4, :] = (sums[2] - sums[3]) / nd
    return v + 0.0, n, float(max(lh.max(), la.max()))


def ranks(x):
    """(rank_count, better_count) int64 [R, R] of values x [S, R]: the rank rule as a double loop over the teams."""
    S, R = x.shape
    rank = np.zeros((S, R), dtype=np.int64)
    better = np.zeros((R, R), dtype=np.int64)
    for t in range(R):
        for u in range(R):
            if u == t:
                continue
            ahead = (x[:, u] > x[:, t]) | ((x[:, u] == x[:, t]) & (u < t))
            rank[:, t] += ahead
            better[t, u] = int((x[:, t] > x[:, u]).sum())
    count = np.zeros((R, R), dtype=np.int64)
    for t in range(R):
        for r in range(R):
            count[t, r] = int((rank[:, t] == r).sum())
    return count, better


def summarise(v, quantiles):
    S = v.shape[0]
    q = np.asarray(quantiles, dtype=np.float64).reshape(-1)
    quant = np.quantile(v, q, axis=0).transpose(1, 0, 2) if q.size else np.empty((v.shape[1], 0, v.shape[2]))
    return {"mean": v.mean(axis=0), "sd": v.std(axis=0, ddof=1) if S > 1 else np.zeros(v.shape[1:]), "quantile": quant}


def device_part(log_rates, rho, teams, opponents, venue, G, points, rank_by, quantiles, team_conf=None,
                opp_conf=None, return_draws=False):
    """What HipContext.team_ratings returns; `venue` and `rank_by` by name."""
    v, n, top = values_from(log_rates, rho, teams, opponents, venue, G, points, team_conf, opp_conf)
    out = summarise(v, quantiles)
    count, better = ranks(v[:, STATISTICS.index(rank_by), :])
    out.update(rank_count=count.astype(np.int32), better_count=better.astype(np.int32), matches=n.astype(np.int32),
               top_rate=top)
    if return_draws:
        out["draws"] = v
    return out


def model_log_rates(m, week=None):
    """`log_rates(h, a, neutral, conf)` of a hand-built model (loglik_ref.hand_model), on one gameweek's tables for
    the dynamic class: the model's own upload into the numpy stand-in context."""
    ctx = FakePredictCtx()
    if week is not None:
        m._predict_gameweek = week
    m._upload_posterior(ctx)
    fn = lambda h, a, neutral, conf: ctx._log_rates(h, a, neutral, conf)
    fn.plain = ctx.venue is None
    return fn


def team_ratings(m, teams=None, opponents=None, venue=None, G=15, points=(3, 1, 0), rank_by="points",
                 quantiles=(0.05, 0.5, 0.95), team_conf=None, week=None):
    """The restatement of `team_ratings` for one gameweek (no leading axis): the raw device part with "draws"."""
    names = [str(t) for t in m.teams]
    teams = names if teams is None else list(teams)
    opponents = teams if opponents is None else list(opponents)
    lr = model_log_rates(m, week)
    if venue is None:
        venue = "both" if lr.plain else "neutral"
    tc = oc = None
    if team_conf is not None:
        tc = [m._conferences_dict[team_conf[t]] for t in teams]
        oc = [m._conferences_dict[team_conf[t]] for t in opponents]
    return device_part(lr, np.asarray(m.corr_coef, dtype=np.float64), [names.index(t) for t in teams],
                       [names.index(t) for t in opponents], venue, G, points, rank_by, quantiles, tc, oc, True)


# ---- the cases of the class tests, shared by the host and the GPU tests
def conf_of(m):
    """team -> confederation name for the World-Cup hand model: team i in confederation i mod C."""
    return {str(t): str(m.conferences[i % len(m.conferences)]) for i, t in enumerate(m.teams)}


def class_cases(kind, G):
    """(venue, points) per case: every venue mode the class takes at depth G, and non-default points once."""
    venues = ("both", "home", "away") + (("neutral",) if kind in ("neutral", "wc", "dynamic") else ())
    cases = [(v, (3, 1, 0)) for v in venues]
    if G == 15:
        cases.append((venues[-1], (2, 1, 0)))
    return cases


def points_gate(points):
    return 2e-12 * max(1.0, float(sum(abs(p) for p in points)))
