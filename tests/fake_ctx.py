"""TEST-ONLY stand-in for bpl._ffi.HipContext: same surface, but the potential is the
CPU oracle (through the NUTS harness).  Lets the host orchestration (bpl/_mcmc.py,
bpl/_dist.py: chain ownership, key splitting, broadcast, gather, constrain) run under
gloo on a box without a GPU.  Never imported by product code."""
import numpy as np
import torch

import dc_oracle as O
import dc_oracle_c as OC


class RecordingCtx:
    """TEST-ONLY recording stand-in for bpl._ffi.HipContext's fit surface, for the fit drivers of all
    five model classes (bpl/_mcmc.py:sample_chains).  Nothing is sampled: the draws of a chain are a
    fixed function of its key and start point (`stub_draws`), the constrain steps fixed slices of the
    draws.  Every call is appended to the class-level `log` as (name, payload); `fail` names a call
    that raises instead (an exception instance).  `lockstep_code`: None (lock step works) or the
    BplHipError code `nuts_run_chains` raises."""
    log = []
    fail = {}
    lockstep_code = None

    @classmethod
    def reset(cls, fail=None, lockstep_code=None):
        cls.log, cls.fail, cls.lockstep_code = [], dict(fail or {}), lockstep_code

    def __init__(self, device_index=0):
        self.device, self.dim = torch.device("cpu"), 0
        self._note("create", device_index)

    def _note(self, name, payload=None):
        self.log.append((name, payload))
        if name in self.fail:
            raise self.fail[name]

    @staticmethod
    def _arr(a):
        if a is None:
            return None
        return np.array(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)

    def set_fixtures(self, model, h, a, x, y, n_teams, weights=None, covariates_std=None):
        k = 0 if covariates_std is None else np.asarray(covariates_std).shape[1]
        self.model, self.n_teams = model, n_teams
        self.dim = 2 * n_teams + 5 if model == O.MODEL_BASIC else 3 * n_teams + 2 * k + 7
        self._note("set_fixtures", (model, n_teams, [self._arr(v) for v in (h, a, x, y, weights, covariates_std)]))
        return self

    def set_fixtures_neutral(self, h, a, x, y, nv, n_teams, weights=None, covariates_std=None, home_conf=None,
                             away_conf=None, n_conf=0):
        k = 0 if covariates_std is None else np.asarray(covariates_std).shape[1]
        self.n_teams, self.dim = n_teams, 6 * n_teams + 2 * k + n_conf + 13
        self._note("set_fixtures_neutral", (n_teams, n_conf, [self._arr(v) for v in (
            h, a, x, y, nv, weights, covariates_std, home_conf, away_conf)]))
        return self

    def set_fixtures_dynamic(self, h, a, x, y, gw, nv, n_teams, n_gameweeks, covariates_std=None, random_walk=True):
        k = 0 if covariates_std is None else np.asarray(covariates_std).shape[1]
        self.n_teams, self.n_gameweeks = n_teams, n_gameweeks
        self.dim = 7 * n_gameweeks * n_teams + 10 * n_gameweeks + 2 + 2 * k
        self._note("set_fixtures_dynamic", (n_teams, n_gameweeks, bool(random_walk),
                                            [self._arr(v) for v in (h, a, x, y, gw, nv, covariates_std)]))
        return self

    @staticmethod
    def _cfg(cfg):
        return tuple((f, getattr(cfg, f)) for f, _ in cfg._fields_)

    @staticmethod
    def stub_draws(cfg, key, z0, dim):
        """([kept, dim] draws, the stats dict of HipContext.nuts_run) of the chain with this key and start."""
        kept = cfg.num_samples // cfg.thinning
        rs = np.random.RandomState([int(key[0]), int(key[1])])
        d = 0.1 * rs.standard_normal((kept, dim)) + (0.0 if z0 is None else np.asarray(z0, np.float64))
        st = {"potential_energy": rs.standard_normal(kept), "accept_prob": rs.uniform(0.6, 1.0, kept),
              "step_size": np.full(kept, 0.25), "num_steps": rs.randint(1, 64, kept).astype(np.int32),
              "diverging": (rs.uniform(size=kept) < 0.1).astype(np.int32), "corr_coef": rs.uniform(-0.05, 0.03, kept),
              "inverse_mass_matrix": np.ones(dim), "final_step_size": 0.25 + 1e-3 * (int(key[1]) % 7),
              "mean_accept_prob": 0.8, "total_leapfrogs": 100 + int(key[1]) % 11, "total_divergences": int(key[1]) % 3,
              "wall_seconds": 1.0 + (int(key[1]) % 5)}
        return d, st

    def nuts_run(self, cfg, key, z0=None):
        if z0 is not None and np.shape(z0) != (self.dim,):  # (HipContext's own check, before any device call)
            raise ValueError(f"init_params must have shape ({self.dim},)")
        self._note("nuts_run", (self._cfg(cfg), tuple(key), self._arr(z0)))
        return self.stub_draws(cfg, key, z0, self.dim)

    def nuts_run_chains(self, cfg, keys, z0=None):
        n = len(keys)
        if z0 is not None and np.shape(z0) == (self.dim,):  # (HipContext tiles one point over the chains)
            z0 = np.tile(np.asarray(z0, np.float64), (n, 1))
        if z0 is not None and np.shape(z0) != (n, self.dim):
            raise ValueError(f"init_params must have shape ({n}, {self.dim})")
        self._note("nuts_run_chains", (self._cfg(cfg), [tuple(k) for k in keys], self._arr(z0)))
        if self.lockstep_code is not None:
            from bpl._ffi import BplHipError

            raise BplHipError(self.lockstep_code, "stub")
        return [self.stub_draws(cfg, k, None if z0 is None else z0[i], self.dim) for i, k in enumerate(keys)]

    def constrain(self, z):
        self._note("constrain", self._arr(z))
        t = self.n_teams
        ha = z[:, 2 * t].copy() if self.model == O.MODEL_BASIC else z[:, 2 * t:3 * t].copy()
        return {"attack": z[:, :t].copy(), "defence": z[:, t:2 * t].copy(), "home_advantage": ha,
                "corr_coef": 0.05 * np.tanh(z[:, -1])}

    def constrain_dynamic(self, z):
        self._note("constrain_dynamic", self._arr(z))
        g, t = self.n_gameweeks, self.n_teams
        names = ("attack", "defence", "home_attack", "away_attack", "home_defence", "away_defence")
        return {nm: z[:, i * g * t:(i + 1) * g * t].reshape(z.shape[0], g, t).copy() for i, nm in enumerate(names)}

    def close(self):
        self.log.append(("close", None))


class FakeCtx:
    def __init__(self, device_index=0):
        self.device = torch.device("cpu")
        self.dim = 0

    def set_fixtures(self, model, h, a, x, y, n_teams, weights=None, covariates_std=None):
        def np_(t, dt):
            t = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
            return t.view(np.uint16) if (dt == np.uint16 and t.dtype == np.int16) else t.astype(dt)

        fx = O.Fixtures(np_(h, np.uint16), np_(a, np.uint16), np_(x, np.uint8), np_(y, np.uint8),
                        n_teams, weights=None if weights is None else np_(weights, np.float64))
        self.fx, self.model, self.n_teams = fx, model, n_teams
        self.cf = OC.CFixtures(model, fx)
        if covariates_std is not None:  # already standardised by the caller
            self.cf.K = covariates_std.shape[1]
            self.cf.xs = np.ascontiguousarray(covariates_std, dtype=np.float64)
            self.cf.D = O.latent_dim(model, n_teams, self.cf.K)
        self.dim = self.cf.D
        return self

    def nuts_run(self, cfg, key, z0=None):
        rc, draws, stats, summ = OC.nuts_dc(self.cf, cfg.num_warmup, cfg.num_samples, key,
                                            thin=cfg.thinning, z0=z0)
        assert rc == 0
        kept = draws.shape[0]
        out = {"potential_energy": stats[:, 0], "accept_prob": stats[:, 1],
               "step_size": np.full(kept, summ[0]), "num_steps": stats[:, 2].astype(np.int32),
               "diverging": stats[:, 3].astype(np.int32), "corr_coef": np.zeros(kept),
               "inverse_mass_matrix": summ[4:], "final_step_size": summ[0],
               "mean_accept_prob": summ[1], "total_leapfrogs": int(summ[2]),
               "total_divergences": int(summ[3]), "wall_seconds": 1.0}
        return draws, out

    def constrain(self, z):
        T, sl = self.n_teams, O.site_slices(self.model, self.n_teams, self.cf.K)
        s = z.shape[0]
        att, dfn, corr = np.empty((s, T)), np.empty((s, T)), np.empty(s)
        ha = np.empty(s) if self.model == O.MODEL_BASIC else np.empty((s, T))
        fx = self.fx
        if self.cf.K:  # un-standardised copy is not kept: rebuild a Fixtures with xs as raw
            fx = O.Fixtures(fx.home_idx, fx.away_idx, fx.home_goals, fx.away_goals, T,
                            weights=fx.weights, covariates=self.cf.xs)
        for i in range(s):
            _, _, aux = O.potential_and_grad(self.model, fx, z[i])
            att[i], dfn[i], ha[i], corr[i] = aux["attack"], aux["defence"], aux["home_advantage"], aux["corr_coef"]
        return {"attack": att, "defence": dfn, "home_advantage": ha, "corr_coef": corr}

    def close(self):
        pass


class FakePredictCtx:
    """TEST-ONLY numpy (float64) predict backend with bpl._ffi.HipContext's predict surface:
    a restatement of the reference's predict_score_proba -- bpl/dixon_coles.py:126-163 for the
    league models, bpl/neutral_dixon_coles.py:399-488 / bpl/neutral_dixon_coles_WC.py:363-470 for the
    venue-aware family -- with the tau term of bpl/_util.py:35-93.  The CPU API tests inject it as
    `model._predict_ctx`; the GPU tests use it as the float64 comparator of the device kernels."""

    def predict_set_posterior(self, attack, defence, home_advantage, corr_coef):
        self.att, self.dfn = np.asarray(attack, float), np.asarray(defence, float)
        self.ha, self.cc = np.asarray(home_advantage, float), np.asarray(corr_coef, float)
        self.venue = None

    def predict_set_posterior_venue(self, attack, defence, home_attack, away_attack, home_defence,
                                    away_defence, corr_coef, confederation_strength=None):
        self.att, self.dfn = np.asarray(attack, float), np.asarray(defence, float)
        self.venue = [np.asarray(t, float) for t in (home_attack, away_attack, home_defence, away_defence)]
        self.conf = None if confederation_strength is None else np.asarray(confederation_strength, float)
        self.cc = np.asarray(corr_coef, float)

    def _log_rates(self, h, a, neutral, conf):
        eh = self.att[:, h] - self.dfn[:, a]
        ea = self.att[:, a] - self.dfn[:, h]
        if self.venue is None:
            assert neutral is None and conf is None
            return eh + (self.ha[:, None] if self.ha.ndim == 1 else self.ha[:, h]), ea
        assert neutral is not None and (conf is None) == (self.conf is None)
        hat, aat, hdf, adf = self.venue
        on = 1.0 - np.broadcast_to(np.asarray(neutral, float), h.shape)
        eh = eh + on * hat[:, h] - on * adf[:, a]
        ea = ea + on * aat[:, a] - on * hdf[:, h]
        if conf is not None:
            hc = np.broadcast_to(np.asarray(conf[0], int), h.shape)
            ac = np.broadcast_to(np.asarray(conf[1], int), h.shape)
            d = self.conf[:, hc] - self.conf[:, ac]
            eh, ea = eh + d, ea - d
        return eh, ea

    def predict_score_proba(self, h, a, x, y, neutral=None, conf=None):
        from scipy.special import gammaln

        h, a = np.asarray(h, int), np.asarray(a, int)
        x, y = np.asarray(x, int), np.asarray(y, int)
        eh, ea = self._log_rates(h, a, neutral, conf)
        lh, la = np.exp(eh), np.exp(ea)
        rho = self.cc[:, None]
        tau = np.ones_like(lh)
        tau = np.where((x == 0) & (y == 0), np.clip(1 - rho * lh * la, 0, None), tau)
        tau = np.where((x == 1) & (y == 0), np.clip(1 + rho * la, 0, None), tau)
        tau = np.where((x == 0) & (y == 1), np.clip(1 + rho * lh, 0, None), tau)
        tau = np.where((x == 1) & (y == 1), np.clip(1 - rho + 0 * lh, 0, None), tau)
        ph = np.exp(eh * x - gammaln(x + 1.0) - lh)
        pa = np.exp(ea * y - gammaln(y + 1.0) - la)
        return (tau * ph * pa).mean(axis=0)

    def predict_score_grid(self, h, a, max_goals, neutral=None, conf=None):
        h, a = np.asarray(h, int), np.asarray(a, int)
        g1 = max_goals + 1
        xs, ys = np.meshgrid(np.arange(g1), np.arange(g1), indexing="ij")
        out = np.empty((len(h), g1, g1))
        nv = None if neutral is None else np.broadcast_to(np.asarray(neutral), h.shape)
        for i in range(len(h)):
            ci = None if conf is None else (np.broadcast_to(np.asarray(conf[0]), h.shape)[i],
                                            np.broadcast_to(np.asarray(conf[1]), h.shape)[i])
            out[i] = self.predict_score_proba(np.full(g1 * g1, h[i]), np.full(g1 * g1, a[i]),
                                              xs.ravel(), ys.ravel(),
                                              None if nv is None else nv[i], ci).reshape(g1, g1)
        return out
