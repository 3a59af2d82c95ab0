"""TEST-ONLY numpy float32 emulation of the walk of `predict_score_grid` (csrc/dc_predict.hip.h), and the
input sets of tests/test_gpu_predict.py.

The emulation restates what the kernel does to its numbers, operation by operation in float32, vectorised
over fixtures and cells: the float32 posterior copies, the log-rates in the kernel's association, the rates
and pmf(0) through exp2 of a float32 product with log2(e), the first tile's e^-r r^k without the factorials
(1 / (x! y!) on the finished float64 cell), the recurrence p(k + 1) = p(k) * (r * 1 / (k + 1)) of the later
tiles (a restarted tile repeats the same products, so one chain gives every tile's vector), the MFMA's
float32 fma chain over the draws of a block (draw 16 k + g in instruction g, k = 0..3) folded into float64
every 256 draws, and the four tau cells as per-lane float32 fma chains of p * max(1 + rho c, 0) summed over
the wave in float64.  What it does not restate: the error of v_exp_f32 itself (exp2 is taken correctly
rounded) and which of the tau expressions the compiler contracts (taken as fused).

tests/test_predict_emu_host.py holds it against tests/fake_ctx.py:FakePredictCtx on these input sets: the
float32 METHOD sits inside half of the grid gate, so a device result outside the gate is the kernel's."""
import numpy as np

import loglik_ref as LR

F32, F64 = np.float32, np.float64
LOG2E = F32(1.44269504088896341)
VENUE_TABLES = ("attack", "defence", "home_attack", "away_attack", "home_defence", "away_defence")


# ---- the input sets
def posterior(kind, S, T, seed=0, week=1, C=3):
    """(venue, args): the hand-built posterior of loglik_ref.hand_model as the arguments of
    predict_set_posterior (venue False) or predict_set_posterior_venue (True); the dynamic class gives the
    tables of gameweek `week`."""
    m = LR.hand_model(kind, S=S, T=T, seed=seed, C=C)
    if kind in ("basic", "extended"):
        return False, [m.attack, m.defence, m.home_advantage, m.corr_coef]
    tabs = [getattr(m, nm) for nm in VENUE_TABLES]
    if kind == "dynamic":
        tabs = [np.ascontiguousarray(t[:, week, :]) for t in tabs]
    return True, tabs + [m.corr_coef, m.confederation_strength if kind == "wc" else None]


def set_posterior(ctx, venue, args):
    (ctx.predict_set_posterior_venue if venue else ctx.predict_set_posterior)(*args)


def with_corr(venue, args, corr_coef):
    out = list(args)
    out[6 if venue else 3] = np.asarray(corr_coef, dtype=F64)
    return venue, out


def fixtures(kind, M, T, seed=0, C=3):
    """(h, a, kw) of M fixtures: the last one's home team and the first one's away team are T - 1; for the
    venue-aware kinds `neutral` alternates 0, 1; with confederations the first row has equal ones and the
    second different ones."""
    rs = np.random.RandomState(1000 + seed)
    h = rs.randint(0, T, M)
    a = (h + 1 + rs.randint(0, T - 1, M)) % T
    h[-1], a[-1] = T - 1, 0
    if M > 1:
        h[0], a[0] = T - 2, T - 1
    kw = {}
    if kind not in ("basic", "extended"):
        kw["neutral"] = (np.arange(M) % 2).astype(np.uint8)
    if kind == "wc":
        hc, ac = rs.randint(0, C, M), rs.randint(0, C, M)
        ac[0] = hc[0]
        if M > 1:
            ac[1] = (hc[1] + 1) % C
        kw["conf"] = (hc, ac)
    return h, a, kw


CLIP_PATTERNS = ("all", "third", "all_but_one_in_50", "mixed_sign")


def clipped_corr(pattern, corr_coef):
    """corr_coef with 5.0 (every tau of a positive c clipped at rates about 1) in one of four patterns."""
    s = np.arange(corr_coef.size)
    if pattern == "all":
        return np.full(corr_coef.size, 5.0)
    if pattern == "third":
        return np.where(s % 3 == 0, 5.0, corr_coef)
    if pattern == "all_but_one_in_50":
        return np.where(s % 50 == 7, corr_coef, 5.0)
    if pattern == "mixed_sign":
        return np.where(s % 2 == 0, -5.0, 5.0)
    raise ValueError(pattern)


# The gate is tight for float32: a tail cell (x about 14) above the 1e-12 floor is carried by the few draws with
# the largest rates, and its error is x times the rounding of their log-rates.  Over all the input sets of
# test_gpu_predict.py the emulation's largest err / bound is between 0.42 and 0.76 for the bases 0..23 and under
# 0.5 for three of them; 14 has the least (tests/test_predict_emu_host.py asserts 0.5).
SEED_BASE = 14


def case(kind, S, T, M, pattern=None):
    """(venue, args, h, a, kw) of one input set; the seeds follow from the shape, so the device tests and the
    host test of the emulation see the same numbers."""
    seed = SEED_BASE + S + 7 * M + 13 * T
    venue, args = posterior(kind, S, T, seed=seed)
    if pattern is not None:
        venue, args = with_corr(venue, args, clipped_corr(pattern, args[6 if venue else 3]))
    return (venue, args) + fixtures(kind, M, T, seed=seed + 1)


def grid_bound(want):
    """The grid gate of tests/test_gpu_fit.py, per cell."""
    return 3e-6 * want + 1e-12


# ---- the walk
def _exp2(x):
    return np.exp2(x.astype(F64)).astype(F32)


def _fma(a, b, c):
    # float32 operands: the product is exact in float64, the sum is rounded once more to float32
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


class GridEmu:
    """predict_set_posterior[_venue] / predict_score_grid of HipContext, by the kernel's arithmetic."""

    def predict_set_posterior(self, attack, defence, home_advantage, corr_coef):
        self.att, self.dfn = np.asarray(attack).astype(F32), np.asarray(defence).astype(F32)
        self.ha, self.cc = np.asarray(home_advantage).astype(F32), np.asarray(corr_coef).astype(F32)
        self.venue = None

    def predict_set_posterior_venue(self, attack, defence, home_attack, away_attack, home_defence,
                                    away_defence, corr_coef, confederation_strength=None):
        self.att, self.dfn = np.asarray(attack).astype(F32), np.asarray(defence).astype(F32)
        self.venue = [np.asarray(t).astype(F32) for t in (home_attack, away_attack, home_defence, away_defence)]
        self.conf = None if confederation_strength is None else np.asarray(confederation_strength).astype(F32)
        self.cc = np.asarray(corr_coef).astype(F32)

    def _log_rates(self, h, a, neutral, conf):
        """[M, S] float32 each."""
        ah, aa, dh, da = self.att[:, h].T, self.att[:, a].T, self.dfn[:, h].T, self.dfn[:, a].T
        if self.venue is None:
            ha = self.ha[None, :] if self.ha.ndim == 1 else self.ha[:, h].T
            return (ah - da) + ha, aa - dh
        hat, aat, hdf, adf = self.venue
        on = (1 - np.broadcast_to(np.asarray(neutral), h.shape)).astype(F32)[:, None]   # 0 or 1: on * v is exact
        eh = ((ah - da) + on * hat[:, h].T) - on * adf[:, a].T
        ea = ((aa - dh) + on * aat[:, a].T) - on * hdf[:, h].T
        if self.conf is not None:
            hc = np.broadcast_to(np.asarray(conf[0], int), h.shape)
            ac = np.broadcast_to(np.asarray(conf[1], int), h.shape)
            dc = self.conf[:, hc].T - self.conf[:, ac].T
            eh, ea = eh + dc, ea - dc
        return eh, ea

    @staticmethod
    def _mfma_mean_sum(A, B):
        """sum over draws of A[m, s, x] B[m, s, y] as the kernel takes it: blocks of 64 draws, instruction g
        of a block the draws 16 k + g (k = 0..3) as one float32 fma chain, folded into float64 every 4 blocks."""
        M, S, nx = A.shape
        accd = np.zeros((M, nx, B.shape[2]), F64)
        acc = np.zeros_like(accd, dtype=F32)
        blocks = (S + 63) // 64
        for b in range(blocks):
            for g in range(16):
                for k in range(4):
                    s = 64 * b + 16 * k + g
                    if s < S:   # (a draw beyond S has pmf 0: the fma leaves the accumulator as it is)
                        acc = _fma(A[:, s, :, None], B[:, s, None, :], acc)
            if b % 4 == 3 or b == blocks - 1:
                accd += acc.astype(F64)
                acc[...] = 0
        return accd

    def predict_score_grid(self, h, a, max_goals, neutral=None, conf=None):
        h, a = np.asarray(h, int), np.asarray(a, int)
        G1, S = max_goals + 1, self.cc.size
        eh, ea = self._log_rates(h, a, neutral, conf)
        lh, la = _exp2(eh * LOG2E), _exp2(ea * LOG2E)
        ph, pa = _exp2(-lh * LOG2E), _exp2(-la * LOG2E)
        rk = (1.0 / (np.arange(64, dtype=F64) + 1.0)).astype(F32)

        def chain(p0, rate, n, factorials):
            out = np.empty(p0.shape + (n,), F32)
            out[..., 0] = p0
            for k in range(n - 1):
                out[..., k + 1] = out[..., k] * (rate * rk[k] if factorials else rate)
            return out

        out = self._mfma_mean_sum(chain(ph, lh, G1, True), chain(pa, la, G1, True))
        n0 = min(G1, 16)   # the first tile: no factorials in the strip, 1 / (x! y!) on the float64 cell
        low = self._mfma_mean_sum(chain(ph, lh, n0, False), chain(pa, la, n0, False))
        rfact = 1.0 / np.cumprod(np.concatenate([[1.0], np.arange(1.0, 16.0)]))
        out[:, :n0, :n0] = low * (rfact[:n0, None] * rfact[None, :n0])
        # the four tau cells: lane = draw % 64, one float32 fma chain per lane over the blocks
        rho = self.cc[None, :]
        zero, one = F32(0), np.ones_like(lh)
        p1h, p1a = ph * lh, pa * la
        cells = {(0, 0): (ph * pa, np.maximum(_fma(-(rho * lh), la, one), zero)),
                 (0, 1): (ph * p1a, np.maximum(_fma(rho * one, lh, one), zero)),
                 (1, 0): (p1h * pa, np.maximum(_fma(rho * one, la, one), zero)),
                 (1, 1): (p1h * p1a, np.maximum(one - rho, zero))}
        for (x, y), (p, tau) in cells.items():
            if x > max_goals or y > max_goals:
                continue
            lanes = np.zeros((h.size, 64), F32)
            for s0 in range(0, S, 64):
                n = min(64, S - s0)
                lanes[:, :n] = _fma(p[:, s0:s0 + n], tau[:, s0:s0 + n], lanes[:, :n])
            out[:, x, y] = lanes.astype(F64).sum(axis=1)
        return out * (1.0 / S)
