// dc_loo.hip.h -- leave-one-out forecasts of the fixtures a fit has seen: each fixture's own Pareto-smoothed
// importance weights (dc_loglik.hip.h: the weights PSIS-LOO forms from r = -ll) applied to that fixture's
// per-draw forecasts (dc_outcome.hip.h).  Per fixture n, with ll_s, p_s = (p_H, p_D, p_A) and the grid
// q_s(a, b) = max(1 + rho_s c(a, b), 0) Pois(a; lh) Pois(b; la) on 0..G (not renormalised) of draw s, the actual
// goals x, y and the weights w_s = exp(x_s) / sum exp(x_s), x_s the smoothed log ratios of loglik_summary (raw
// when nothing is smoothed):
//     proba      sum_s w_s p_s                       the leave-one-out forecast
//     proba_in   mean_s p_s                          what outcome_tiles (dc_score.hip.h) gives
//     elpd_loo   lse(x + ll) - lse(x), pareto_k, tail_len     as loglik_summary (the same lines)
//     ess        (sum w)^2 / sum w^2 of the unnormalised weights = 1 / sum_s w_s^2
//     pit        home (lower, upper), away (lower, upper): lower = sum_s w_s sum_{a < x} sum_b q_s(a, b), upper
//                the same with a <= x, a and b on 0..G (x > G: both are the weighted grid mass); away on the
//                other marginal with y.  The probability integral transform of the goal counts.
// A fixture with ll = -inf in some draw (a clipped tau cell) takes the limit of the definition: uniform weights
// over the draws with ll = -inf, 0 elsewhere; elpd_loo = -inf, pareto_k = +inf, tail_len = 0, ess = the number of
// such draws.  Nothing is NaN for finite tables.  DESIGN.md section 32.
//
// One kernel, loo_forecast: ONE WAVE PER FIXTURE, lane = draw on the TEAM-major tables, SUM_WAVES waves per
// workgroup, the LDS of loglik_summary.  Passes over the draws, each recomputing ll (dcl::ll_at):
//   1  min of ll (loglik_summary's max, sum and second moment are not needed)
//   2  the first digit's histogram of x = min ll - ll, then dcl::psis_tail with the lambda loglik_summary passes;
//      the L smoothed tail values (dcl::psis_smoothed) overwrite the tail's z values in LDS, so that the
//      quantile's log1p, expm1 and log are over before the sums below are live (registers)
//   f  in the draw order of loglik_summary's pass f: per lane the draws lane, lane + 64, ... outside the smoothed
//      tail, then the tail entries lane, lane + 64, ... with their smoothed values.  Per draw: ll, the log rates,
//      the weight exp(x_s), dcs::outcome_probs and the four marginal sums (marginal_cdfs: a second, smaller
//      walk over k), into
//        nine plain sums     sum w, sum w^2, sum w p (3), sum w cdf (4)
//        three plain sums    sum p
//        two running lse     (x) and (x + ll): elpd_loo exactly as loglik_summary forms it
//      then xor butterflies (dcl::wave_sum, dcl::wave_lse) and one division by sum w.
// A fixture with a -inf draw skips pass 2 and runs pass f with weights 1 (ll = -inf) and 0.
//
// Why plain sums of exp(x_s) are safe.  Every x_s is <= 0, so no term exceeds 1 and nothing overflows.  The sum
// cannot vanish either: (a) when nothing is smoothed the draw with the smallest ll has x_s = min ll - ll_s = 0
// exactly, a weight of 1; (b) a smoothed tail draw had x_s > cutoff >= log DBL_MIN before smoothing and has
// log(q + exp(cutoff)) with q > 0 after it, so its weight is at least exp(cutoff) >= DBL_MIN, a normal number,
// and the largest of them is the GPD quantile at 1 - 1/(2L) of exceedances z = exp(x) - exp(cutoff) whose own
// maximum is 1 - exp(cutoff): of order one.  Draws far below carry weights that round to 0 next to it, which is
// what the lse form would give them as well.  In the -inf case the weights are 0 or 1 and at least one is 1.
// No floating-point atomics; every sum has a fixed order that does not depend on where the fixture stands in
// the query: results are bit-identical from run to run and under a permutation of the fixtures.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_loglik.hip.h"    // dcl::Fix, make_fix, ll_at, log_rates_at, psis_tail, psis_smoothed, the wave helpers
#include "dc_outcome.hip.h"   // dcs::outcome_probs, SCORE_MAX_GOALS

namespace dcloo {

struct LooArgs {
    dcq::Posterior<double> P;   // TEAM-major
    dcq::Queries Q;             // the fixtures with their actual goals
    double* elpd_loo;           // [M] each
    double* pareto_k;
    double* ess;
    int32_t* tail_len;
    double* proba;              // [M, 3]
    double* proba_in;           // [M, 3]
    double* pit;                // [M, 4]
    int G;
    int tail_m;                 // as dcl::LoglikArgs
    double log_dbl_min;
    double rk[dcs::SCORE_MAX_GOALS + 1];   // rk[k] = 1 / k (k >= 1)
};

// The marginal sums of one draw's grid at the actual goals x, y: c[0] = sum_{a < x} sum_b q(a, b), c[1] the same
// with a <= x, c[2] and c[3] on the away marginal with y.  The rows a >= 2 carry no tau cell, so their sum over
// b is Pois(a; lh) times the away mass on 0..G; the rows 0 and 1 are written out with the tau factors of
// dcs::outcome_probs (a clipped cell is exactly 0).  O(G).
__device__ __forceinline__ void marginal_cdfs(double eh, double ea, double rho, int G, const double* rk, int x, int y,
                                              double* c) {
#pragma clang fp contract(off)
    const double lh = exp(eh), la = exp(ea);
    const double u0 = exp(-lh), v0 = exp(-la);
    const double u1 = G >= 1 ? u0 * lh : 0.0, v1 = G >= 1 ? v0 * la : 0.0;   // (G = 0: the grid is one cell)
    const double q00 = fmax(1.0 + rho * -(lh * la), 0.0) * (u0 * v0);
    const double q10 = fmax(1.0 + rho * la, 0.0) * (u1 * v0);
    const double q01 = fmax(1.0 + rho * lh, 0.0) * (u0 * v1);
    const double q11 = fmax(1.0 + rho * -1.0, 0.0) * (u1 * v1);
    double u = u1, v = v1;
    double su = 0.0, sv = 0.0;   // Pois over 2..G
    double bu = 0.0, bv = 0.0;   // ... over 2..min(x, G + 1) - 1 and 2..min(y, G + 1) - 1
    double au = 0.0, av = 0.0;   // Pois(x), Pois(y) when the actual count is in 2..G
#pragma unroll 1
    for (int k = 2; k <= G; ++k) {
        const double r = rk[k];
        u = u * (lh * r);
        v = v * (la * r);
        su = su + u;
        sv = sv + v;
        bu = bu + (k < x ? u : 0.0);
        bv = bv + (k < y ? v : 0.0);
        au = k == x ? u : au;
        av = k == y ? v : av;
    }
    const double mu = (u0 + u1) + su, mv = (v0 + v1) + sv;   // the masses on 0..G
    const double h0 = (q00 + q01) + u0 * sv, h1 = (q10 + q11) + u1 * sv;   // home rows 0 and 1
    const double a0 = (q00 + q10) + v0 * su, a1 = (q01 + q11) + v1 * su;   // away columns 0 and 1
    const double hlo = (x > 0 ? h0 : 0.0) + (x > 1 ? h1 : 0.0) + bu * mv;
    const double alo = (y > 0 ? a0 : 0.0) + (y > 1 ? a1 : 0.0) + bv * mu;
    // fmax as in outcome_probs: a rate beyond float64 gives 0, not NaN
    c[0] = fmax(hlo, 0.0);
    c[1] = fmax(hlo + (x == 0 ? h0 : (x == 1 ? h1 : au * mv)), 0.0);
    c[2] = fmax(alo, 0.0);
    c[3] = fmax(alo + (y == 0 ? a0 : (y == 1 ? a1 : av * mu)), 0.0);
}

template <bool VENUE>
__global__ __launch_bounds__(64 * dcl::SUM_WAVES) void loo_forecast(LooArgs A) {
    __shared__ unsigned long long tkey[dcl::SUM_WAVES][dcl::LOGLIK_MAX_TAIL];   // tail keys, then the tail's z values
    __shared__ uint16_t tidx[dcl::SUM_WAVES][dcl::LOGLIK_MAX_TAIL];             // tail draws
    __shared__ uint32_t hist[dcl::SUM_WAVES][256];
    __shared__ double cut[dcl::SUM_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long n = (long long)blockIdx.x * dcl::SUM_WAVES + w;
    if (n >= A.Q.M) return;   // (wave uniform; no workgroup barrier below)
    const dcl::Fix F = dcl::make_fix<VENUE>(A.P, A.Q, n);
    const int S = A.P.S;

    // pass 1: the min of ll (loglik_summary's max, sum and pass-2 moments are not needed)
    double mn = INFINITY;
    for (int s = lane; s < S; s += 64) mn = fmin(mn, dcl::ll_at<VENUE>(F, s));
    mn = dcl::wave_min(mn);
    const bool bad = __ballot(!(mn > -INFINITY)) != 0ull;   // some draw has ll = -inf (a scalar: the wave agrees)

    // the selection's first digit, then the selection, gather, sort and fit: the call of loglik_summary.  The sums
    // of the final pass start after it, so that they are not live across the fit.
    dcl::PsisTail T{};
    T.kk = INFINITY;
    if (!bad) {
        uint32_t* hw = hist[w];
        for (int i = lane; i < 256; i += 64) hw[i] = 0u;
        dcl::wave_lds_order();
        for (int s = lane; s < S; s += 64) atomicAdd(&hw[dcl::key_of(dcl::x_of(mn, dcl::ll_at<VENUE>(F, s))) >> 56], 1u);
        T = dcl::psis_tail([&](int s) { return dcl::x_of(mn, dcl::ll_at<VENUE>(F, s)); }, S, A.tail_m, A.log_dbl_min, lane,
                           hw, tkey[w], tidx[w], &cut[w]);
    }
    const uint16_t* iw = tidx[w];
    unsigned long long* kw = tkey[w];
    const int L = T.L;
    const double kk = T.kk;
    const bool smooth = kk < INFINITY;   // (L > 4 and a usable fit; never with a -inf draw)
    // the smoothed tail values take the place of the tail's z values (as bits), so that the quantile's log1p,
    // expm1 and log are done with before the sums of the final pass are live
    if (smooth) {
        dcl::wave_lds_order();
        for (int i = lane; i < L; i += 64) kw[T.base + i] = (unsigned long long)__double_as_longlong(dcl::psis_smoothed(T, i));
        dcl::wave_lds_order();
    }

    // the 9 + 3 plain sums and the two lse pairs of one lane
    double sw = 0.0, sw2 = 0.0, wp[3] = {0.0, 0.0, 0.0}, wc[4] = {0.0, 0.0, 0.0, 0.0}, sp[3] = {0.0, 0.0, 0.0};
    double ma = -INFINITY, sa = 0.0, mb = -INFINITY, sb = 0.0;
    auto take = [&](int s, double wt) {
        double eh, ea, pH, pD, pA, c[4];
        dcl::log_rates_at<VENUE>(F, s, &eh, &ea);
        const double rho = F.corr[s];
        dcs::outcome_probs(eh, ea, rho, A.G, A.rk, &pH, &pD, &pA);
        marginal_cdfs(eh, ea, rho, A.G, A.rk, F.x, F.y, c);
        sw += wt;
        sw2 += wt * wt;
        wp[0] += wt * pH;
        wp[1] += wt * pD;
        wp[2] += wt * pA;
#pragma unroll
        for (int k = 0; k < 4; ++k) wc[k] += wt * c[k];
        sp[0] += pH;
        sp[1] += pD;
        sp[2] += pA;
    };
    // the final pass, in the order of loglik_summary's pass f.  With a -inf draw: the limit, weight 1 on the draws
    // with ll = -inf and 0 on the others
#pragma unroll 1
    for (int s = lane; s < S; s += 64) {
        const double v = dcl::ll_at<VENUE>(F, s);
        double wt;
        if (bad) {
            wt = v > -INFINITY ? 0.0 : 1.0;
        } else {
            const double x = dcl::x_of(mn, v);
            if (smooth && x > T.cutoff) continue;   // a tail draw: below
            dcl::lse_add(ma, sa, x);
            dcl::lse_add(mb, sb, x + v);
            wt = exp(x);
        }
        take(s, wt);
    }
    if (smooth) {
#pragma unroll 1
        for (int i = lane; i < L; i += 64) {
            const int s = iw[T.base + i];
            const double v = dcl::ll_at<VENUE>(F, s);
            const double x = __longlong_as_double((long long)kw[T.base + i]);
            dcl::lse_add(ma, sa, x);
            dcl::lse_add(mb, sb, x + v);
            take(s, exp(x));
        }
    }

    sw = dcl::wave_sum(sw);
    sw2 = dcl::wave_sum(sw2);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        wp[k] = dcl::wave_sum(wp[k]);
        sp[k] = dcl::wave_sum(sp[k]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) wc[k] = dcl::wave_sum(wc[k]);
    double elpd = -INFINITY;
    if (!bad) {
        const double lse_x = dcl::wave_lse(ma, sa), lse_xl = dcl::wave_lse(mb, sb);
        elpd = lse_xl - lse_x;
    }
    if (lane == 0) {
        A.elpd_loo[n] = elpd;
        A.pareto_k[n] = kk;
        A.tail_len[n] = L;
        A.ess[n] = (sw * sw) / sw2;
    }
    // lanes 0..2 the forecast, 3..5 the in-sample forecast, 6..9 the transform
    if (lane < 3) A.proba[n * 3 + lane] = (lane == 0 ? wp[0] : (lane == 1 ? wp[1] : wp[2])) / sw;
    else if (lane < 6) A.proba_in[n * 3 + (lane - 3)] = (lane == 3 ? sp[0] : (lane == 4 ? sp[1] : sp[2])) / (double)S;
    else if (lane < 10) A.pit[n * 4 + (lane - 6)] = (lane == 6 ? wc[0] : (lane == 7 ? wc[1] : (lane == 8 ? wc[2] : wc[3]))) / sw;
}

}  // namespace dcloo
