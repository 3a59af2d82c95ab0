// dc_period.hip.h -- period markets of a fitted model on the device: markets on the score at a split of the
// match (half time, the hour, the tenth minute) TOGETHER with the final score.  Goal times are exchangeable
// within a match (dc_inplay.hip.h), so a side's goals before the share f of the match's scoring are
// Binomial(final goals, f) and Pois(x; l) Binom(a; x, f) = Pois(a; f l) Pois(x - a; (1 - f) l): the joint law
// of the score (a, b) at the split and the final score (x, y) is fixed by the law dc_market.hip.h sums.  Per
// posterior draw s, fixture n and market k with float64 weights W_k[a, b, x, y]:
//     v[s, k, n]    = sum W_k[a, b, x, y] p(a, b, x, y)       over 0 <= a <= x <= G, 0 <= b <= y <= G
//     p(a, b, x, y) = F(x, y) Pois(a; f lh) Pois(x - a; (1 - f) lh) Pois(b; f la) Pois(y - b; (1 - f) la)
//     F(x, y)       = max(1 + rho_s c(x, y), 0) on {0, 1}^2, else 1
// with the FULL-MATCH rates of dcl::log_rates_at and the tau coefficient c of dcl::ll_at on the FINAL score.
// Not renormalised and truncated by the final score only, so sum_{a, b} p = q of dc_market.hip.h for every f.
// Pois(0; 0) = 1 and Pois(k > 0; 0) = 0 fall out of the recurrences (no logarithm of f or 1 - f is taken): f = 0
// and f = 1 are legal.  Everything in float64.
//
// period_values keeps dcm::market_values' structure: lane = draw on the team-major tables; the four waves of a
// workgroup share one fixture and one pass of PERIOD_KPASS markets and take neighbouring draw tiles, so the row
// pointers, the split and the weights are wave-uniform.  The grid is rank one in four factors,
// u1_a u2_c v1_b v2_d with c = x - a and d = y - b, apart from the F factor.  The walk (period_walk below, which
// the host uses to pack the weights): blocks of PERIOD_DB second-period away counts d, whose v2_d (Poisson
// recurrence, 1 / k from the table in the kernel arguments) stay in registers; inside a block the home pairs
// (a, c), a + c <= G, with h = u1_a u2_c carried by ONE multiplication per step of c; inside a pair the
// first-period away counts b, b + d0 <= G, with hb = h v1_b carried by one multiplication per step of b (plus
// one for la1 / b); inside that the block's d with b + d <= G: one multiplication (hb v2_d) and one fma per
// market per cell.  So a cell costs 1 + PERIOD_KPASS float64 instructions and a step of b two more:
// 9.25 per cell and pass at PERIOD_DB = 8 on full blocks, as market_values.  F is applied by FINAL cell: the
// block d0 = 0 with a + c <= 1 and b <= 1 holds the nine (a, b, c, d) combinations that end in {0, 1}^2 (one
// for 0-0, two each for 1-0 and 0-1, four for 1-1) and each is multiplied by its cell's factor; a clipped cell
// contributes an exact 0.  The weights are read in walk order from a [pass][cell][PERIOD_KPASS] copy of the
// READABLE cells only (a cell's PERIOD_KPASS weights are one wave-uniform 64-byte load; the tail of the last pass
// holds zeros).  Registers only: no LDS, no scratch, no barrier; vector stores only.  The values go to
// vals[fixture of the chunk][k][s], draws contiguous, and dcm::market_summary summarises them.
// A value's accumulation order depends on nothing but its own (draw, fixture, market): results are bit-identical
// from run to run, under any chunking of the fixtures and under any order of the fixtures.  Contraction is off
// and every fma is explicit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_market.hip.h"   // dcm::MarketArgs, market_summary; dcl::Fix, fix_rows, log_rates_at

namespace dcpd {

constexpr int PERIOD_MAX_GOALS = 31;     // include/bplhip.h BPLHIP_PERIOD_MAX_GOALS
constexpr int PERIOD_MAX_MARKETS = 32;   // include/bplhip.h BPLHIP_PERIOD_MAX_MARKETS
constexpr int PERIOD_KPASS = dcm::MARKET_KPASS;
constexpr int PERIOD_DB = 8;             // second-period away counts per block
constexpr int PERIOD_WAVES = dcm::MARKET_WAVES;

struct PeriodArgs {
    dcm::MarketArgs M;     // as market_values reads it, but M.w is [ceil(K / PERIOD_KPASS)][T^2][PERIOD_KPASS], T = (G+1)(G+2)/2
    const double* split;   // [M.Q.M]: the share of the match's scoring before the split, in [0, 1]
};

// the readable cells (a, b, x, y) in the order period_values walks them: fn(a, b, x, y) for each of the T^2
template <class Fn>
inline void period_walk(int G, Fn&& fn) {
    for (int d0 = 0; d0 <= G; d0 += PERIOD_DB)
        for (int a = 0; a <= G; ++a)
            for (int c = 0; a + c <= G; ++c)
                for (int b = 0; b + d0 <= G; ++b)
                    for (int j = 0; j < PERIOD_DB && b + d0 + j <= G; ++j) fn(a, b, a + c, b + d0 + j);
}

// grid: (fixture of the chunk, draw tile group, pass)
template <bool VENUE>
__global__ __launch_bounds__(64 * PERIOD_WAVES) void period_values(PeriodArgs P) {
#pragma clang fp contract(off)
    const dcm::MarketArgs& A = P.M;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int S = A.P.S, G = A.G;
    const int s = (blockIdx.y * PERIOD_WAVES + wave) * 64 + lane;
    const long long f = blockIdx.x;
    const int pass = blockIdx.z;
    if (s >= S) return;   // (no barrier below)
    const dcl::Fix F = dcl::fix_rows<VENUE>(A.P, A.Q, A.n0 + f);
    double eh, ea;
    dcl::log_rates_at<VENUE>(F, s, &eh, &ea);
    const double rho = F.corr[s];
    const double lh = exp(eh), la = exp(ea);
    const double sp = P.split[A.n0 + f], rs = 1.0 - sp;   // (uniform; 0 and 1 are exact)
    const double lh1 = sp * lh, lh2 = rs * lh, la1 = sp * la, la2 = rs * la;
    const double u10 = exp(-lh1), u20 = exp(-lh2), v10 = exp(-la1), v20 = exp(-la2);   // (exp(-0) = 1)
    // the tau factors of the FINAL scores (0,0), (0,1), (1,0), (1,1) with the full-match rates (c as in dcl::ll_at)
    const double t00 = fmax(1.0 + rho * -(lh * la), 0.0), t01 = fmax(1.0 + rho * lh, 0.0);
    const double t10 = fmax(1.0 + rho * la, 0.0), t11 = fmax(1.0 + rho * -1.0, 0.0);
    const size_t T = (size_t)(G + 1) * (size_t)(G + 2) / 2;
    const double* __restrict__ wc = A.w + (size_t)pass * T * T * PERIOD_KPASS;   // the next cell of the walk
    double acc[PERIOD_KPASS];
#pragma unroll
    for (int k = 0; k < PERIOD_KPASS; ++k) acc[k] = 0.0;
    double vd = v20;   // Pois(d0; la2) of the block's first count
#pragma unroll 1
    for (int d0 = 0; d0 <= G; d0 += PERIOD_DB) {
        double v[PERIOD_DB];
        v[0] = d0 == 0 ? v20 : vd * (la2 * A.rk[d0]);
#pragma unroll
        for (int j = 1; j < PERIOD_DB; ++j) v[j] = d0 + j <= G ? v[j - 1] * (la2 * A.rk[d0 + j]) : 0.0;
        vd = v[PERIOD_DB - 1];
        const int nb = G - d0;   // b = 0 .. nb
        double u1 = u10;
#pragma unroll 1
        for (int a = 0; a <= G; ++a) {
            if (a > 0) u1 = u1 * (lh1 * A.rk[a]);
            double h = u1 * u20;
#pragma unroll 1
            for (int c = 0; a + c <= G; ++c) {
                if (c > 0) h = h * (lh2 * A.rk[c]);
                const int x = a + c;
                double hb = h * v10;
#pragma unroll 1
                for (int b = 0; b <= nb; ++b) {
                    if (b > 0) hb = hb * (la1 * A.rk[b]);
                    const int nj = nb - b + 1 < PERIOD_DB ? nb - b + 1 : PERIOD_DB;   // (uniform)
                    if (d0 == 0 && x <= 1 && b <= 1) {
                        // the cells that end in {0, 1}^2: y = b + j <= 1 carries the factor of the final (x, y)
                        const double f0 = x == 0 ? (b == 0 ? t00 : t01) : (b == 0 ? t10 : t11);
                        const double f1 = x == 0 ? t01 : t11;   // (j = 1 ends in y = 1 only from b = 0)
#pragma unroll
                        for (int j = 0; j < PERIOD_DB; ++j) {
                            if (j < nj) {
                                double t = hb * v[j];
                                if (j == 0) t = f0 * t;
                                if (j == 1 && b == 0) t = f1 * t;
#pragma unroll
                                for (int k = 0; k < PERIOD_KPASS; ++k) acc[k] = fma(wc[j * PERIOD_KPASS + k], t, acc[k]);
                            }
                        }
                    } else if (nj == PERIOD_DB) {
#pragma unroll
                        for (int j = 0; j < PERIOD_DB; ++j) {
                            const double t = hb * v[j];
#pragma unroll
                            for (int k = 0; k < PERIOD_KPASS; ++k) acc[k] = fma(wc[j * PERIOD_KPASS + k], t, acc[k]);
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < PERIOD_DB; ++j) {
                            if (j < nj) {
                                const double t = hb * v[j];
#pragma unroll
                                for (int k = 0; k < PERIOD_KPASS; ++k) acc[k] = fma(wc[j * PERIOD_KPASS + k], t, acc[k]);
                            }
                        }
                    }
                    wc += (size_t)nj * PERIOD_KPASS;
                }
            }
        }
    }
    const int k0 = pass * PERIOD_KPASS;
    double* out = A.vals + ((size_t)f * (size_t)A.K + (size_t)k0) * (size_t)S + (size_t)s;
#pragma unroll
    for (int k = 0; k < PERIOD_KPASS; ++k)
        if (k0 + k < A.K) out[(size_t)k * (size_t)S] = acc[k] + 0.0;   // (+ 0.0: never -0)
}

}  // namespace dcpd
