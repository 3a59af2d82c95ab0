// dc_score.hip.h -- proper scoring rules of a fitted model's win / draw / loss forecasts on the device:
// the per-draw outcome probabilities of every (posterior draw s, fixture n), reduced over BOTH axes
// without ever storing the [draws, fixtures, 3] array.  Per draw and fixture, in float64:
//     q(x, y) = max(1 + rho_s c(x, y), 0) Pois(x; lh) Pois(y; la)      on 0 <= x, y <= G (not renormalised)
//     p_H, p_D, p_A = the sums of q over x > y, x = y, x < y
// with the rates of dcl::log_rates_at (the product forms of dc_posterior.hip.h, read from the TEAM-major
// float64 copies, lane = draw) and the tau coefficient c of dcl::ll_at.  Outputs:
//     proba[n, 3]      mean over the draws of (p_H, p_D, p_A): what predict_outcome_proba averages
//     draw_sums[s, 3]  sum over the fixtures of log p_o, sum_k (p_k - 1[k = o])^2 and
//                      ((p_H - o_H)^2 + (p_H + p_D - o_H - o_D)^2) / 2 of draw s's OWN p, o the observed class
//
// O(G) per (draw, fixture): one walk over k carries u = Pois(k; lh), v = Pois(k; la) and their running
// sums below k; u (sum of v below k), v (sum of u below k) and u v accumulate the three triangles.  The four
// tau cells (0,0), (0,1), (1,0), (1,1) are the terms of depths 0 and 1 (at G = 0 only (0,0) exists): those
// two depths are written out, each cell times max(1 + rho c, 0), and the walk runs from k = 2.  (Equal to
// correcting the plain sums by (max(1 + rho c, 0) - 1) Pois Pois afterwards, except that a clipped cell
// contributes an exact 0.)  1 / k comes from a table in the kernel arguments.
//
// Two kernels:
//   outcome_tiles   A wave owns 128 draws (lane = draw, two per lane: SCORE_D) x SCORE_NF = 128 fixtures.
//       It walks its fixtures; per fixture the two draws' p are added and summed over the wave (xor
//       butterflies) into p_part[draw tile][n][3]; per lane the three rules accumulate in registers
//       over the fixtures into d_part[fixture tile][3][s].  The four waves of a workgroup share the
//       fixture tile (its query columns and row pointers are scalar) and take neighbouring draw tiles.
//       Registers only: no LDS, no scratch, no barrier.
//   outcome_reduce  adds the tiles in index order, one thread per output element, and divides the
//       probabilities by S.
// No floating-point atomics; every sum has a fixed order: results are bit-identical from run to run, and
// a fixture's probabilities do not depend on where it stands in the query.  Each p is computed once, so
// nothing has to agree across passes; the walk is still written with contraction off and explicit fma,
// so that the two unrolled draws of a lane run the same operations.
// The partials take 3/8 byte per (draw, fixture) (the log-likelihood matrix takes 8).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_loglik.hip.h"   // dcl::Fix, fix_rows, log_rates_at, wave_sum
#include "dc_outcome.hip.h"  // dcs::outcome_probs, SCORE_MAX_GOALS

namespace dcs {

constexpr int SCORE_D = 2;            // draws per lane
constexpr int SCORE_DRAWS = 64 * SCORE_D;
constexpr int SCORE_NF = 128;         // fixtures per wave
constexpr int SCORE_WAVES = 4;

struct ScoreArgs {
    dcq::Posterior<double> P;   // TEAM-major
    dcq::Queries Q;             // the fixtures with their actual goals
    int G;
    int TS, TN;                 // draw tiles ceil(S / SCORE_DRAWS), fixture tiles ceil(M / SCORE_NF)
    double* p_part;             // [TS, M, 3]
    double* d_part;             // [TN, 3, S]
    double* proba;              // [M, 3]
    double* draw_sums;          // [S, 3]
    double rk[SCORE_MAX_GOALS + 1];   // rk[k] = 1 / k (k >= 1)
};

template <bool VENUE>
__global__ __launch_bounds__(64 * SCORE_WAVES) void outcome_tiles(ScoreArgs A) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ts = blockIdx.y * SCORE_WAVES + wave;
    const int S = A.P.S;
    const long long M = A.Q.M;
    if (ts >= A.TS) return;   // (wave uniform; no barrier below)
    const long long n0 = (long long)blockIdx.x * SCORE_NF;
    const long long n1 = n0 + SCORE_NF < M ? n0 + SCORE_NF : M;
    double dsum[SCORE_D][3];
#pragma unroll
    for (int d = 0; d < SCORE_D; ++d) dsum[d][0] = dsum[d][1] = dsum[d][2] = 0.0;
#pragma unroll 1
    for (long long n = n0; n < n1; ++n) {
        const dcl::Fix F = dcl::fix_rows<VENUE>(A.P, A.Q, n);
        const int x = A.Q.x[n], y = A.Q.y[n];
        const int o = x > y ? 0 : (x == y ? 1 : 2);
        const double oh = o == 0 ? 1.0 : 0.0, od = o == 1 ? 1.0 : 0.0, oa = o == 2 ? 1.0 : 0.0;
        double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int d = 0; d < SCORE_D; ++d) {
            const int s = ts * SCORE_DRAWS + d * 64 + lane;
            if (s < S) {
                double eh, ea, pH, pD, pA;
                dcl::log_rates_at<VENUE>(F, s, &eh, &ea);
                outcome_probs(eh, ea, F.corr[s], A.G, A.rk, &pH, &pD, &pA);
                acc[0] += pH;
                acc[1] += pD;
                acc[2] += pA;
                const double po = o == 0 ? pH : (o == 1 ? pD : pA);
                const double bh = pH - oh, bd = pD - od, ba = pA - oa;
                const double c2 = (pH + pD) - (oh + od);
                dsum[d][0] += log(po);   // (log 0 = -inf stays -inf; nothing here is +inf)
                dsum[d][1] += bh * bh + bd * bd + ba * ba;
                dsum[d][2] += 0.5 * (bh * bh + c2 * c2);
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] = dcl::wave_sum(acc[k]);
        if (lane < 3) A.p_part[((size_t)ts * (size_t)M + (size_t)n) * 3 + lane] = lane == 0 ? acc[0] : (lane == 1 ? acc[1] : acc[2]);
    }
#pragma unroll
    for (int d = 0; d < SCORE_D; ++d) {
        const int s = ts * SCORE_DRAWS + d * 64 + lane;
        if (s < S) {
#pragma unroll
            for (int k = 0; k < 3; ++k) A.d_part[((size_t)blockIdx.x * 3 + k) * (size_t)S + s] = dsum[d][k];
        }
    }
}

// one thread per element of proba [M, 3], then of draw_sums [S, 3]
__global__ __launch_bounds__(256) void outcome_reduce(ScoreArgs A) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t M3 = (size_t)A.Q.M * 3, S = (size_t)A.P.S;
    if (i < M3) {
        double t = 0.0;
        for (int ts = 0; ts < A.TS; ++ts) t += A.p_part[(size_t)ts * M3 + i];
        A.proba[i] = t / (double)A.P.S;
    } else if (i < M3 + 3 * S) {
        const size_t j = i - M3, k = j / S, s = j - k * S;
        double t = 0.0;
        for (int tn = 0; tn < A.TN; ++tn) t += A.d_part[((size_t)tn * 3 + k) * S + s];
        A.draw_sums[s * 3 + k] = t;
    }
}

}  // namespace dcs
