// dc_ratings.hip.h -- team ratings of a fitted model on the device: how a team does against a FIELD of
// opponents, formed PER DRAW and then summarised over the draws, and the rank of every rated team per draw
// (a rank exists only per draw: none of this can be put together from posterior means).
// Per posterior draw s and rated team t, over the n_t matches t plays against the opponents o != t, walked in
// the order given (venue 0 "both": t hosts o, then o hosts t; 1 "home"; 2 "away"; 3 "neutral": t listed first on
// neutral ground, venue form only), with the log rates of dcl::log_rates_at and (p_H, p_D, p_A) of
// dcs::outcome_probs at depth G, seen from t's side:
//     points          sum (W p_win + D p_draw + L p_loss) / n_t        (left to right)
//     win             sum p_win / n_t
//     goals_for       sum exp(t's log rate) / n_t                      (the marginal mean of the UNCLIPPED law: tau
//     goals_against   sum exp(the opponent's log rate) / n_t            leaves the marginals Poisson; not truncated at G)
//     goal_difference (sum goals_for - sum goals_against) / n_t
// Everything in float64 with contraction off; every sum runs in match order.
//
// Two kernels (the summary over the draws is dcm::market_summary on the stored values, K = 5, M = R):
//   ratings_values  lane = draw on the team-major tables; ONE WAVE PER (rated team, 64-draw tile), the four waves
//       of a workgroup take neighbouring draw tiles; the opponents are wave-uniform, so the row pointers come
//       from scalar loads.  Four running sums per lane (the difference is formed from two of them at the end).
//       Registers only: no LDS, no scratch, no barrier.  The values go to vals[team of the chunk][k][s], draws
//       contiguous (the layout market_summary reads), and the ranked statistic to ranked[team][s], which stays
//       resident over the chunks.
//   ratings_rank    ONE WAVE PER RATED TEAM t over ranked[R][S]: lanes walk the draws in tiles of 64 holding
//       v_t[s]; the wave loops over u reading v_u[s] (coalesced 512 B) and counts, per lane, the teams ahead of t
//       in that draw: those with a strictly larger value plus those with an equal value listed earlier, so a
//       draw's ranks are a permutation.  better[u] += popcount(ballot(v_t > v_u)) goes to a wave-uniform LDS
//       counter and the rank histogram of t is built with integer LDS atomics.  The tiles of draws are dealt over
//       gridDim.y workgroups per team, each adding its two int32 rows to the zeroed outputs with integer atomics
//       at the end.  Integers only: the counts are exact and order-free.  LDS: 2 x RATINGS_MAX_TEAMS x 4 B per
//       wave, 32 KB per workgroup; no scratch, no workgroup barrier.
// No floating-point atomics: results are bit-identical from run to run and under any chunking of the teams.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_loglik.hip.h"    // dcl::Fix, fix_rows_of, log_rates_at, wave_lds_order
#include "dc_outcome.hip.h"   // dcs::outcome_probs

namespace dcr {

constexpr int RATINGS_MAX_TEAMS = 1024;   // include/bplhip.h BPLHIP_RATINGS_MAX_TEAMS
constexpr int RATINGS_STATS = 5;          // points, win, goals_for, goals_against, goal_difference
constexpr int RATINGS_WAVES = 4;
constexpr int RATINGS_BOTH = 0, RATINGS_HOME = 1, RATINGS_AWAY = 2, RATINGS_NEUTRAL = 3;

struct RatingsArgs {
    dcq::Posterior<double> P;    // TEAM-major
    int R, NO;                   // rated teams, opponents
    int venue, G, rank_by;
    long long t0, tc;            // the chunk: rated teams t0 .. t0 + tc - 1
    const uint16_t *team, *tconf;   // [R] model indices (confederations: null without them)
    const uint16_t *opp, *oconf;    // [NO]
    double pw, pd, pl;           // points of a win, a draw, a loss
    double* vals;                // [tc, RATINGS_STATS, S]
    double* ranked;              // [R, S]: the rank_by statistic
    int32_t* rank_count;         // [R, R], zeroed before ratings_rank
    int32_t* better_count;       // [R, R], likewise
    double rk[dcs::SCORE_MAX_GOALS + 1];   // rk[k] = 1 / k (k >= 1)
};

// grid: (rated team of the chunk, draw tile group)
template <bool VENUE>
__global__ __launch_bounds__(64 * RATINGS_WAVES) void ratings_values(RatingsArgs A) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int S = A.P.S;
    const int s = (blockIdx.y * RATINGS_WAVES + wave) * 64 + lane;
    const long long f = blockIdx.x;
    if (s >= S) return;   // (no barrier below)
    const int t = A.team[A.t0 + f];
    const int tcf = A.tconf ? A.tconf[A.t0 + f] : 0;
    const double rho = A.P.corr[s];
    const int neutral = A.venue == RATINGS_NEUTRAL ? 1 : 0;
    double pts = 0.0, win = 0.0, gf = 0.0, ga = 0.0;
    int n = 0;
#pragma unroll 1
    for (int o = 0; o < A.NO; ++o) {
        const int u = A.opp[o];
        if (u == t) continue;   // (wave uniform) a team never meets itself
        const int ucf = A.oconf ? A.oconf[o] : 0;
#pragma unroll 1
        for (int leg = 0; leg < 2; ++leg) {
            // leg 0: t listed first (hosting, or on neutral ground); leg 1: t visiting
            if (leg == 0 ? A.venue == RATINGS_AWAY : (A.venue != RATINGS_BOTH && A.venue != RATINGS_AWAY)) continue;
            const bool first = leg == 0;
            const dcl::Fix F = first ? dcl::fix_rows_of<VENUE>(A.P, t, u, neutral, tcf, ucf)
                                     : dcl::fix_rows_of<VENUE>(A.P, u, t, 0, ucf, tcf);
            double eh, ea, pH, pD, pA;
            dcl::log_rates_at<VENUE>(F, s, &eh, &ea);
            dcs::outcome_probs(eh, ea, rho, A.G, A.rk, &pH, &pD, &pA);
            const double lh = exp(eh), la = exp(ea);
            const double p_win = first ? pH : pA, p_loss = first ? pA : pH;
            pts = pts + (A.pw * p_win + A.pd * pD + A.pl * p_loss);
            win = win + p_win;
            gf = gf + (first ? lh : la);
            ga = ga + (first ? la : lh);
            ++n;
        }
    }
    const double nd = (double)n;   // (>= 1: checked on the host)
    double v[RATINGS_STATS];
    v[0] = pts / nd + 0.0;   // (+ 0.0: never -0, dcl::key_of)
    v[1] = win / nd + 0.0;
    v[2] = gf / nd + 0.0;
    v[3] = ga / nd + 0.0;
    v[4] = (gf - ga) / nd + 0.0;
    double* out = A.vals + (size_t)f * RATINGS_STATS * (size_t)S + (size_t)s;
    double ranked = v[0];
#pragma unroll
    for (int k = 0; k < RATINGS_STATS; ++k) {
        out[(size_t)k * (size_t)S] = v[k];
        if (k == A.rank_by) ranked = v[k];
    }
    A.ranked[(size_t)(A.t0 + f) * (size_t)S + (size_t)s] = ranked;
}

// grid: (ceil(R / RATINGS_WAVES), draw slices); wave -> rated team, the workgroups of a column take every
// gridDim.y-th tile of 64 draws.  rank_count and better_count arrive zeroed and take each wave's rows through
// integer atomics (exact, and the same sum in any order).  It reads stored values only; VENUE names the rate form
// of the entry that launched it, so that a kernel trace tells the two apart
template <bool VENUE>
__global__ __launch_bounds__(64 * RATINGS_WAVES) void ratings_rank(RatingsArgs A) {
    __shared__ uint32_t hist[RATINGS_WAVES][RATINGS_MAX_TEAMS];     // draws in which t held rank r
    __shared__ uint32_t better[RATINGS_WAVES][RATINGS_MAX_TEAMS];   // draws with v_t > v_u
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int R = A.R, S = A.P.S;
    const int t = blockIdx.x * RATINGS_WAVES + w;
    if (t >= R) return;   // (wave uniform; no workgroup barrier below)
    uint32_t* hw = hist[w];
    uint32_t* bw = better[w];
    for (int i = lane; i < R; i += 64) {
        hw[i] = 0u;
        bw[i] = 0u;
    }
    dcl::wave_lds_order();
    const double* __restrict__ vt_row = A.ranked + (size_t)t * (size_t)S;
#pragma unroll 1
    for (int s0 = (int)blockIdx.y * 64; s0 < S; s0 += (int)gridDim.y * 64) {
        const int s = s0 + lane;
        const bool on = s < S;
        const double* __restrict__ col = A.ranked + (size_t)(on ? s : 0);   // (a lane past the end reads draw 0, unused)
        const double vt = vt_row[on ? s : 0];
        int rank = 0;
        // one opponent: the lanes ahead of it to its counter, this lane's rank (never counts u = t: rank <= R - 1)
        auto step = [&](int u, double vu) {
            const uint32_t ahead = (uint32_t)__popcll(__ballot(on && vt > vu));
            if (lane == 0) bw[u] += ahead;
            rank += (vu > vt || (vu == vt && u < t)) ? 1 : 0;
        };
        int u = 0;
#pragma unroll 1
        for (; u + 4 <= R; u += 4) {
            double vu[4];   // four rows in flight
#pragma unroll
            for (int j = 0; j < 4; ++j) vu[j] = col[(size_t)(u + j) * (size_t)S];
#pragma unroll
            for (int j = 0; j < 4; ++j) step(u + j, vu[j]);
        }
#pragma unroll 1
        for (; u < R; ++u) step(u, col[(size_t)u * (size_t)S]);
        if (on) atomicAdd(&hw[rank], 1u);
    }
    dcl::wave_lds_order();
    for (int i = lane; i < R; i += 64) {
        if (hw[i]) atomicAdd(&A.rank_count[(size_t)t * (size_t)R + (size_t)i], (int32_t)hw[i]);
        if (bw[i]) atomicAdd(&A.better_count[(size_t)t * (size_t)R + (size_t)i], (int32_t)bw[i]);
    }
}

}  // namespace dcr
