// dc_tournament_live.hip.h -- a tournament on a day with group matches IN PROGRESS, and with weighted draws
// (simulate_tournament's `in_play`, `reweight` and `log_weights`): dc_live.hip.h's counterpart
// for the venue-form neutral models.  dc_tournament.hip.h plays every group fixture from 0-0 with the posterior draws
// at equal weight; here L of the group matches start from a state (a, b, t) -- current score in the LISTED order of
// the two sides and elapsed fraction -- and the draws carry weights: the joint likelihood of all the states and / or
// the caller's log weights.  Three launches on one stream, nothing comes back to the host between them:
//   live_cup_loglik   lane = draw on the TEAM-major venue tables, a sequential loop over the L states (wave-uniform
//       operands): l[s, m] = log Pois(a; lh t) + log Pois(b; la t) + log Z as dclive::live_loglik forms it, with the
//       rates of the tournament -- the venue BRANCH form and then the confederations, operation for operation as
//       dct::play forms them (contraction off: exp receives the same bits here and in the simulator).  The host has
//       decided the venue: a state arrives with its home / away model indices, its score in the home / away
//       orientation and the flag on.  lgamma from the 64-entry table in the arguments, a count of 0 takes no
//       logarithm.  L0[s] = sum_m l[s, m] in m order, L[s] = (L0[s] if reweight) + (lw[s] if given).  No LDS.
//   dclive::live_weights   as it is (dc_live.hip.h), through a dclive::LiveArgs whose draw count and buffers are
//       filled: the maximum, w = exp(L - max L), the fixed-association scan C, W, ess, log_evidence.
//   live_cup<H2H>, live_cup_et<H2H>, live_cup_table<H2H>, live_cup_table_et<H2H>   dc_tournament_body.hip.inc with
//       LIVE set -- the text of dct::dc_tournament, dc_tournament_et, cup_alloc and cup_alloc_et -- which adds
//       - the draw of simulation j: with weights SYSTEMATIC RESAMPLING on the scan, dc_season_live's formula on
//         the same block: U = unit_open(o0) of the threefry block (0, RESAMPLE_COUNTER) under the call's key,
//         step = W / N, target_j = min((j + U) step, W), s_j = min(#{s : C[s] < target_j}, S - 1) by
//         dclive::search_scan; without weights (C null) s_j = j mod S.  Every match of the simulation, in the groups
//         and in the knockout rounds, is played on that draw;
//       - after the F ordinary group fixtures, lane = match in play: fixture F + m of the concatenated list is
//         played from its state by dclive::sample_conditional on the block (j, F + m).  The venue is decided as for
//         any fixture; when the host is listed second the sides swap and the state's two goal counts swap with
//         them.  The final score is booked like any fixture's and, when asked, stored in the LISTED order;
//       - the draw of every simulation, stored by lane 0 when asked.
//       The ranking, the allocation fill, the knockout rounds and the histograms are the body's: they see another s.
// The kick-off kernels stay what they were: the flag is read through `if constexpr` only, and these are kernels of
// their own because a branch that dct's kernels never take still moved their code (DESIGN.md sections 42, 43).
// Integer atomics only, no floating-point atomics, vector stores only: every output is bit-identical run to run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_live.hip.h"         // dclive::sample_conditional, search_scan, RESAMPLE_COUNTER, LIVE_THREADS
#include "dc_tournament.hip.h"   // dct::TournamentArgs, LiveCup, play's rate form, the body

namespace dct {

// the draw of simulation j (every lane of the wave calls it: the search is wave uniform).  The call's offset U, W and
// the step are formed again for every simulation -- one threefry block, one load and one division beside a whole
// tournament -- and not held across the loop: these kernels have no register to spare
__device__ inline int live_draw(const TournamentArgs& A, const LiveCup& V, long long j, int lane) {
    if (!V.C) return (int)(j % A.S);
    uint32_t o0, o1;
    nd::tf_block(A.key_hi, A.key_lo, 0u, dclive::RESAMPLE_COUNTER, &o0, &o1);
    const double U = dcr::unit_open(o0), W = V.C[A.S - 1], step = W / (double)A.n_sims;
    const double target = fmin(((double)j + U) * step, W);
    return min(dclive::search_scan(V.C, A.S, target, lane), A.S - 1);
}
// match in play m of simulation j on draw s: dct::play's venue and rates, the state in the home / away orientation,
// the conditional sampler on the block (j, F + m); returns the FINAL scoreline in the (home, away) orientation and
// the home / away slots, and stores it in the listed order when asked
__device__ inline void play_live(const TournamentArgs& A, const LiveCup& V, const uint32_t* sinfo, int s, long long j,
                                 int m, int* hs, int* as, int* x, int* y) {
#pragma clang fp contract(off)
    const uint32_t sl = A.fix[V.F + m];
    const int p = (int)(sl & 0xFFu), q = (int)(sl >> 8);
    const uint32_t ip = sinfo[p], iq = sinfo[q];
    const bool hp = (ip >> 24) & 1u, hq = (iq >> 24) & 1u;
    const bool swap = hq && !hp;
    const uint32_t ih = swap ? iq : ip, ia = swap ? ip : iq;
    *hs = swap ? q : p;
    *as = swap ? p : q;
    const int h = (int)(ih & 0xFFFFu), a = (int)(ia & 0xFFFFu);
    double eh, ea;
    const dcq::Posterior<double> P{A.S, A.T, A.C, A.attack, A.defence, nullptr, 0, A.home_attack, A.away_attack,
                                   A.home_defence, A.away_defence, A.conf, A.corr};
    dcq::log_rates_venue_branch(P, s, h, a, hp != hq, &eh, &ea);
    if (P.C) dcq::add_confederations(P, s, (int)((ih >> 16) & 0xFFu), (int)((ia >> 16) & 0xFFu), &eh, &ea);
    const double lh = exp(eh), la = exp(ea), rho = P.corr[s];
    const uint32_t st = V.st_goals[m];
    const int gp = (int)(st & 0xFFu), gq = (int)(st >> 8);   // the listed sides' goals
    uint32_t o0, o1;
    nd::tf_block(A.key_hi, A.key_lo, (uint32_t)j, (uint32_t)(V.F + m), &o0, &o1);
    dclive::sample_conditional(lh, la, rho, swap ? gq : gp, swap ? gp : gq, 1.0 - V.st_t[m], dcr::unit_open(o0),
                               dcr::unit_open(o1), x, y);
    if (V.final_home) {
        V.final_home[(size_t)j * V.L + m] = (uint8_t)(swap ? *y : *x);
        V.final_away[(size_t)j * V.L + m] = (uint8_t)(swap ? *x : *y);
    }
}

}  // namespace dct

namespace dctl {

// the states as the host resolved them, and the draws' log weights: what live_cup_loglik reads and writes
struct CupStates {
    int S, L, C, reweight;
    const double* attack;         // TEAM-major [T, S], as the five below
    const double* defence;
    const double* home_attack;
    const double* away_attack;
    const double* home_defence;
    const double* away_defence;
    const double* conf;           // [C, S] or null
    const double* corr;           // [S]
    const uint32_t* st_side;      // [L]: home | away << 16 (model indices, after the venue swap)
    const uint32_t* st_state;     // [L]: a | b << 8 (home / away goals) | on << 16
    const uint32_t* st_conf;      // [L]: home | away << 16 confederations (read when C != 0)
    const double* st_t;           // [L] elapsed fraction
    const double* lw;             // [S] log weights, or null
    double* Lw;                   // [S] L
    double* L0;                   // [S] the state part alone
    double lgf[dclive::LIVE_MAX_GOALS + 1];   // lgf[k] = lgamma(k + 1)
};

// grid: ceil(S / LIVE_THREADS) workgroups
__global__ __launch_bounds__(dclive::LIVE_THREADS) void live_cup_loglik(CupStates A) {
#pragma clang fp contract(off)
    const int s = blockIdx.x * dclive::LIVE_THREADS + threadIdx.x;
    const size_t S = (size_t)A.S;
    if (s >= A.S) return;   // (no barrier below)
    const double rho = A.corr[s];
    double l0 = 0.0;
#pragma unroll 1
    for (int m = 0; m < A.L; ++m) {
        const uint32_t hw = A.st_side[m], g = A.st_state[m];   // (wave uniform)
        const int h = (int)(hw & 0xFFFFu), aw = (int)(hw >> 16);
        const int a = (int)(g & 0xFFu), b = (int)((g >> 8) & 0xFFu);
        const bool on = (g >> 16) & 1u;
        const double t = A.st_t[m], r = 1.0 - t;
        // dcq::log_rates_venue_branch and add_confederations on the team-major tables
        double eh = A.attack[h * S + s] - A.defence[aw * S + s];
        double ea = A.attack[aw * S + s] - A.defence[h * S + s];
        if (on) {
            eh = eh + (A.home_attack[h * S + s] - A.away_defence[aw * S + s]);
            ea = ea + (A.away_attack[aw * S + s] - A.home_defence[h * S + s]);
        }
        if (A.C) {
            const uint32_t cw = A.st_conf[m];
            const double dc = A.conf[(cw & 0xFFFFu) * S + s] - A.conf[(cw >> 16) * S + s];
            eh = eh + dc;
            ea = ea - dc;
        }
        const double lh = exp(eh), la = exp(ea);
        const double lhr = lh * r, lar = la * r;
        const double u0 = exp(-lhr), v0 = exp(-lar);
        const double c00 = rho * -(lh * la), c01 = rho * lh, c10 = rho * la, c11 = rho * -1.0;
        // Z: the tau cells at or beyond (a, b), each (f - 1) u_(x-a) v_(y-b), f - 1 = max(rho c, -1)
        const double u1 = u0 * lhr, v1 = v0 * lar;
        const double hx0 = a == 0 ? u0 : 0.0, hx1 = a == 0 ? u1 : (a == 1 ? u0 : 0.0);
        const double hy0 = b == 0 ? v0 : 0.0, hy1 = b == 0 ? v1 : (b == 1 ? v0 : 0.0);
        const double Z = 1.0 + (((fmax(c00, -1.0) * (hx0 * hy0) + fmax(c01, -1.0) * (hx0 * hy1)) +
                                 fmax(c10, -1.0) * (hx1 * hy0)) + fmax(c11, -1.0) * (hx1 * hy1));
        // a count of 0 takes no logarithm (t = 0 comes with 0-0)
        const double lt = log(t);
        const double pa = (a > 0 ? (double)a * (eh + lt) : 0.0) - lh * t - A.lgf[a];
        const double pb = (b > 0 ? (double)b * (ea + lt) : 0.0) - la * t - A.lgf[b];
        l0 = l0 + ((pa + pb) + log(Z));
    }
    A.L0[s] = l0;
    A.Lw[s] = (A.reweight ? l0 : 0.0) + (A.lw ? A.lw[s] : 0.0);
}

// The eight simulators: the body of dc_tournament.hip.h's kernels with LIVE set, launched in their place when, and
// only when, weights are in force or a match is in play.  H2H, ET and the launch shapes are those kernels'; `_table`
// is the body under a best-of-rest allocation table (ALLOC).
// The second launch bound asks for four waves per SIMD, 128 VGPRs: the conditional sampler beside the redraw loop
// took four of the eight to 130 .. 137 without it, one wave per SIMD fewer than their kick-off twins hold.
constexpr int LIVE_CUP_WAVES_PER_SIMD = 4;
template <bool H2H>
__global__ __launch_bounds__(64 * dct::TOURNAMENT_WAVES, LIVE_CUP_WAVES_PER_SIMD) void live_cup(dct::TournamentArgs A, dch::PairArgs H, dct::LiveCup V) {
    using namespace dct;
    constexpr bool ET = false, ALLOC = false, LIVE = true;
    const dck::KnockoutArgs K{};   // (named by the discarded extra-time statements; never read)
#include "dc_tournament_body.hip.inc"
}
template <bool H2H>
__global__ __launch_bounds__(64 * dct::TOURNAMENT_WAVES, LIVE_CUP_WAVES_PER_SIMD) void live_cup_et(dct::TournamentArgs A, dch::PairArgs H,
                                                                          dck::KnockoutArgs K, dct::LiveCup V) {
    using namespace dct;
    constexpr bool ET = true, ALLOC = false, LIVE = true;
#include "dc_tournament_body.hip.inc"
}
template <bool H2H>
__global__ __launch_bounds__(64 * dct::TOURNAMENT_WAVES, LIVE_CUP_WAVES_PER_SIMD) void live_cup_table(dct::TournamentArgs A, dch::PairArgs H,
                                                                             dct::LiveCup V) {
    using namespace dct;
    constexpr bool ET = false, ALLOC = true, LIVE = true;
    const dck::KnockoutArgs K{};
#include "dc_tournament_body.hip.inc"
}
template <bool H2H>
__global__ __launch_bounds__(64 * dct::TOURNAMENT_WAVES, LIVE_CUP_WAVES_PER_SIMD) void live_cup_table_et(dct::TournamentArgs A, dch::PairArgs H,
                                                                                dck::KnockoutArgs K, dct::LiveCup V) {
    using namespace dct;
    constexpr bool ET = true, ALLOC = true, LIVE = true;
#include "dc_tournament_body.hip.inc"
}

}  // namespace dctl
