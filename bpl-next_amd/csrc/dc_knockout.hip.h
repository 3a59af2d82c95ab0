// dc_knockout.hip.h -- the extra-time knockout rule of simulate_tournament (knockout_rule="extra_time"): what
// the dc_tournament_et kernels (dc_tournament.hip.h: the shared body with ET = true) do in place of the redrawn
// level scoreline.
//
// Knockout match k of simulation j on draw s, between entries p (2m) and q (2m + 1), reads at most four
// threefry blocks (j, 0x40000000 | k << 5 | t) (dc_sampler.hip.h lists the counter space):
//   one leg    t = 0: the venue and orientation of dct::play (the host flags); not level: the winner is through.
//   two legs   t = 0: p at home, on = 1;  t = 1: q at home, on = 1 (the host flags are not read).  The aggregates
//              are x1 + y2 for p and y1 + x2 for q; level, and with away_goals set, the away goals y2 (p) and y1 (q)
//              decide when they differ.  Away goals are applied after the two legs only.
//   extra time t = 2: the venue and orientation of the only leg, or of leg 2, both rates times `scale`, the same
//              rho and the same sampler (tau is formed from the scaled rates, clipped as everywhere); the goals are
//              added to the totals.
//   shoot-out  t = 3: p is through iff unit_open(o0) < 1 / (1 + exp(-(strength[p] - strength[q]))); with equal
//              strengths that is exactly 0.5 and no word sits on the boundary.
// No redraws, no attempt cap.  All float64, contraction off; tests/knockout_ref.py restates it in numpy, operation
// for operation.  How each match was decided (DECIDED_*) is counted per round in a per-workgroup LDS histogram,
// flushed once per workgroup with global u64 atomics, and written per simulation by the match's lane when asked.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_posterior.hip.h"   // dcq::Posterior, log_rates_venue_branch
#include "dc_sampler.hip.h"     // dcr::sample_scoreline, unit_open
#include "nuts_dev.hip.h"       // nd::tf_block

namespace dck {

constexpr int KNOCKOUT_MAX_ROUNDS = 6;
constexpr int DECIDED_KINDS = 4;
constexpr int DECIDED_NORMAL = 0, DECIDED_AWAY_GOALS = 1, DECIDED_EXTRA_TIME = 2, DECIDED_SHOOTOUT = 3;
constexpr uint32_t BLOCK_LEG2 = 1u, BLOCK_EXTRA_TIME = 2u, BLOCK_SHOOTOUT = 3u;

struct KnockoutArgs {
    uint32_t legs_mask;                  // bit r: round r is a two-legged tie
    int away_goals;                      // 0 / 1
    double scale;                        // extra time: both rates times this, in (0, 1]
    const double* strength;              // [n] shoot-out strength per slot
    unsigned long long* decided_counts;  // [KNOCKOUT_MAX_ROUNDS, DECIDED_KINDS] (zeroed by the caller)
    uint8_t* sim_decided;                // [n_sims, 2^R - 1] or null
};

// the workgroup's [round][kind] histogram (only the extra-time instantiations call this, so only they hold it)
__device__ __forceinline__ uint32_t* decided_hist() {
    __shared__ uint32_t hist[KNOCKOUT_MAX_ROUNDS * DECIDED_KINDS];
    return hist;
}

// one leg of simulation j on draw s with a forced orientation: slot hs at home against slot as, at hs's venue
// (on) or a neutral one, both rates times c (1.0: exact).  TA: dct::TournamentArgs
template <class TA>
__device__ inline void play_leg(const TA& A, const uint32_t* sinfo, int s, uint32_t j, uint32_t ctr, int hs, int as,
                                bool on, double c, int* x, int* y) {
#pragma clang fp contract(off)
    const uint32_t ih = sinfo[hs], ia = sinfo[as];
    const int h = (int)(ih & 0xFFFFu), a = (int)(ia & 0xFFFFu);
    double eh, ea;
    const dcq::Posterior<double> P{A.S, A.T, A.C, A.attack, A.defence, nullptr, 0, A.home_attack, A.away_attack,
                                   A.home_defence, A.away_defence, A.conf, A.corr};
    dcq::log_rates_venue_branch(P, s, h, a, on, &eh, &ea);
    if (P.C) dcq::add_confederations(P, s, (int)((ih >> 16) & 0xFFu), (int)((ia >> 16) & 0xFFu), &eh, &ea);
    const double lh = exp(eh) * c, la = exp(ea) * c, rho = P.corr[s];
    uint32_t o0, o1;
    nd::tf_block(A.key_hi, A.key_lo, j, ctr, &o0, &o1);
    dcr::sample_scoreline(lh, la, rho, dcr::unit_open(o0), dcr::unit_open(o1), x, y);
}

// the decision ladder of one tie between entries p and q; ctr = KNOCKOUT_COUNTER | k << 5.  Returns the slot
// that goes through and how it was decided.  One loop over the blocks 0, (1,) 2: one copy of the sampler.
template <class TA>
__device__ inline int decide(const TA& A, const KnockoutArgs& K, const uint32_t* sinfo, int s, uint32_t j, uint32_t ctr,
                             int p, int q, bool two, int* how) {
#pragma clang fp contract(off)
    const bool hp = (sinfo[p] >> 24) & 1u, hq = (sinfo[q] >> 24) & 1u;
    int gp = 0, gq = 0, y1 = 0;
    for (uint32_t t = 0; t <= BLOCK_EXTRA_TIME; t = (t == 0 && !two) ? BLOCK_EXTRA_TIME : t + 1) {
        const bool q_home = two ? t >= BLOCK_LEG2 : (hq && !hp);
        const bool on = two || hp != hq;
        int x, y;
        play_leg(A, sinfo, s, j, ctr | t, q_home ? q : p, q_home ? p : q, on, t == BLOCK_EXTRA_TIME ? K.scale : 1.0, &x,
                 &y);
        gp += q_home ? y : x;
        gq += q_home ? x : y;
        if (two && t == 0) {
            y1 = y;   // q's away goals
            continue;
        }
        if (gp != gq) {
            *how = t == BLOCK_EXTRA_TIME ? DECIDED_EXTRA_TIME : DECIDED_NORMAL;
            return gp > gq ? p : q;
        }
        // leg 2 has q at home: y is p's away goals
        if (t == BLOCK_LEG2 && K.away_goals && y != y1) {
            *how = DECIDED_AWAY_GOALS;
            return y > y1 ? p : q;
        }
    }
    uint32_t o0, o1;
    nd::tf_block(A.key_hi, A.key_lo, j, ctr | BLOCK_SHOOTOUT, &o0, &o1);
    const double P = 1.0 / (1.0 + exp(-(K.strength[p] - K.strength[q])));
    *how = DECIDED_SHOOTOUT;
    return dcr::unit_open(o0) < P ? p : q;
}

}  // namespace dck
